"""An independent statement of what sagen_png_filter writes, and the frames the PNG tests share.  numpy only, row by row, no code shared
with spatialaudiogen_amd or csrc/png_core.h.

The rule (include/sagen.h): each row takes, of None / Sub / Up / Average / Paeth, the filter whose sum of min(v, 256 - v) over the
filtered bytes is smallest, the lowest number among equals; the row above row 0 is zeros; bytes left of the row are zeros."""
import numpy as np

B = 16384           # input bytes per deflate block (include/sagen.h)
POISON = 0xA5


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_row(cur, up, bpp):
    """cur, up: the row and the one above as int arrays [w bpp] -> (filter number, filtered uint8 row)."""
    cur, up = cur.astype(np.int64), up.astype(np.int64)
    a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
    c = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
    a, c = a[:cur.size], c[:cur.size]
    candidates = [cur, cur - a, cur - up, cur - (a + up) // 2, cur - _paeth(a, up, c)]
    best, least = None, None
    for number, cand in enumerate(candidates):
        v = np.mod(cand, 256)
        cost = int(np.minimum(v, 256 - v).sum())
        if least is None or cost < least:
            best, least = (number, v.astype(np.uint8)), cost
    return best


def filter_rows(frames):
    """frames uint8 [n, h, w, 3] or [n, h, w] -> [n, h, 1 + w c] as the op writes them."""
    frames = np.asarray(frames)
    bpp = 3 if frames.ndim == 4 else 1
    n, h = frames.shape[:2]
    flat = frames.reshape(n, h, -1)
    out = np.zeros((n, h, 1 + flat.shape[2]), np.uint8)
    for f in range(n):
        for y in range(h):
            up = flat[f, y - 1] if y else np.zeros_like(flat[f, y])
            number, row = filter_row(flat[f, y], up, bpp)
            out[f, y, 0] = number
            out[f, y, 1:] = row
    return out


def unfilter(rows, w, comps):
    """The decoder's side, for the oracle's own check: rows [h, 1 + w c] -> pixels [h, w c]."""
    h = rows.shape[0]
    out = np.zeros((h, w * comps), np.int64)
    for y in range(h):
        t, row = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(w * comps, np.int64)
        for x in range(w * comps):
            a = out[y, x - comps] if x >= comps else 0
            c = up[x - comps] if x >= comps else 0
            pred = [0, a, up[x], (a + up[x]) // 2, int(_paeth(np.int64(a), np.int64(up[x]), np.int64(c)))][t]
            out[y, x] = (row[x] + pred) % 256
    return out.astype(np.uint8)


def natural(seed, h=224, w=448):
    """A deterministic frame with the spectrum of a photograph: per channel white noise shaped in the Fourier domain by
    1 / (1e-3 + |k|)^1.5, scaled to 0..255, plus N(0, 2) noise, rounded and clipped.  uint8 [h, w, 3]."""
    rs = np.random.RandomState(seed)
    ky, kx = np.meshgrid(np.fft.fftfreq(h), np.fft.fftfreq(w), indexing='ij')
    shape = 1. / (1e-3 + np.sqrt(ky * ky + kx * kx)) ** 1.5
    out = np.zeros((h, w, 3), np.uint8)
    for c in range(3):
        field = np.real(np.fft.ifft2(np.fft.fft2(rs.randn(h, w)) * shape))
        field = (field - field.min()) / (field.max() - field.min()) * 255.
        out[:, :, c] = np.clip(np.rint(field + rs.randn(h, w) * 2.), 0, 255).astype(np.uint8)
    return out


# ---- the small cases (tests/test_gpu_png.py, tools/make_png_fixture.py, tests/test_png_host.py) --------------------------------------
def filter_cases():
    """name -> frames [n, h, w, 3] or [n, h, w]."""
    rs = np.random.RandomState(5)
    cases = {}
    for h, w in ((1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (17, 9), (9, 17)):
        cases['grey_%dx%d' % (h, w)] = rs.randint(0, 256, (2, h, w)).astype(np.uint8)
        cases['rgb_%dx%d' % (h, w)] = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    # gradients (Sub leaves 3 a byte) under rows of noise, which make Up, Average and Paeth useless for them
    grad = rs.randint(0, 256, (6, 40, 3))
    grad[1::2] = (3 * np.arange(40) + 4)[None, :, None]
    cases['gradient_sub_wins'] = grad.astype(np.uint8)[None]
    row = rs.randint(0, 256, (1, 300, 3))
    cases['repeated_rows_up_wins'] = np.repeat(row, 5, 0).astype(np.uint8)[None]
    # one grey row 0, 2: None costs 2, Sub 2, Up 2, Average 0 + 2, Paeth 2 - every filter ties, None wins; the row below repeats it: Up 0 wins
    cases['tie'] = np.array([[[0, 2], [0, 2], [1, 255]]], np.uint8)
    return cases


def _no_two_alike(counts, values):
    """A string in which value i stands counts[i] times and no two neighbours are equal (the largest count is below half)."""
    order = np.argsort(-np.asarray(counts), kind='stable')
    flat = np.concatenate([np.full(counts[i], values[i], np.uint8) for i in order])
    out = np.zeros(flat.size, np.uint8)
    half = (flat.size + 1) // 2
    out[0::2] = flat[:half]
    out[1::2] = flat[half:]
    assert (out[1:] != out[:-1]).all()
    return out


def deflate_cases():
    """name -> uint8 [n, length]: the strings of one call."""
    rs = np.random.RandomState(9)
    cases = {}
    for length in (0, 1, 2, 3, B - 1, B, B + 1, 2 * B + 5):
        sparse = (rs.randint(0, 5, length) * 50).astype(np.uint8)
        sparse[rs.rand(length) < 0.7] = 0                                   # runs of zeros of every short length, a few symbols between them
        cases['length_%d' % length] = np.stack([sparse, np.zeros(length, np.uint8)], 0)
    for m in (1, 2, 3, 4, 258, 259, 260, 261, 262, 600):
        inside = np.concatenate([[7, 9], np.full(m, 200), [9, 7]]).astype(np.uint8)
        lead = B - m // 2 - 1
        head = (np.arange(lead) % 251 + 1).astype(np.uint8)                 # no two neighbours alike, nothing like the run's byte 0
        across = np.concatenate([head, np.zeros(m, np.uint8), [1, 2, 3]]).astype(np.uint8)
        cases['run_%d' % m] = inside[None]
        cases['run_%d_across_blocks' % m] = across[None]
    cases['zeros'] = np.zeros((1, 3 * B), np.uint8)
    # 258 blocks, more than the 256 whose positions one pass of the placing walk holds; a stored block among fixed ones moves every
    # block behind it to a byte boundary plus its own bits
    many = np.zeros(257 * B + 3, np.uint8)
    many[100 * B:101 * B] = rs.randint(0, 256, B)
    many[200 * B + 5::4099] = 77
    cases['many_blocks'] = many[None]
    cases['uniform_random'] = rs.randint(0, 256, (2, B + 100)).astype(np.uint8)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 4180
    cases['fibonacci'] = _no_two_alike(fib, [3 * i + 1 for i in range(17)])[None]
    return cases


RECORDED = ('length_0', 'length_1', 'length_2', 'length_3', 'run_1', 'run_2', 'run_3', 'run_4', 'run_258', 'run_259', 'run_260', 'run_261',
            'run_262', 'run_600', 'run_3_across_blocks', 'run_600_across_blocks', 'zeros', 'fibonacci', 'length_%d' % (B + 1), 'many_blocks')
