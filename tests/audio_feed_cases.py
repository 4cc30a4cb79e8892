"""The op-level cases of sagen_assemble_audio (include/sagen.h), shared by tests/test_cpu_twin_audio_feed.py (the CPU twin, through
ctypes on numpy arrays) and tests/test_gpu_audio_feed.py (the device library, through torch): the inputs, and the expected outputs made
by explicit numpy - the rows of a window found with Python integers (no int64 to overflow) as an intersection of intervals, not row by
row as the kernel does; the rotation elementwise, c * Y + s * X and c * X - s * Y in float64, never `.dot` (a BLAS may fuse or reorder);
one `.astype(float32)` at the end.  Everything is compared as bit patterns: there is no tolerance anywhere in these cases.

A `call` is   call(samples [n_samples, channels] int16 | float32 | float64, lead int32 [n_out], read_from int64 [n_out],
                   count int32 [n_out], rot float64 [n_out, 2] or None, size, want, t_off, t_len, offset=0)
              -> {name: numpy float32} for the names in `want`: 'full' [n_out, size, channels], 'mono' [n_out, size],
                 'target' [n_out, t_len, channels - 1]
`offset`: the samples are to be handed over at a base that lies `offset` elements behind an aligned allocation.  The outputs are
filled with NaN before the call, so an element the op leaves out shows."""
import numpy as np

from util import rng

N_SAMPLES = 100
SIZES = [37, 255, 256, 257]                     # below one workgroup of 256 rows, one short of it, exactly it, one more
CHANNELS = [1, 2, 3, 4, 9]
DTYPES = [np.int16, np.float32, np.float64]     # sample_type 0, 1, 2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
ANGLES = [-np.pi, 0.0, 0.7853981633974483 * 1.37, np.nextafter(np.pi, 0.0)]     # -pi, 0, an arbitrary one, the largest double below pi


def sample_type(dtype):
    return DTYPES.index(np.dtype(dtype).type)


def samples_of(n, channels, dtype, seed=0):
    r = rng(1000 * channels + 10 * sample_type(dtype) + seed)
    if np.dtype(dtype) == np.int16:
        s = r.integers(-32768, 32768, size=(n, channels)).astype(np.int16)
        if n:
            s[0, 0], s[n - 1, channels - 1] = -32768, 32767
        return s
    s = (0.6 * r.normal(size=(n, channels))).astype(dtype)             # float64: values that are no float32, the narrowing rounds
    if n > 2:
        s[1, :] = -0.0                                                  # kept where nothing rotates
    return s


def windows(size, n=N_SAMPLES):
    """(lead, read_from, count) rows: what feeder.window_table writes, and what it never would"""
    return [
        (0, 0, size),                           # runs off the end of the samples when size > n
        (5, 10, size - 5),                      # a lead
        (0, n - 20, 20),                        # a trail: the count stops the window
        (0, n - 20, size),                      # ... and the end of the samples does
        (3, 7, 0),                              # count = 0: a padding window
        (size, 0, 10), (size + 7, 3, size),     # lead >= size
        (0, -4, size), (2, -n - 50, size),      # negative read_from: the rows before sample 0 are zeros
        (0, n, 5), (0, n + 1000, size),         # read_from >= n_samples
        (2, I64_MIN, 50), (0, I64_MIN + 1, size), (0, I64_MAX, 50), (1, I64_MAX - 3, size),
        (-3, 4, 20), (-size, 0, 2 * size),      # negative lead: the window starts inside the run
        (4, 4, -5), (0, 0, I32_MIN),            # negative count
        (I32_MIN, 0, I32_MAX), (I32_MAX, 0, I32_MAX), (-1, I64_MAX, I32_MAX), (I32_MIN, I64_MIN, I32_MAX),
        (1, 1, size - 1),
    ]


def columns(rows):
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.int32))


def rot_of(angles):
    a = np.asarray(angles, np.float64)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], 1))


def values(samples):
    """feeder.load_wav's values of stored samples"""
    if samples.dtype == np.int16:
        return samples.astype(np.float64) / 32768.0
    return samples.astype(np.float64)


def expected(samples, lead, read_from, count, rot, size, t_off, t_len):
    n, channels = samples.shape
    vals = values(samples)
    full = np.zeros((len(lead), size, channels), np.float64)
    live = np.zeros((len(lead), size), bool)
    for i in range(len(lead)):
        ld, rf, cnt = int(lead[i]), int(read_from[i]), int(count[i])   # Python integers from here on
        lo = max(0, ld, ld - rf)                # j >= 0;  k = j - ld >= 0;  rf + k >= 0
        hi = min(size, ld + cnt, ld - rf + n)   # j < size;  k < cnt;  rf + k < n
        if lo < hi:
            full[i, lo:hi] = vals[rf + lo - ld:rf + hi - ld]
            live[i, lo:hi] = True
    if rot is not None:
        c, s = rot[:, 0][:, None], rot[:, 1][:, None]
        y, x = full[..., 1].copy(), full[..., 3].copy()
        full[..., 1] = c * y + s * x
        full[..., 3] = c * x - s * y
        full[~live] = 0.0                       # padding rows stay 0.0: they are not rotated (-1 * 0.0 would be -0.0)
    full = full.astype(np.float32)
    out = {'full': full, 'mono': np.ascontiguousarray(full[..., 0])}
    if t_len:
        out['target'] = np.ascontiguousarray(full[:, t_off:t_off + t_len, 1:])
    return out


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    g, w = got.view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, '%d of %d elements differ, the first at %d (%r, not %r)' % (bad.size, got.size, bad[0], got.reshape(-1)[bad[0]],
                                                                                      want.reshape(-1)[bad[0]])


def check(call, samples, rows, rot, size, want, t_off=0, t_len=0, offset=0):
    lead, read_from, count = columns(rows)
    got = call(samples, lead, read_from, count, rot, size, want, t_off, t_len, offset=offset)
    exp = expected(samples, lead, read_from, count, rot, size, t_off, t_len)
    assert sorted(got) == sorted(want)
    for name in want:
        same_bits(got[name], exp[name])
    return got


def target_ranges(size):
    """(t_off, t_len): both ends, one row and all rows"""
    return [(0, 1), (size - 1, 1), (0, size), (size // 3, size - size // 3), (0, size // 2)]


def check_shape(call, size, channels, dtype):
    """every window kind at one (size, channels, sample type): each output alone, all three together, the target rows at both ends"""
    s = samples_of(N_SAMPLES, channels, dtype)
    rows = windows(size)
    got = check(call, s, rows, None, size, ('full',))
    assert np.count_nonzero(got['full'][0]) > 0.9 * min(size, N_SAMPLES) * channels           # not vacuous
    if np.dtype(dtype) != np.int16:
        assert np.signbit(got['full'][0, 1]).all()                                            # the row of -0.0 is still -0.0
    check(call, s, rows, None, size, ('mono',))
    if channels >= 2:
        for t_off, t_len in target_ranges(size):
            check(call, s, rows, None, size, ('target',), t_off, t_len)
        check(call, s, rows, None, size, ('full', 'mono', 'target'), size // 3, size - size // 3)
        check(call, s, rows, None, size, ('mono', 'target'), size - 1, 1)
    if channels == 4:
        rot = rot_of([ANGLES[i % len(ANGLES)] for i in range(len(rows))])
        got = check(call, s, rows, rot, size, ('full', 'mono', 'target'), 0, size)
        plain = expected(s, *columns(rows), None, size, 0, size)
        assert not np.array_equal(got['full'][2], plain['full'][2])                           # the arbitrary angle does rotate
        for want in (('full',), ('mono',), ('target',)):
            check(call, s, rows, rot, size, want, size // 2, size - size // 2)


def check_grid_strides(call):
    """1030 windows of 5 rows: more than one pass of the grid's item rows"""
    s = samples_of(N_SAMPLES, 4, np.int16, seed=1)
    r = rng(11)
    rows = [(int(l), int(f), int(c)) for l, f, c in zip(r.integers(-2, 4, 1030), r.integers(-3, N_SAMPLES + 2, 1030), r.integers(-1, 7, 1030))]
    rot = rot_of(r.uniform(-np.pi, np.pi, 1030))
    got = check(call, s, rows, rot, 5, ('full', 'mono', 'target'), 1, 3)
    assert np.count_nonzero(got['mono'][1024:]) > 0
    s3 = samples_of(N_SAMPLES, 3, np.float32, seed=1)
    check(call, s3, rows, None, 5, ('full', 'mono', 'target'), 0, 5)


def check_offset_base(call):
    """4 channels at a base that is aligned to its element only: the element-wise path, the same bits"""
    for dtype in DTYPES:
        s = samples_of(N_SAMPLES, 4, dtype, seed=2)
        rows = windows(257)
        rot = rot_of([ANGLES[(i + 1) % len(ANGLES)] for i in range(len(rows))])
        for r in (None, rot):
            a = check(call, s, rows, r, 257, ('full', 'mono', 'target'), 100, 57, offset=1)
            b = check(call, s, rows, r, 257, ('full', 'mono', 'target'), 100, 57, offset=0)
            for name in a:
                same_bits(a[name], b[name])


# ---- feeder.DeviceAudio against the host feeder over an ambix folder ---------------------------------------------------------------
RATE, CONTEXT, SIZE = 48000, 1.0, 52799
T_OFF, T_LEN = 24000, 4800                      # the centre 0.1 s: train.py:107-111 / Evaluator._finish
TIMES = [0.5, 0.6, 1.0, 1.7, 2.4, 2.9, 0.0, 3.3]                     # leads, whole windows, trails, a window that starts before the clip
ROTATIONS = [-np.pi, None, 0.3, float(np.nextafter(np.pi, 0.0)), -2.2, 1.0, None, 3.0]
ROTATION_SEED = 5


def make_ambix(folder, subtype='PCM_16', short_last=0, secs=3, seed=ROTATION_SEED):
    """`secs` one-second pieces of 4 channels; the last one `short_last` samples short"""
    import os
    from spatialaudiogen_amd import feeder as F
    os.makedirs(folder)
    audio = np.clip(0.3 * rng(seed).normal(size=(secs * RATE, 4)), -1, 1)
    for i in range(secs):
        piece = audio[i * RATE:(i + 1) * RATE - (short_last if i == secs - 1 else 0)]
        F.save_wav(os.path.join(folder, '%06d.wav' % i), piece, RATE, subtype)
    return folder


def host_windows(folder, rotations=None):
    """WavPieces.assemble(...).astype(float32) of TIMES: what evaluate and train feed from"""
    from spatialaudiogen_amd import feeder as F
    wp = F.WavPieces(folder, RATE)
    tab = F.window_table(TIMES, CONTEXT, SIZE, RATE, wp.num_frames)
    rotations = rotations or [None] * len(TIMES)
    return np.stack([wp.assemble(tab, k, SIZE, rotations[k]) for k in range(len(TIMES))], 0).astype(np.float32)


def plain_windows(folder):
    """(float64 windows [n, size, 4] of TIMES by the host feeder, no rotation; which of their rows hold samples [n, size])"""
    from spatialaudiogen_amd import feeder as F
    wp = F.WavPieces(folder, RATE)
    tab = F.window_table(TIMES, CONTEXT, SIZE, RATE, wp.num_frames)
    plain = np.stack([wp.assemble(tab, k, SIZE) for k in range(len(TIMES))], 0)
    j = np.arange(SIZE)[None, :]
    return plain, (j >= tab.lead[:, None]) & (j < (tab.lead + tab.read_count)[:, None])


def oracle_rotated(plain, live, rotations):
    """the fixed-order rotation of the sample rows of float64 windows [n, size, 4] (padding rows stay 0.0), then the float32 cast;
    None: no rotation"""
    out = plain.copy()
    for k, r in enumerate(rotations):
        if r is not None:
            c, s = np.cos(r), np.sin(r)
            y, x = plain[k, :, 1], plain[k, :, 3]
            out[k, :, 1] = np.where(live[k], c * y + s * x, 0.0)
            out[k, :, 3] = np.where(live[k], c * x - s * y, 0.0)
    return out.astype(np.float32)


def ordered(x):
    """float32 bit patterns as integers in the order of the values (one step = one ulp; -0.0 and +0.0 coincide)"""
    i = x.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def within_one_ulp(got, want, cap=1e-4):
    """every element within 1 float32 ulp, at most `cap` of them different at all"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    d = np.abs(ordered(got) - ordered(want))
    assert d.max() <= 1, 'an element is %d ulps off' % d.max()
    assert np.count_nonzero(d) <= cap * d.size, '%d of %d elements differ' % (np.count_nonzero(d), d.size)


def check_device_audio_plain(device, folder):
    """no rotation: bit-identical to the host feeder, the three outputs of one launch and the zero windows of pad_to"""
    from spatialaudiogen_amd import feeder as F
    da = F.DeviceAudio(folder, RATE, device=device)
    wp = F.WavPieces(folder, RATE)
    assert (da.num_frames, da.num_channels, da.rate, da.num_files) == (wp.num_frames, wp.num_channels, wp.rate, wp.num_files)
    want = host_windows(folder)
    n = len(TIMES)
    full, mono, target = da.batch(TIMES, CONTEXT, SIZE, pad_to=n + 2, want=('full', 'mono', 'target'), t_off=T_OFF, t_len=T_LEN)
    assert full.device.type == device and tuple(mono.shape) == (n + 2, SIZE, 1) and tuple(target.shape) == (n + 2, T_LEN, 3)
    full, mono, target = full.cpu().numpy(), mono.cpu().numpy(), target.cpu().numpy()
    same_bits(full[:n], want)
    same_bits(mono[:n, :, 0], np.ascontiguousarray(want[..., 0]))
    same_bits(target[:n], np.ascontiguousarray(want[:, T_OFF:T_OFF + T_LEN, 1:]))
    assert not full[n:].any() and not mono[n:].any() and not target[n:].any()
    (mono_only,) = da.batch(TIMES[:3], CONTEXT, SIZE)
    same_bits(mono_only.cpu().numpy()[:, :, 0], np.ascontiguousarray(want[:3, :, 0]))
    assert tuple(da.batch([], CONTEXT, SIZE)[0].shape) == (0, SIZE, 1)
    return da


def check_device_audio_rotated(device, folder):
    from spatialaudiogen_amd import feeder as F
    da = F.DeviceAudio(folder, RATE, device=device)
    (full,) = da.batch(TIMES, CONTEXT, SIZE, rotations=ROTATIONS, want=('full',))
    host = host_windows(folder, ROTATIONS)
    assert not np.array_equal(host, host_windows(folder))
    within_one_ulp(full.cpu().numpy(), host)
    plain, live = plain_windows(folder)
    same_bits(full.cpu().numpy(), oracle_rotated(plain, live, ROTATIONS))       # and exactly the fixed order
    one = da.batch(TIMES[:2], CONTEXT, SIZE, rotations=0.3, want='full')[0].cpu().numpy()
    same_bits(one, oracle_rotated(plain[:2], live[:2], [0.3, 0.3]))


def check_no_samples(call):
    """n_samples == 0 with a null `samples`: every window is padding, whatever the table says"""
    for channels in (1, 4):
        s = np.zeros((0, channels), np.float32)
        want = ('full', 'mono', 'target') if channels > 1 else ('full', 'mono')
        got = check(call, s, windows(37, 0), None, 37, want, 3, 30 if channels > 1 else 0)
        assert all(not g.any() and not np.signbit(g).any() for g in got.values())
