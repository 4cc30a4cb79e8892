"""PNG frames encoded on the device (csrc/png.hip through png.filter_rows / png.deflate / png.PngEncoder and the --encode device flag of
overlay and deploy).  Everything here is exact: the filtered rows equal the oracle's (tests/png_oracle.py) byte for byte, zlib's inflate
returns every input, the recorded streams (tests/golden/png_v1.npz, as the CPU twin wrote them) come back bit for bit, PIL decodes every
file to the pixels it was given.  The arithmetic is integer end to end (include/sagen.h), so there is no tolerance to choose.

The size conditions are those of the scheme, not of this code: a per-block Huffman code plus runs at distance 1 gives 178.7 KB on
natural(1) where PIL's default save gives 183.2 KB (5 % of margin for the plain block headers and the heuristic length limit); one
colour is nothing but runs (zlib's Z_RLE: 671 bytes; raw / 64 = 4 707); noise is stored, at the bound.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_png_host.py)."""
import ctypes as C
import io
import os
import zlib

import numpy as np
import pytest

import png_oracle as PO
from util import ensure_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'png_v1.npz')
OP_CASES = ('test_filter_rows_equal_the_oracle or test_deflate_case or test_capacity_rule or test_refusals_leave_every_output_untouched or '
            'test_recorded_streams_are_reproduced or test_encoder_files_open_in_pil or test_encoder_retry_at_the_bound')
POISON = PO.POISON
B = PO.B
FILTER_CASES = PO.filter_cases()
DEFLATE_CASES = PO.deflate_cases()


def _dev():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    if _lib.IS_CPU_TWIN:
        return 'cpu'
    import torch
    assert torch.cuda.is_available()
    return 'cuda'


def _t(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).to(_dev())


def _bound(length):
    from spatialaudiogen_amd import _lib
    return int(_lib.lib().sagen_deflate_max_bytes(length))


def _deflate(strings, stride=None, out=None):
    """Through the C ABI: one copy in, one call -> (out, sizes, status) as numpy; `out` starts as POISON."""
    import torch
    from spatialaudiogen_amd import png
    strings = np.ascontiguousarray(strings)
    n, length = strings.shape
    stride = stride or (_bound(length) + 3) // 4 * 4
    if out is None:
        out = torch.full((n, stride), POISON, dtype=torch.uint8, device=_dev())
    o, sizes, status = png.deflate(_t(strings), stride, out)
    return o.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()


def _inflate(stream):
    d = zlib.decompressobj()
    data = d.decompress(bytes(stream))
    assert d.eof and not d.unused_data
    return data


def _same_pixels(data, frame):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()                                                           # (reads every chunk: a bad CRC raises)
    assert im.mode == ('RGB' if frame.ndim == 3 else 'L') and np.array_equal(np.asarray(im), frame)


@pytest.mark.parametrize('name', sorted(FILTER_CASES))
def test_filter_rows_equal_the_oracle(name):
    from spatialaudiogen_amd import png
    frames = FILTER_CASES[name]
    want = PO.filter_rows(frames)
    got = png.filter_rows(_t(frames)).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), name
    if name == 'gradient_sub_wins':
        assert (want[:, 1::2, 0] == 1).all()
    if name == 'repeated_rows_up_wins':
        assert (want[:, 1:, 0] == 2).all()
    if name == 'tie':
        assert want[0, :, 0].tolist()[:2] == [0, 2]
    comps = 3 if frames.ndim == 4 else 1
    assert np.array_equal(PO.unfilter(want[0], frames.shape[2], comps), frames[0].reshape(frames.shape[1], -1))


@pytest.mark.parametrize('name', sorted(DEFLATE_CASES))
def test_deflate_case(name):
    strings = DEFLATE_CASES[name]
    n, length = strings.shape
    bound = _bound(length)
    assert 0 < bound <= length + 6 * max(1, -(-length // B)) + 7
    out, sizes, status = _deflate(strings)
    assert not status.any(), (name, status)
    for f in range(n):
        assert _inflate(out[f, :sizes[f]]) == strings[f].tobytes(), (name, f)
        assert 8 <= sizes[f] <= bound and (out[f, sizes[f]:] == POISON).all(), (name, f, sizes[f], bound)
    if name == 'zeros':
        assert sizes[0] < 400                                          # a literal and 64 matches a block
    if name == 'uniform_random':
        assert (sizes > length).all()                                   # stored: nothing to gain
    if name.startswith('run_') and not name.endswith('blocks'):
        assert sizes[0] < 8 + 6 + 10                                    # 2 + 4 framing, four literals, the run in at most 4 + 3 tokens, fixed codes


def test_capacity_rule():
    """A stride below what the noise needs: CAPACITY with the true size, the frames around it exact, nothing past any row.  The rows of
    `out` lie inside a larger poisoned tensor."""
    import torch
    rs = np.random.RandomState(3)
    strings = np.stack([np.zeros(1000, np.uint8), rs.randint(0, 256, 1000).astype(np.uint8), np.full(1000, 9, np.uint8),
                        rs.randint(0, 256, 1000).astype(np.uint8)], 0)
    full, full_sizes, _ = _deflate(strings)
    assert [s > 64 for s in full_sizes] == [False, True, False, True]
    big = torch.full((16 + 4 * 64 + 64,), POISON, dtype=torch.uint8, device=_dev())
    out, sizes, status = _deflate(strings, 64, big[16:16 + 4 * 64].view(4, 64))
    assert status.tolist() == [0, 1, 0, 1] and sizes.tolist() == full_sizes.tolist()
    for j in (0, 2):
        assert out[j, :sizes[j]].tobytes() == full[j, :sizes[j]].tobytes() and (out[j, sizes[j]:] == POISON).all()
    guard = big.cpu().numpy()
    assert (guard[:16] == POISON).all() and (guard[16 + 4 * 64:] == POISON).all()
    # a stride of exactly what the frame needs is enough
    need = (int(full_sizes[1]) + 3) // 4 * 4
    out, sizes, status = _deflate(strings[1:2], need)
    assert status.tolist() == [0] and _inflate(out[0, :sizes[0]]) == strings[1].tobytes()


def test_refusals_leave_every_output_untouched():
    import torch
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd.ops import _stream
    dev = _dev()
    l = _lib.lib()
    data = _t(np.arange(600, dtype=np.uint8).reshape(2, 300))
    frames = _t(np.arange(2 * 5 * 4 * 3, dtype=np.uint8).reshape(2, 5, 4, 3))
    rows = torch.full((2, 5, 13), POISON, dtype=torch.uint8, device=dev)
    out = torch.full((2, 512), POISON, dtype=torch.uint8, device=dev)
    sizes = torch.full((2,), -1, dtype=torch.int32, device=dev)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev)
    need = l.sagen_deflate_scratch_bytes(2, 300, 512)
    assert need >= 2 * (286 * 4 + 300) and need % 16 == 0
    scratch = torch.empty(need // 8, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def deflate(d=ptr(data), n=2, length=300, o=ptr(out), stride=512, sz=ptr(sizes), st=ptr(status), sc=ptr(scratch), sc_bytes=need):
        return l.sagen_deflate(d, n, length, o, stride, sz, st, sc, sc_bytes, _stream())

    def filt(fr=ptr(frames), n=2, w=4, h=5, comps=3, r=ptr(rows)):
        return l.sagen_png_filter(fr, n, w, h, comps, r, _stream())

    for kw in (dict(d=None), dict(o=None), dict(sz=None), dict(st=None), dict(sc=None)):
        assert deflate(**kw) == -1, kw
    for kw in (dict(n=-1), dict(length=-1), dict(stride=0), dict(stride=-4), dict(stride=510), dict(o=C.c_void_p(out.data_ptr() + 2)),
               dict(sz=C.c_void_p(sizes.data_ptr() + 2)), dict(st=C.c_void_p(status.data_ptr() + 1)), dict(sc=C.c_void_p(scratch.data_ptr() + 8))):
        assert deflate(**kw) == -2, (kw, l.sagen_last_error())
    for kw in (dict(n=65536), dict(length=(1 << 28) + 1), dict(stride=(1 << 28) + 4)):
        assert deflate(**kw) == -3, (kw, l.sagen_last_error())
    assert deflate(sc_bytes=need - 1) == -5 and deflate(sc_bytes=0) == -5
    assert l.sagen_deflate_scratch_bytes(0, 300, 512) == 0 and l.sagen_deflate_scratch_bytes(2, 300, 510) == 0
    assert l.sagen_deflate_scratch_bytes(2, -1, 512) == 0 and l.sagen_deflate_max_bytes(-1) == 0 and l.sagen_deflate_max_bytes((1 << 28) + 1) == 0
    assert l.sagen_deflate_max_bytes(300) == 300 + 6 + 6 and l.sagen_deflate_max_bytes(4 * B + 1) == 4 * B + 1 + 6 + 27
    for kw in (dict(fr=None), dict(r=None)):
        assert filt(**kw) == -1, kw
    for kw in (dict(n=-1), dict(w=0), dict(h=0), dict(w=-3)):
        assert filt(**kw) == -2, (kw, l.sagen_last_error())
    for kw in (dict(comps=2), dict(comps=4), dict(comps=0), dict(w=16385), dict(h=16385), dict(n=65536)):
        assert filt(**kw) == -3, (kw, l.sagen_last_error())
    assert deflate(n=0) == 0 and deflate(n=0, d=None, o=None, sz=None, st=None, sc=None) == 0 and filt(n=0) == 0 and filt(n=0, fr=None, r=None) == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((rows == POISON).all()) and sizes.tolist() == [-1, -1] and status.tolist() == [-1, -1]
    assert deflate() == 0 and filt() == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert status.tolist() == [0, 0] and [_inflate(o[f, :sizes[f]]) for f in range(2)] == [bytes(r) for r in data.cpu().numpy()]
    assert np.array_equal(rows.cpu().numpy(), PO.filter_rows(frames.cpu().numpy()))


def test_recorded_streams_are_reproduced():
    """tests/golden/png_v1.npz: the small cases and their streams as the CPU twin produced them (tools/make_png_fixture.py).  The twin and
    the device must both write exactly these bytes."""
    from spatialaudiogen_amd import png
    z = np.load(GOLDEN)
    names = [str(n) for n in z['names']]
    assert names == list(PO.RECORDED)
    for name in names:
        strings = DEFLATE_CASES[name]
        assert np.array_equal(z['in_' + name], strings), name          # the generator still makes what was recorded
        out, sizes, status = _deflate(strings)
        assert not status.any() and sizes.tolist() == z['sizes_' + name].tolist(), name
        for f in range(strings.shape[0]):
            assert out[f, :sizes[f]].tobytes() == z['out_' + name][f, :sizes[f]].tobytes(), (name, f)
    for name in [str(n) for n in z['filter_names']]:
        assert np.array_equal(png.filter_rows(_t(FILTER_CASES[name])).cpu().numpy(), z['rows_' + name]), name


def test_encoder_files_open_in_pil():
    """Small frames through PngEncoder, RGB and grey, also at a stride that is too small for all of them (each is redone at the bound)."""
    from spatialaudiogen_amd import png
    for name in ('rgb_17x9', 'grey_17x9', 'gradient_sub_wins', 'rgb_1x1', 'tie'):
        frames = FILTER_CASES[name]
        for stride in (None, 8):
            files = png.PngEncoder(_dev(), stride=stride).encode(_t(frames))
            assert len(files) == frames.shape[0]
            for f, data in enumerate(files):
                _same_pixels(data, frames[f])
    assert png.PngEncoder(_dev()).encode(_t(FILTER_CASES['rgb_3x5'][:0])) == []
    assert len(png.png_file(3, 2, 3, b'')) == 57


def test_encoder_retry_at_the_bound_gives_the_files_of_the_bound():
    """Two 8 x 8 noise frames need about 200 bytes each: at stride 16 both are redone alone, and the files are those of stride None."""
    from spatialaudiogen_amd import png
    frames = _t(np.random.RandomState(11).randint(0, 256, (2, 8, 8, 3)).astype(np.uint8))
    status = png.deflate(png.filter_rows(frames), 16)[2]
    assert status.tolist() == [1, 1]
    assert png.PngEncoder(_dev(), stride=16).encode(frames) == png.PngEncoder(_dev()).encode(frames)


# ---- a flagship-sized call (needs the device) ------------------------------------------------------------------------------------------
def test_sixty_four_frames_of_224x448():
    """One call of 64 frames: natural(1), one colour, uniform noise, and 61 more of the three kinds.  PIL opens every file, accepts the
    CRCs and returns the frame; the sizes meet the scheme's."""
    import torch
    from PIL import Image
    from spatialaudiogen_amd import png
    assert torch.cuda.is_available()
    ensure_lib()
    rs = np.random.RandomState(64)
    nat = [PO.natural(s) for s in (1, 2, 3)]
    frames = [nat[0], np.broadcast_to(np.array([200, 30, 90], np.uint8), (224, 448, 3)).copy(), rs.randint(0, 256, (224, 448, 3)).astype(np.uint8)]
    for k in range(61):
        kind = k % 4
        if kind == 0:
            frames.append(np.roll(nat[k % 3], 7 * k + 1, 1))
        elif kind == 1:
            frames.append(np.ascontiguousarray(nat[k % 3][::-1]))
        elif kind == 2:
            frames.append(np.full((224, 448, 3), k, np.uint8))
        else:
            a = nat[k % 3].copy()
            a[40:120, 100:300] = (k, 2 * k, 255 - k)                    # a flat patch: long runs inside a natural frame
            frames.append(a)
    frames = np.stack(frames, 0)
    files = png.PngEncoder('cuda').encode(torch.as_tensor(frames).cuda())
    assert len(files) == 64
    for f in range(64):
        _same_pixels(files[f], frames[f])
    raw = 224 * (1 + 448 * 3)
    buf = io.BytesIO()
    Image.fromarray(frames[0]).save(buf, 'PNG')
    print('natural(1): %d bytes, PIL %d; one colour: %d; noise: %d (bound %d + 57)' % (len(files[0]), len(buf.getvalue()), len(files[1]), len(files[2]),
                                                                                      _bound(raw)))
    assert len(files[0]) <= 1.05 * len(buf.getvalue())
    assert len(files[1]) < raw / 64.
    assert len(files[2]) <= _bound(raw) + 57
    # the same call against the twin: the streams are the same bytes
    from spatialaudiogen_amd import build
    tw = C.CDLL(build.build_cpu_twin())
    P, I, I64 = C.c_void_p, C.c_int, C.c_int64
    tw.sagen_png_filter.argtypes = [P, I, I, I, I, P, P]
    tw.sagen_deflate.argtypes = [P, I, I64, P, I64, P, P, P, C.c_size_t, P]
    tw.sagen_deflate_scratch_bytes.restype = C.c_size_t
    tw.sagen_deflate_scratch_bytes.argtypes = [I, I64, I64]
    sub = np.ascontiguousarray(frames[:4])
    rows = np.zeros((4, 224, 1 + 448 * 3), np.uint8)
    assert tw.sagen_png_filter(sub.ctypes.data, 4, 448, 224, 3, rows.ctypes.data, None) == 0
    stride = (_bound(raw) + 3) // 4 * 4
    out, sizes, status = np.zeros((4, stride), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.int32)
    need = tw.sagen_deflate_scratch_bytes(4, raw, stride)
    scratch = np.zeros(need // 8 + 2, np.float64)
    sc = (scratch.ctypes.data + 15) // 16 * 16
    assert tw.sagen_deflate(rows.ctypes.data, 4, raw, out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data, sc, need, None) == 0
    for f in range(4):
        assert files[f] == png.png_file(448, 224, 3, out[f, :sizes[f]].tobytes()), f


# ---- command lines (need the device) ---------------------------------------------------------------------------------------------------
def _read(folder):
    from PIL import Image
    names = sorted(os.listdir(folder))
    return names, [np.asarray(Image.open(os.path.join(folder, f))) for f in names]


def test_command_lines_write_the_same_pictures_either_way(tmp_path):
    """overlay and deploy --overlay_dir on a 2.5 s clip, --encode host / device / no flag: the same names, the same pixels; the host
    folder holds exactly what PIL's default save makes of those pixels, which is what the command wrote before the flag existed."""
    import torch
    from PIL import Image
    assert torch.cuda.is_available()
    ensure_lib()
    from test_feeder import make_clip
    from spatialaudiogen_amd import deploy, overlay
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    np.savez(str(model_dir / 'variables.npz'), **init_weights(variable_specs(['audio']), seed=8, mode='test'))
    (model_dir / 'train-params.txt').write_text(
        "encoders: ['audio']\nseparation: unet_mask\nambi_order: 1\naudio_rate: 48000\nvideo_rate: 10\ncontext: 1.0\n"
        "num_sep_tracks: 32\nloc_units: [512, 512]\n")
    clip_dir = str(tmp_path / 'clip')
    make_clip(clip_dir, secs=4, video=True)
    wav = str(tmp_path / 'ambi.wav')
    folders = {}
    for mode in ('none', 'host', 'device'):
        folders['deploy_' + mode] = str(tmp_path / ('deploy_' + mode))
        flag = [] if mode == 'none' else ['--encode', mode]
        deploy.main([str(model_dir), clip_dir, '--deploy_duration', '2.5', '--output_fn', wav, '--overlay_dir', folders['deploy_' + mode]] + flag)
    for mode in ('none', 'host', 'device'):
        folders['overlay_' + mode] = str(tmp_path / ('overlay_' + mode))
        flag = [] if mode == 'none' else ['--encode', mode]
        overlay.main([wav, os.path.join(clip_dir, 'video'), folders['overlay_' + mode], '--block', '7'] + flag)
    for tool in ('deploy', 'overlay'):
        names, host = _read(folders[tool + '_host'])
        assert names == ['%06d.png' % i for i in range(15)]
        for mode in ('none', 'device'):
            other_names, other = _read(folders['%s_%s' % (tool, mode)])
            assert other_names == names
            for a, b in zip(host, other):
                assert a.shape == (224, 448, 3) and np.array_equal(a, b), (tool, mode)
        differ = 0
        for f, pixels in zip(names, host):
            buf = io.BytesIO()
            Image.fromarray(pixels).save(buf, 'PNG')
            data = open(os.path.join(folders[tool + '_host'], f), 'rb').read()
            assert data == buf.getvalue() == open(os.path.join(folders[tool + '_none'], f), 'rb').read(), (tool, f)
            differ += data != open(os.path.join(folders[tool + '_device'], f), 'rb').read()
        assert differ == 15                                            # the device's files are its own bytes
    with pytest.raises(SystemExit):
        deploy.main([str(model_dir), clip_dir, '--deploy_duration', '2.5', '--output_fn', wav, '--encode', 'device'])
    model = deploy.W2XYZ(str(model_dir))
    from spatialaudiogen_amd import png
    pred, files = model.deploy_and_overlay(clip_dir, 0., 2.5, overlay.Overlay(4), encoder=png.PngEncoder('cuda'))
    assert files == [open(os.path.join(folders['deploy_device'], '%06d.png' % i), 'rb').read() for i in range(15)]
