"""Baseline JPEG encode on the device (csrc/jpeg_enc.hip through jpeg.encode_streams / jpeg.JpegEncoder) against the files PIL wrote on
libjpeg-turbo when tests/golden/jpeg_enc_v1.npz was made: EQUALITY, every byte, every size, every status.  The arithmetic is integer end
to end (include/sagen.h), so there is no tolerance to choose.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_jpeg_enc.py)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import jpeg_enc_oracle as JE
from test_jpeg_enc_host import FACTORS, SUBSAMPLING, fixture, pil_file, scan_of, turbo
from util import ensure_lib

pytestmark = pytest.mark.gpu

OP_CASES = ('test_each_fixture_case_alone or test_cases_of_one_geometry_in_one_call or test_capacity_rule or test_refusals_leave_every_output_untouched or '
            'test_bad_quantiser_gives_every_frame_range or test_device_decode_of_device_encoded_files')
POISON = 0xA5


def _dev():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    if _lib.IS_CPU_TWIN:
        return 'cpu'
    import torch
    assert torch.cuda.is_available()
    return 'cuda'


def _default_stride(img):
    return max((img.size + 63) // 64 * 64, 4096)


def _encode(images, quality, sampling, stride=None, out=None):
    """Through the C ABI: one copy in, one call -> (out, sizes, status) as numpy."""
    import torch
    from spatialaudiogen_amd import jpeg
    frames = torch.as_tensor(np.stack(images, 0)).to(_dev())
    hs, vs = FACTORS[sampling]
    o, sizes, status = jpeg.encode_streams(frames, jpeg.quality_tables(quality), hs, vs, stride or _default_stride(images[0]), out)
    return o.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('k', range(30))
def test_each_fixture_case_alone(k):
    import torch
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling = fixture()
    n = names[k]
    want = scan_of(data[n])
    out, sizes, status = _encode([image[n]], quality[n], sampling[n])
    assert status.tolist() == [0] and sizes.tolist() == [len(want)], n
    assert out[0, :len(want)].tobytes() == want, n
    enc = jpeg.JpegEncoder(_dev(), quality[n], SUBSAMPLING[sampling[n]])
    assert enc.encode(torch.as_tensor(image[n][None]).to(_dev())) == [data[n]], n


def test_cases_of_one_geometry_in_one_call():
    """Everything that shares sampling, size and quality in one call, the first of them once more at the end: the frames' streams
    start at different bits and bytes of their rows' scans."""
    names, image, data, quality, sampling = fixture()
    groups = {}
    for n in names:
        groups.setdefault((sampling[n], image[n].shape, quality[n]), []).append(n)
    assert sum(len(v) > 1 for v in groups.values()) >= 2
    for key, members in sorted(groups.items(), key=str):
        members = members + members[:1]
        out, sizes, status = _encode([image[n] for n in members], key[2], key[0])
        assert not status.any(), (key, status)
        for j, n in enumerate(members):
            want = scan_of(data[n])
            assert sizes[j] == len(want) and out[j, :len(want)].tobytes() == want, (key, n)


def test_capacity_rule():
    """stride 64: the noise frames need about 600 bytes, the flat ones about 10.  The rows of `out` lie inside a larger poisoned tensor:
    what a long frame writes past its row would land in the exact row behind it, or in the poison behind the last."""
    import torch
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling = fixture()
    noise = image['420_17x23_q95_noise']
    frames = [np.full_like(noise, 40), noise, np.full_like(noise, 200), noise[::-1].copy()]
    want = [scan_of(JE.encode(f, 95, '4:2:0')) for f in frames]
    assert [len(w) > 64 for w in want] == [False, True, False, True] and scan_of(data['420_17x23_q95_noise']) == want[1]
    big = torch.full((16 + 4 * 64 + 64,), POISON, dtype=torch.uint8, device=_dev())
    out, sizes, status = _encode(frames, 95, '420', 64, big[16:16 + 4 * 64].view(4, 64))
    assert status.tolist() == [0, 1, 0, 1]
    assert sizes.tolist() == [len(w) for w in want]
    for j in (0, 2):
        assert out[j, :sizes[j]].tobytes() == want[j], j
        assert (out[j, sizes[j]:] == POISON).all()                      # nothing behind the stream's end either
    guard = big.cpu().numpy()
    assert (guard[:16] == POISON).all() and (guard[16 + 4 * 64:] == POISON).all()
    enc = jpeg.JpegEncoder(_dev(), 95, '4:2:0', stride=64)
    assert enc.encode(torch.as_tensor(np.stack(frames, 0)).to(_dev())) == [JE.encode(f, 95, '4:2:0') for f in frames]
    # a stride of exactly what the frame needs is enough
    out, sizes, status = _encode(frames[1:2], 95, '420', (len(want[1]) + 3) // 4 * 4)
    assert status.tolist() == [0] and out[0, :len(want[1])].tobytes() == want[1]


def test_refusals_leave_every_output_untouched():
    import torch
    from spatialaudiogen_amd import _lib, jpeg
    from spatialaudiogen_amd.ops import _stream
    names, image, data, quality, sampling = fixture()
    dev = _dev()
    l = _lib.lib()
    img = image['420_17x23_q75_noise']
    frames = torch.as_tensor(img[None]).to(dev)
    qt = torch.as_tensor(np.ascontiguousarray(jpeg.quality_tables(75)[:, JE.zigzag()]).view(np.int16)).to(dev)
    out = torch.full((1, 4096), POISON, dtype=torch.uint8, device=dev)
    sizes = torch.full((1,), -1, dtype=torch.int32, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    need = l.sagen_jpeg_encode_scratch_bytes(1, 17, 23, 3, 2, 2, 4096)
    assert need > 24 * 128 and need % 16 == 0
    scratch = torch.empty(need // 8, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(fr=ptr(frames), n=1, w=17, h=23, comps=3, hs=2, vs=2, q=ptr(qt), o=ptr(out), stride=4096, sz=ptr(sizes), st=ptr(status), sc=ptr(scratch),
             sc_bytes=need):
        return l.sagen_jpeg_encode(fr, n, w, h, comps, hs, vs, q, o, stride, sz, st, sc, sc_bytes, _stream())

    for kw in (dict(fr=None), dict(q=None), dict(o=None), dict(sz=None), dict(st=None), dict(sc=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(n=-1), dict(w=0), dict(h=0), dict(stride=0), dict(stride=-4), dict(stride=4094), dict(o=C.c_void_p(out.data_ptr() + 2)),
               dict(sz=C.c_void_p(sizes.data_ptr() + 2)), dict(st=C.c_void_p(status.data_ptr() + 1)), dict(q=C.c_void_p(qt.data_ptr() + 1)),
               dict(sc=C.c_void_p(scratch.data_ptr() + 8))):
        assert call(**kw) == -2, (kw, l.sagen_last_error())
    for kw in (dict(comps=4), dict(comps=2), dict(hs=1, vs=2), dict(hs=4, vs=1), dict(comps=1, hs=2, vs=2), dict(w=16385), dict(h=16385), dict(n=65536),
               dict(stride=(1 << 28) + 4)):
        assert call(**kw) == -3, (kw, l.sagen_last_error())
    assert b'stride' in l.sagen_last_error()
    assert call(sc_bytes=need - 1) == -5 and call(sc_bytes=0) == -5
    assert l.sagen_jpeg_encode_scratch_bytes(1, 17, 23, 3, 1, 2, 4096) == 0 and l.sagen_jpeg_encode_scratch_bytes(0, 17, 23, 3, 2, 2, 4096) == 0
    assert l.sagen_jpeg_encode_scratch_bytes(1, 17, 23, 3, 2, 2, 4095) == 0 and l.sagen_jpeg_encode_max_bytes(17, 23, 3, 1, 2) == 0
    assert l.sagen_jpeg_encode_max_bytes(17, 23, 3, 2, 2) == 2 * ((24 * 1658 + 7) // 8) + 2          # 2 x 2 MCUs of 6 blocks
    assert l.sagen_jpeg_encode_max_bytes(17, 23, 1, 1, 1) == 2 * ((9 * 1658 + 7) // 8) + 2
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((out == POISON).all()) and sizes.tolist() == [-1] and status.tolist() == [-1]       # every refused call left the outputs alone
    assert call(n=0) == 0 and call(n=0, fr=None, q=None, o=None, sz=None, st=None, sc=None) == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((out == POISON).all()) and sizes.tolist() == [-1]
    assert call() == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    want = scan_of(data['420_17x23_q75_noise'])
    assert status.tolist() == [0] and sizes.tolist() == [len(want)] and out.cpu().numpy()[0, :len(want)].tobytes() == want


def test_bad_quantiser_gives_every_frame_range():
    import torch
    from spatialaudiogen_amd import _lib, jpeg
    names, image, data, quality, sampling = fixture()
    frames = torch.as_tensor(np.stack([image['420_17x23_q75_noise']] * 2, 0)).to(_dev())
    for bad in (0, 256):
        q = jpeg.quality_tables(75).copy()
        q[1, 63] = bad
        out, sizes, status = jpeg.encode_streams(frames, q, 2, 2, 4096)
        assert status.cpu().tolist() == [_lib.SAGEN_JPEG_ENC_ST_RANGE] * 2
    with pytest.raises(ValueError, match='frame 7'):
        enc = jpeg.JpegEncoder(_dev(), 75)
        enc.qtabs = q
        enc.encode(frames, first=7)


def test_device_decode_of_device_encoded_files():
    """The loop closed: frames -> JpegEncoder -> JpegDecoder equals PIL's decode of PIL's files."""
    import torch
    from PIL import Image
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling = fixture()
    members = ['420_17x23_q95_noise', '420_17x23_q95_smooth']
    frames = torch.as_tensor(np.stack([image[n] for n in members], 0)).to(_dev())
    files = jpeg.JpegEncoder(_dev(), 95, '4:2:0').encode(frames)
    got = jpeg.JpegDecoder(_dev()).decode(files).cpu().numpy()
    for j, n in enumerate(members):
        assert np.array_equal(got[j], np.asarray(Image.open(io.BytesIO(data[n])).convert('RGB'))), n


# ---- a flagship-sized call (needs the device) ------------------------------------------------------------------------------------------
def _twin_encode(frames, quality, hs, vs, stride):
    """The same call on the CPU twin, loaded beside the HIP library, on numpy buffers."""
    from spatialaudiogen_amd import build, jpeg
    l = C.CDLL(build.build_cpu_twin())
    P, I = C.c_void_p, C.c_int
    l.sagen_jpeg_encode_scratch_bytes.restype = C.c_size_t
    l.sagen_jpeg_encode_scratch_bytes.argtypes = [I] * 6 + [C.c_int64]
    l.sagen_jpeg_encode.argtypes = [P, I, I, I, I, I, I, P, P, C.c_int64, P, P, P, C.c_size_t, P]
    n, h, w = frames.shape[:3]
    comps = 3 if frames.ndim == 4 else 1
    q = np.ascontiguousarray(jpeg.quality_tables(quality)[:, JE.zigzag()])
    out, sizes, status = np.zeros((n, stride), np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    need = l.sagen_jpeg_encode_scratch_bytes(n, w, h, comps, hs, vs, stride)
    scratch = np.zeros(need // 8 + 2, np.float64)
    sc = (scratch.ctypes.data + 15) // 16 * 16
    frames = np.ascontiguousarray(frames)
    assert l.sagen_jpeg_encode(frames.ctypes.data, n, w, h, comps, hs, vs, q.ctypes.data, out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data,
                               sc, need, None) == 0
    return out, sizes, status


def test_twelve_frames_of_224x448_equal_the_twin_and_live_pil():
    """2 352 blocks a frame: ten tiles of the bit-position scan, seventeen of the stuffing scan."""
    import torch
    assert torch.cuda.is_available()
    rs = np.random.RandomState(12)
    y, x = np.mgrid[0:224, 0:448]
    frames = []
    for k in range(12):
        a = np.stack([127 + 100 * np.sin(x / 23. + k), 127 + 100 * np.cos(y / 17. - k), (x + 2 * y + 20 * k) % 256], -1) + rs.randint(-12, 13, (224, 448, 3))
        frames.append(np.clip(a, 0, 255).astype(np.uint8))
    stride = _default_stride(frames[0])
    got, sizes, status = _encode(frames, 95, '420', stride)
    ref, ref_sizes, ref_status = _twin_encode(np.stack(frames, 0), 95, 2, 2, stride)
    assert not status.any() and not ref_status.any()
    assert np.array_equal(sizes, ref_sizes) and sizes.min() > 2 * 4096
    for k in range(12):
        assert np.array_equal(got[k, :sizes[k]], ref[k, :sizes[k]]), k
        if turbo():
            assert got[k, :sizes[k]].tobytes() == scan_of(pil_file(frames[k], 95, '420')), k


# ---- command lines (need the device) ---------------------------------------------------------------------------------------------------
def _folder(path, n, h, w, seed):
    from PIL import Image
    os.makedirs(path)
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    for k in range(n):
        a = np.stack([127 + 100 * np.sin((x + 3 * k) / 9.), 127 + 100 * np.cos(y / 7.), (3 * x + 2 * y + 9 * k) % 256], -1) + rs.randint(-8, 9, (h, w, 3))
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(os.path.join(path, '%06d.jpg' % k), quality=95)


def _same_files(a, b):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) > 0
    for f in os.listdir(a):
        assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), f


def test_project_command_line_writes_the_same_files_either_way(tmp_path):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import project
    src = str(tmp_path / 'in')
    _folder(src, 6, 32, 64, 1)
    for mode in ('host', 'device'):
        project.main([src, str(tmp_path / mode), '--from', 'er', '--to', 'er', '--size', '24', '48', '--decode', mode, '--encode', mode, '--block', '4'])
    _same_files(str(tmp_path / 'host'), str(tmp_path / 'device'))
    assert len(os.listdir(str(tmp_path / 'host'))) == 6


def test_flow_command_line_writes_the_same_files_either_way(tmp_path):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import flow
    src = str(tmp_path / 'in')
    _folder(src, 6, 32, 64, 2)
    for mode in ('host', 'device'):
        flow.main([src, str(tmp_path / mode), '--levels', '2', '--iters', '4', '--decode', mode, '--encode', mode, '--block', '4'])
    _same_files(str(tmp_path / 'host'), str(tmp_path / 'device'))
    assert 'flow_limits.npy' in os.listdir(str(tmp_path / 'host')) and len(os.listdir(str(tmp_path / 'host'))) == 7


def test_png_with_device_encode_is_refused_before_any_file_is_touched(tmp_path):
    ensure_lib()
    from spatialaudiogen_amd import flow, project
    src, dst = str(tmp_path / 'in'), str(tmp_path / 'out')
    _folder(src, 2, 32, 64, 3)
    os.makedirs(dst)
    with open(os.path.join(dst, '000000.png'), 'wb') as f:
        f.write(b'kept')
    for run in (lambda: project.main([src, dst, '--from', 'er', '--to', 'er', '--size', '24', '48', '--format', 'png', '--encode', 'device', '--overwrite']),
                lambda: flow.main([src, dst, '--format', 'png', '--encode', 'device', '--overwrite'])):
        with pytest.raises(SystemExit) as e:
            run()
        assert e.value.code not in (0, None) and '--encode device' in str(e.value.code)
        assert os.listdir(dst) == ['000000.png'] and open(os.path.join(dst, '000000.png'), 'rb').read() == b'kept'
