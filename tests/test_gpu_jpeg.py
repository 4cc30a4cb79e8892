"""Baseline JPEG decode on the device (csrc/jpeg.hip through jpeg.decode_packed / jpeg.JpegDecoder) against the pixels PIL decoded on
libjpeg-turbo when tests/golden/jpeg_v1.npz was made: EQUALITY, every byte, every status 0.  The arithmetic is integer end to end
(include/sagen.h), so there is no tolerance to choose.  Valid streams only: damaged ones go to the CPU twin and to a sanitizer
build (tests/test_cpu_twin_jpeg.py), never to a device.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_jpeg.py)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from test_jpeg_host import fixture, turbo
from util import ensure_lib

pytestmark = pytest.mark.gpu

OP_CASES = ('test_each_fixture_stream_alone or test_streams_of_one_geometry_in_one_call or test_error_codes or '
            'test_decoder_keeps_input_order_across_geometries or test_unsupported_file_falls_back_with_one_warning')


def _dev():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    if _lib.IS_CPU_TWIN:
        return 'cpu'
    import torch
    assert torch.cuda.is_available()
    return 'cuda'


def _decode(datas):
    """Through the C ABI: parse + pack on the host, one copy, one call -> (pixels, status) as numpy."""
    import torch
    from spatialaudiogen_amd import jpeg
    dev = _dev()
    packed = jpeg.pack(datas, [jpeg.parse(d) for d in datas])
    out, status = jpeg.decode_packed(packed, torch.as_tensor(packed.buffer).to(dev))
    return out.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('k', range(30))
def test_each_fixture_stream_alone(k):
    names, data, rgb, _ = fixture()
    got, status = _decode([data[names[k]]])
    assert status.tolist() == [0], names[k]
    assert got.dtype == np.uint8 and got.shape == (1,) + rgb[names[k]].shape
    assert np.array_equal(got[0], rgb[names[k]]), names[k]


def _geometries():
    from spatialaudiogen_amd import jpeg
    names, data, _, _ = fixture()
    groups = {}
    for n in names:
        groups.setdefault(tuple(jpeg.parse(data[n])[:5]), []).append(n)
    return groups


def test_streams_of_one_geometry_in_one_call():
    """Mixed quantisation tables, Huffman tables (standard and per-file) and restart settings in one call; the single-MCU sizes, the
    partial MCUs, the plane one chroma column wide and the 48 x 64 frame with an interval of 3 blocks are all among them."""
    from spatialaudiogen_amd import jpeg
    names, data, rgb, _ = fixture()
    groups = _geometries()
    assert sum(len(v) for v in groups.values()) == 30 and sum(len(v) > 1 for v in groups.values()) >= 4
    for geom, members in sorted(groups.items()):
        members = members + members[:1]                                 # (a stream twice: its tables are shared, its pixels equal)
        got, status = _decode([data[n] for n in members])
        assert not status.any(), (geom, status)
        for j, n in enumerate(members):
            assert np.array_equal(got[j], rgb[n]), (geom, n)
    mixed = groups[(17, 23, 3, 2, 2)]
    infos = [jpeg.parse(data[n]) for n in mixed]
    assert len({i.restart_interval for i in infos}) > 1 and len({i.actabs[0] for i in infos}) > 1 and len({i.qtabs[0].tobytes() for i in infos}) > 2
    assert (8, 8, 3, 2, 2) in groups and (48, 64, 3, 2, 2) in groups and (16, 16, 3, 2, 2) in groups


def test_error_codes():
    import torch
    from spatialaudiogen_amd import _lib, jpeg
    from spatialaudiogen_amd.ops import _stream
    names, data, rgb, _ = fixture()
    dev = _dev()
    l = _lib.lib()
    d = data['420_17x23_q75']
    p = jpeg.pack([d], [jpeg.parse(d)])
    staged = torch.as_tensor(p.buffer).to(dev)
    out = torch.full((1, 23, 17, 3), 77, dtype=torch.uint8, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    need = l.sagen_jpeg_decode_scratch_bytes(1, 17, 23, 3, 2, 2, p.n_hufftabs)
    assert need > 6 * 6 * 128 and need % 16 == 0
    scratch = torch.empty(need // 8, dtype=torch.float64, device=dev)
    base = staged.data_ptr()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(bytes_=base + p.bytes_at, total=p.total_bytes, frames=base + p.frames_at, n=1, segs=base + p.segments_at, n_segs=p.n_segments,
             qt=base + p.qtabs_at, n_qt=p.n_qtabs, ht=base + p.hufftabs_at, n_ht=p.n_hufftabs, w=17, h=23, comps=3, hs=2, vs=2, o=ptr(out), st=ptr(status),
             sc=ptr(scratch), sc_bytes=need):
        return l.sagen_jpeg_decode(bytes_, total, frames, n, segs, n_segs, qt, n_qt, ht, n_ht, w, h, comps, hs, vs, o, st, sc, sc_bytes, _stream())

    for kw in (dict(bytes_=None), dict(frames=None), dict(segs=None), dict(qt=None), dict(ht=None), dict(o=None), dict(st=None), dict(sc=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(n=-1), dict(w=0), dict(h=0), dict(total=-4), dict(total=p.total_bytes + 1), dict(n_segs=0), dict(n_qt=0), dict(n_ht=0),
               dict(bytes_=base + p.bytes_at + 1), dict(frames=base + p.frames_at + 4), dict(sc=C.c_void_p(scratch.data_ptr() + 8), sc_bytes=need)):
        assert call(**kw) == -2, (kw, l.sagen_last_error())
    for kw in (dict(comps=4), dict(comps=2), dict(hs=1, vs=2), dict(hs=4, vs=1), dict(comps=1, hs=2, vs=2), dict(w=16385), dict(h=16385), dict(n=65536)):
        assert call(**kw) == -3, (kw, l.sagen_last_error())
    assert b'sampling' in l.sagen_last_error() or b'16384' in l.sagen_last_error() or b'65535' in l.sagen_last_error()
    assert call(sc_bytes=need - 1) == -5 and call(sc_bytes=0) == -5
    assert l.sagen_jpeg_decode_scratch_bytes(1, 17, 23, 3, 1, 2, 4) == 0 and l.sagen_jpeg_decode_scratch_bytes(0, 17, 23, 3, 2, 2, 4) == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((out == 77).all()) and status.tolist() == [-1]          # every refused call left the outputs alone
    assert call(n=0) == 0 and call(n=0, bytes_=None, frames=None, o=None, st=None, sc=None) == 0
    assert bool((out == 77).all())
    assert call() == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert status.tolist() == [0] and np.array_equal(out.cpu().numpy()[0], rgb['420_17x23_q75'])


# ---- JpegDecoder -----------------------------------------------------------------------------------------------------------------------
def test_decoder_keeps_input_order_across_geometries(tmp_path):
    from spatialaudiogen_amd import jpeg
    names, data, rgb, _ = fixture()
    order = ['420_17x23_q75', '444_17x23_q75', '420_17x23_q30_rows', 'grey_17x23_q30_opt', '422_17x23_q75', '420_17x23_q1', '444_17x23_q75']
    items = [data[n] for n in order]
    path = str(tmp_path / 'frame.jpg')
    with open(path, 'wb') as f:
        f.write(items[2])
    items[2] = path                                                     # paths and bytes mix
    dec = jpeg.JpegDecoder(_dev())
    got = dec.decode(items)
    assert got.device.type == _dev() and tuple(got.shape) == (7, 23, 17, 3)
    for j, n in enumerate(order):
        assert np.array_equal(got[j].cpu().numpy(), rgb[n]), n
    assert tuple(dec.decode([]).shape) == (0, 0, 0, 3)
    with pytest.raises(ValueError, match='one size'):
        dec.decode([data['420_17x23_q75'], data['420_33x18_q100']])
    with pytest.raises(ValueError):
        dec.decode([b'no jpeg at all'])
    got = jpeg.load_frames_device([path, path], _dev())
    assert np.array_equal(got[1].cpu().numpy(), rgb['420_17x23_q30_rows'])


def test_unsupported_file_falls_back_with_one_warning():
    import warnings
    from spatialaudiogen_amd import jpeg
    from spatialaudiogen_amd.feeder import imread
    names, data, rgb, rejects = fixture()
    prog = dict((r[0], r[1]) for r in rejects)['progressive']
    want = imread(io.BytesIO(prog))
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(want).save(b, 'JPEG', quality=90)                   # a baseline frame of the same size, between two progressive ones
    base = b.getvalue()
    dec = jpeg.JpegDecoder(_dev())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got = dec.decode([prog, base, prog]).cpu().numpy()
        again = dec.decode([prog]).cpu().numpy()
    caught = [c for c in caught if issubclass(c.category, jpeg.JpegFallbackWarning)]
    assert len(caught) == 1 and 'progressive' in str(caught[0].message)
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want) and np.array_equal(again[0], want)
    if turbo():
        assert np.array_equal(got[1], imread(io.BytesIO(base)))


# ---- a flagship-sized call (needs the device) ------------------------------------------------------------------------------------------
def _twin_decode(datas, infos=None):
    """The same call on the CPU twin, loaded beside the HIP library, on numpy buffers (infos: descriptors other than parse()'s)."""
    from spatialaudiogen_amd import build, jpeg
    l = C.CDLL(build.build_cpu_twin())
    l.sagen_jpeg_decode_scratch_bytes.restype = C.c_size_t
    P, I = C.c_void_p, C.c_int
    l.sagen_jpeg_decode.argtypes = [P, C.c_int64, P, I, P, I, P, I, P, I, I, I, I, I, I, P, P, P, C.c_size_t, P]
    p = jpeg.pack(datas, infos if infos is not None else [jpeg.parse(d) for d in datas])
    w, h, comps, hs, vs = p.geometry
    out, status = np.zeros((p.n, h, w, 3), np.uint8), np.full(p.n, -1, np.int32)
    need = l.sagen_jpeg_decode_scratch_bytes(p.n, w, h, comps, hs, vs, p.n_hufftabs)
    scratch = np.zeros(need // 8 + 2, np.float64)
    buf = np.zeros(p.buffer.size // 8 + 2, np.float64)                  # (an aligned home for the packed bytes)
    buf.view(np.uint8)[:p.buffer.size] = p.buffer
    base = buf.ctypes.data
    sc = (scratch.ctypes.data + 15) // 16 * 16
    assert l.sagen_jpeg_decode(base + p.bytes_at, p.total_bytes, base + p.frames_at, p.n, base + p.segments_at, p.n_segments, base + p.qtabs_at,
                               p.n_qtabs, base + p.hufftabs_at, p.n_hufftabs, w, h, comps, hs, vs, out.ctypes.data, status.ctypes.data, sc, need, None) == 0
    return out, status


def test_twelve_frames_of_224x448_equal_the_twin_and_live_pil():
    import torch
    assert torch.cuda.is_available()
    from PIL import Image
    rs = np.random.RandomState(12)
    y, x = np.mgrid[0:224, 0:448]
    datas = []
    for k in range(12):
        a = np.stack([127 + 100 * np.sin(x / 23. + k), 127 + 100 * np.cos(y / 17. - k), (x + 2 * y + 20 * k) % 256], -1) + rs.randint(-12, 13, (224, 448, 3))
        b = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(b, 'JPEG', quality=95, subsampling=2)
        datas.append(b.getvalue())
    got, status = _decode(datas)
    ref, ref_status = _twin_decode(datas)
    assert not status.any() and not ref_status.any()
    assert np.array_equal(got, ref)
    if turbo():
        for k in range(12):
            assert np.array_equal(got[k], np.asarray(Image.open(io.BytesIO(datas[k])).convert('RGB'))), k


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


def test_project_command_line_gives_the_same_files_either_way(tmp_path):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import project
    src = str(tmp_path / 'in')
    _folder(src, 6, 48, 96, 1)
    for mode in ('host', 'device'):
        project.main([src, str(tmp_path / mode), '--from', 'er', '--to', 'er', '--size', '24', '48', '--decode', mode, '--block', '4'])
    _same_files(str(tmp_path / 'host'), str(tmp_path / 'device'))
    assert len(os.listdir(str(tmp_path / 'host'))) == 6


def test_flow_command_line_gives_the_same_files_either_way(tmp_path):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import flow
    src = str(tmp_path / 'in')
    _folder(src, 5, 32, 64, 2)
    for mode in ('host', 'device'):
        flow.main([src, str(tmp_path / mode), '--levels', '1', '--decode', mode, '--block', '2'])
    _same_files(str(tmp_path / 'host'), str(tmp_path / 'device'))
    assert 'flow_limits.npy' in os.listdir(str(tmp_path / 'host')) and len(os.listdir(str(tmp_path / 'host'))) == 6


def test_overlay_command_line_gives_the_same_files_either_way(tmp_path):
    """1.5 s of first-order ambisonics = 3 maps -> 10 painted frames of the 12 in the folder."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import overlay
    from spatialaudiogen_amd.feeder import save_wav
    src, wav = str(tmp_path / 'in'), str(tmp_path / 'ambi.wav')
    _folder(src, 12, 32, 64, 3)
    save_wav(wav, 0.3 * np.random.RandomState(4).uniform(-1., 1., (72000, 4)), 48000)
    for mode in ('host', 'device'):
        overlay.main([wav, src, str(tmp_path / mode), '--decode', mode, '--block', '4'])
    _same_files(str(tmp_path / 'host'), str(tmp_path / 'device'))
    assert len(os.listdir(str(tmp_path / 'host'))) == 10
