"""JPEG restart intervals on the device (csrc/jpeg_enc.hip through sagen_jpeg_encode_rst, jpeg.encode_streams / jpeg.JpegEncoder)
against the files PIL wrote on libjpeg-turbo with restart_marker_blocks=R when tests/golden/jpeg_rst_v1.npz was made: EQUALITY, every
byte, every size, every status.  The arithmetic is integer end to end (include/sagen.h), so there is no tolerance to choose.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_jpeg_rst.py)."""
import io
import os

import numpy as np
import pytest

import jpeg_enc_oracle as JE
import jpeg_rst_oracle as JR
from test_jpeg_enc_host import FACTORS, SUBSAMPLING
from test_jpeg_enc_host import fixture as plain_fixture
from test_jpeg_enc_host import scan_of as plain_scan_of
from test_jpeg_rst_host import N_CASES, fixture, mcus_of, pil_file, scan_of
from util import ensure_lib

pytestmark = pytest.mark.gpu

OP_CASES = ('test_each_fixture_case_alone or test_cases_of_one_geometry_in_one_call or test_capacity_rule or test_interval_zero_is_the_plain_encoder or '
            'test_device_decode_of_device_written_files or test_bad_quantiser_gives_every_frame_range_and_no_bytes or '
            'test_three_frames_of_64x128_at_one_row or test_encoder_refuses_an_interval_dri_cannot_name or '
            'test_transcode_of_a_plain_file or test_transcode_of_optimised_and_of_segmented_files or test_a_truncated_source or '
            'test_jpeg_restart_command_line')
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


def _encode(images, quality, sampling, interval, stride=None, out=None):
    """Through the C ABI: one copy in, one call -> (out, sizes, status) as numpy."""
    import torch
    from spatialaudiogen_amd import jpeg
    frames = torch.as_tensor(np.stack(images, 0)).to(_dev())
    hs, vs = FACTORS[sampling]
    o, sizes, status = jpeg.encode_streams(frames, jpeg.quality_tables(quality), hs, vs, stride or _default_stride(images[0]), out, restart_interval=interval)
    return o.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('k', range(N_CASES))
def test_each_fixture_case_alone(k):
    """Into a poisoned row: the stream, its size, status 0, and nothing behind the stream's end; then the complete file."""
    import torch
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling, interval = fixture()
    n = names[k]
    want = scan_of(data[n])
    stride = max(_default_stride(image[n]), (len(want) + 3) // 4 * 4)  # (noise at quality 100 is longer than its pixels)
    big = torch.full((16 + stride + 64,), POISON, dtype=torch.uint8, device=_dev())
    out, sizes, status = _encode([image[n]], quality[n], sampling[n], interval[n], stride, big[16:16 + stride].view(1, stride))
    assert status.tolist() == [0] and sizes.tolist() == [len(want)], n
    assert out[0, :len(want)].tobytes() == want, n
    guard = big.cpu().numpy()
    assert (guard[:16] == POISON).all() and (guard[16 + len(want):] == POISON).all(), n
    enc = jpeg.JpegEncoder(_dev(), quality[n], SUBSAMPLING[sampling[n]], restart_blocks=interval[n])
    assert enc.encode(torch.as_tensor(image[n][None]).to(_dev())) == [data[n]], n
    if n.endswith('_rrow'):                                            # rows win over blocks
        enc = jpeg.JpegEncoder(_dev(), quality[n], SUBSAMPLING[sampling[n]], restart_rows=1, restart_blocks=7)
        assert enc.encode(torch.as_tensor(image[n][None]).to(_dev())) == [data[n]], n


def test_cases_of_one_geometry_in_one_call():
    """Everything that shares sampling, size, quality and interval in one call, the first of them once more at the end: the frames'
    segments start at different bits and bytes of their rows' scans."""
    names, image, data, quality, sampling, interval = fixture()
    groups = {}
    for n in names:
        groups.setdefault((sampling[n], image[n].shape, quality[n], interval[n]), []).append(n)
    assert sum(len(v) > 1 for v in groups.values()) >= 2
    for key, members in sorted(groups.items(), key=str):
        members = members + members[:1]
        stride = max(_default_stride(image[members[0]]), max((len(scan_of(data[n])) + 3) // 4 * 4 for n in members))
        out, sizes, status = _encode([image[n] for n in members], key[2], key[0], key[3], stride)
        assert not status.any(), (key, status)
        for j, n in enumerate(members):
            want = scan_of(data[n])
            assert sizes[j] == len(want) and out[j, :len(want)].tobytes() == want, (key, n)


def test_capacity_rule():
    """A stride one word short of what the long frames need: sizes is still filled, nothing is written beyond stride (the rows of
    `out` lie inside a larger poisoned tensor), the neighbours are exact.  A stride of exactly the need is enough, also where the
    stream ends in a marker's neighbourhood; the bound of the header holds."""
    import torch
    from spatialaudiogen_amd import _lib, jpeg
    names, image, data, quality, sampling, interval = fixture()
    noise = image['420_17x23_q75_noise_r1']
    frames = [np.full_like(noise, 40), noise, np.full_like(noise, 200), noise[::-1].copy()]
    want = [scan_of(JR.encode(f, 75, '4:2:0', 1)) for f in frames]
    assert want[1] == scan_of(data['420_17x23_q75_noise_r1'])
    need = max(len(w) for w in want)
    stride = (need + 3) // 4 * 4 - 4                                    # one word short for the longest
    short = [len(w) > stride for w in want]
    assert any(short) and not all(short) and not short[0] and not short[2]
    big = torch.full((16 + 4 * stride + 64,), POISON, dtype=torch.uint8, device=_dev())
    out, sizes, status = _encode(frames, 75, '420', 1, stride, big[16:16 + 4 * stride].view(4, stride))
    assert status.tolist() == [int(s) for s in short]
    assert sizes.tolist() == [len(w) for w in want]
    for j in range(4):
        if not short[j]:
            assert out[j, :sizes[j]].tobytes() == want[j], j
            assert (out[j, sizes[j]:] == POISON).all()                  # nothing behind the stream's end either
    guard = big.cpu().numpy()
    assert (guard[:16] == POISON).all() and (guard[16 + 4 * stride:] == POISON).all()
    enc = jpeg.JpegEncoder(_dev(), 75, '4:2:0', stride=64, restart_blocks=1)                # every frame again at the bound
    assert enc.encode(torch.as_tensor(np.stack(frames, 0)).to(_dev())) == [JR.encode(f, 75, '4:2:0', 1) for f in frames]
    out, sizes, status = _encode(frames[1:2], 75, '420', 1, (len(want[1]) + 3) // 4 * 4)
    assert status.tolist() == [0] and out[0, :len(want[1])].tobytes() == want[1]
    # a stride that cuts the stream inside every marker in turn
    for cut in range(4, len(want[1]), 12):
        big = torch.full((cut + 64,), POISON, dtype=torch.uint8, device=_dev())
        out, sizes, status = _encode(frames[1:2], 75, '420', 1, cut, big[:cut].view(1, cut))
        assert status.tolist() == [1] and sizes.tolist() == [len(want[1])] and (big.cpu().numpy()[cut:] == POISON).all(), cut
    l = _lib.lib()
    for n in names:
        h, w = image[n].shape[:2]
        hs, vs = FACTORS[sampling[n]]
        bound = l.sagen_jpeg_encode_rst_max_bytes(w, h, 1 if sampling[n] == 'grey' else 3, hs, vs, interval[n])
        mx, my = mcus_of(image[n], sampling[n])
        nseg = -(-mx * my // interval[n]) if interval[n] < mx * my else 1
        assert bound == l.sagen_jpeg_encode_max_bytes(w, h, 1 if sampling[n] == 'grey' else 3, hs, vs) + 4 * (nseg - 1) >= len(scan_of(data[n])), n


def test_interval_zero_is_the_plain_encoder():
    """restart_interval = 0 through the new entry gives exactly what sagen_jpeg_encode gives, on all of jpeg_enc_v1.npz; so does an
    interval that reaches over the whole frame, but for the caller's DRI."""
    import ctypes as C
    import torch
    from spatialaudiogen_amd import _lib, jpeg
    from spatialaudiogen_amd.ops import _ptr, _stream
    names, image, data, quality, sampling = plain_fixture()
    dev = _dev()
    l = _lib.lib()
    for n in names:
        img = image[n]
        h, w = img.shape[:2]
        comps = 1 if img.ndim == 2 else 3
        hs, vs = FACTORS[sampling[n]]
        want = plain_scan_of(data[n])
        frames = torch.as_tensor(img[None]).to(dev)
        qt = torch.as_tensor(np.ascontiguousarray(jpeg.quality_tables(quality[n])[:, JE.zigzag()]).view(np.int16)).to(dev)
        for interval in (0, 65535):
            out = torch.full((1, 4096), POISON, dtype=torch.uint8, device=dev)
            sizes = torch.full((1,), -1, dtype=torch.int32, device=dev)
            status = torch.full((1,), -1, dtype=torch.int32, device=dev)
            need = l.sagen_jpeg_encode_rst_scratch_bytes(1, w, h, comps, hs, vs, interval, 4096)
            assert need == l.sagen_jpeg_encode_scratch_bytes(1, w, h, comps, hs, vs, 4096)
            assert l.sagen_jpeg_encode_rst_max_bytes(w, h, comps, hs, vs, interval) == l.sagen_jpeg_encode_max_bytes(w, h, comps, hs, vs)
            scratch = torch.empty(need // 8, dtype=torch.float64, device=dev)
            assert l.sagen_jpeg_encode_rst(_ptr(frames), 1, w, h, comps, hs, vs, interval, _ptr(qt), _ptr(out), 4096, _ptr(sizes), _ptr(status),
                                           _ptr(scratch), need, _stream()) == 0
            got = out.cpu().numpy()
            assert status.tolist() == [0] and sizes.tolist() == [len(want)] and got[0, :len(want)].tobytes() == want, (n, interval)
            assert (got[0, len(want):] == POISON).all(), (n, interval)


def test_device_decode_of_device_written_files():
    """The loop closed: frames -> JpegEncoder with an interval -> JpegDecoder gives PIL's pixels of PIL's files, over as many segments
    as parse reports."""
    import torch
    from PIL import Image
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling, interval = fixture()
    for members in (['420_17x23_q75_noise_r1', '420_17x23_q75_smooth_r1', '420_17x23_q75_saturated_r1'], ['420_48x64_q95_noise_r1'],
                    ['420_40x72_q95_noise_rrow'], ['grey_48x64_q75_noise_r1'], ['422_40x72_q75_saturated_r2']):
        n0 = members[0]
        frames = torch.as_tensor(np.stack([image[n] for n in members], 0)).to(_dev())
        files = jpeg.JpegEncoder(_dev(), quality[n0], SUBSAMPLING[sampling[n0]], restart_blocks=interval[n0]).encode(frames)
        assert files == [data[n] for n in members]
        infos = [jpeg.parse(f) for f in files]
        mx, my = mcus_of(image[n0], sampling[n0])
        assert all(i.restart_interval == interval[n0] and i.segments.size == -(-mx * my // interval[n0]) > 1 for i in infos)
        packed = jpeg.pack(files, infos)
        assert packed.n_segments == sum(i.segments.size for i in infos)
        got, status = jpeg.decode_packed(packed, torch.as_tensor(packed.buffer).to(_dev()))
        assert not status.cpu().numpy().any()
        got = got.cpu().numpy()
        assert np.array_equal(got, jpeg.JpegDecoder(_dev()).decode(files).cpu().numpy())
        for j, n in enumerate(members):
            assert np.array_equal(got[j], np.asarray(Image.open(io.BytesIO(data[n])).convert('RGB'))), n


def test_three_frames_of_64x128_at_one_row():
    """4 x 8 MCUs of 6 blocks at 4:2:0: 192 blocks a frame, so the 256-block tiles of the bit-position scan cross frames' and
    segments' ends; one segment per MCU row.  Against the restatement, and against live PIL where it is libjpeg-turbo."""
    from test_jpeg_enc_host import turbo
    rs = np.random.RandomState(64)
    y, x = np.mgrid[0:64, 0:128]
    frames = []
    for k in range(3):
        a = np.stack([127 + 100 * np.sin(x / 11. + k), 127 + 100 * np.cos(y / 9. - k), (3 * x + 2 * y + 40 * k) % 256], -1) + rs.randint(-30, 31, (64, 128, 3))
        frames.append(np.clip(a, 0, 255).astype(np.uint8))
    frames[1] = rs.randint(0, 256, (64, 128, 3)).astype(np.uint8)      # a long one between two shorter
    want = [scan_of(JR.encode(f, 95, '4:2:0', 8)) for f in frames]
    assert max(len(w) for w in want) > 2 * 4096                        # more than one tile of the stuffing scan
    stride = (max(len(w) for w in want) + 63) // 64 * 64
    out, sizes, status = _encode(frames, 95, '420', 8, stride)
    assert not status.any() and sizes.tolist() == [len(w) for w in want]
    for k in range(3):
        assert out[k, :sizes[k]].tobytes() == want[k], k
        if turbo():
            assert want[k] == scan_of(pil_file(frames[k], 95, '420', restart_marker_rows=1)), k


def test_project_and_flow_command_lines_write_the_same_segmented_files_either_way(tmp_path):
    """--restart_rows 1 on the device: PIL's restart_marker_rows with --encode host, sagen_jpeg_encode_rst with --encode device; the
    folders are identical and every file holds one segment per row of MCUs.  (Through the twin: tests/test_cpu_twin_jpeg_rst.py.)"""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import flow, jpeg, project
    from test_gpu_jpeg_enc import _folder, _same_files
    src = str(tmp_path / 'in')
    _folder(src, 6, 32, 64, 4)
    for mode in ('host', 'device'):
        project.main([src, str(tmp_path / ('p_' + mode)), '--from', 'er', '--to', 'er', '--size', '24', '48', '--decode', mode, '--encode', mode, '--block', '4',
                      '--restart_rows', '1'])
        flow.main([src, str(tmp_path / ('f_' + mode)), '--levels', '2', '--iters', '4', '--decode', mode, '--encode', mode, '--block', '4',
                   '--restart_rows', '1'])
    _same_files(str(tmp_path / 'p_host'), str(tmp_path / 'p_device'))
    _same_files(str(tmp_path / 'f_host'), str(tmp_path / 'f_device'))
    info = jpeg.parse(open(str(tmp_path / 'p_device' / '000003.jpg'), 'rb').read())
    assert (info.width, info.height, info.restart_interval, info.segments.size) == (48, 24, 3, 2)
    info = jpeg.parse(open(str(tmp_path / 'f_device' / '000003.jpg'), 'rb').read())
    assert (info.width, info.height, info.restart_interval, info.segments.size) == (64, 32, 4, 2)


def test_bad_quantiser_gives_every_frame_range_and_no_bytes():
    """As without an interval: RANGE for every frame, sizes 0 (no marker either), the rows untouched."""
    import torch
    from spatialaudiogen_amd import _lib, jpeg
    names, image, data, quality, sampling, interval = fixture()
    frames = torch.as_tensor(np.stack([image['420_17x23_q75_noise_r1']] * 2, 0)).to(_dev())
    for bad in (0, 256):
        q = jpeg.quality_tables(75).copy()
        q[0, 5] = bad
        out = torch.full((2, 4096), POISON, dtype=torch.uint8, device=_dev())
        o, sizes, status = jpeg.encode_streams(frames, q, 2, 2, 4096, out, restart_interval=1)
        assert status.cpu().tolist() == [_lib.SAGEN_JPEG_ENC_ST_RANGE] * 2 and sizes.cpu().tolist() == [0, 0]
        assert bool((out == POISON).all())
    with pytest.raises(ValueError, match='frame 7'):
        enc = jpeg.JpegEncoder(_dev(), 75, restart_rows=1)
        enc.qtabs = q
        enc.encode(frames, first=7)


# ---- re-segmenting files that exist (sagen_jpeg_transcode) -----------------------------------------------------------------------------
def _transcode_inputs():
    """[(name of a fixture case, its plain file)]: what PIL writes without an interval is what the plain restatement writes
    (tests/test_jpeg_enc_host.py proves that on its fixture), so no live PIL is needed for the sources."""
    names, image, data, quality, sampling, interval = fixture()
    return [(n, JE.encode(image[n], quality[n], SUBSAMPLING[sampling[n]])) for n in names]


def test_transcode_of_a_plain_file_is_the_file_pil_writes_with_the_interval():
    """Every fixture case: the plain file of its pixels (standard tables, no interval), transcoded at the case's interval, is THE
    file PIL wrote with restart_marker_blocks - header, DRI, markers and all.  The cases of one geometry go through one call."""
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling, interval = fixture()
    src = dict(_transcode_inputs())
    groups = {}
    for n in names:
        groups.setdefault(interval[n], []).append(n)
    for R, members in sorted(groups.items()):
        got = jpeg.transcode_files([src[n] for n in members], 0, _dev(), R)
        for n, g in zip(members, got):
            assert g == data[n], (n, R)
    n = '420_40x72_q95_noise_rrow'
    assert jpeg.transcode_files([src[n]], 1, _dev()) == [data[n]]                 # rows: rows x MCUs per row
    with pytest.raises(ValueError, match='65535'):
        jpeg.transcode_files([src[n]], 0, _dev(), 65536)


def test_transcode_of_optimised_and_of_segmented_files_keeps_the_pixels():
    """A file with tables of its own (PIL's optimize=True) and files that already hold another interval: PIL decodes the result to
    the pixels of the source, parse shows the new segments, the old DRI is gone and the tables are the standard ones; a file outside
    the decoder's scope (progressive) passes through byte for byte with one warning."""
    import warnings
    from PIL import Image
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling, interval = fixture()
    pixels = lambda d: np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
    for n in ('420_48x64_q95_noise_r1', '422_40x72_q75_saturated_r2', '444_24x40_q1_smooth_r1', 'grey_48x64_q75_noise_r1', '420_9x33_q95_smooth_r1'):
        sub = {} if sampling[n] == 'grey' else dict(subsampling=SUBSAMPLING[sampling[n]])
        b = io.BytesIO()
        Image.fromarray(image[n]).save(b, 'JPEG', quality=quality[n], optimize=True, **sub)
        prog = io.BytesIO()
        Image.fromarray(image[n]).save(prog, 'JPEG', quality=quality[n], progressive=True, **sub)
        sources = [b.getvalue(), data[n], prog.getvalue(), pil_file(image[n], quality[n], sampling[n], restart_marker_blocks=3)]
        assert jpeg.parse(sources[0]).actabs[0] != jpeg.parse(data[n]).actabs[0]          # tables of its own
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            got = jpeg.transcode_files(sources, 1, _dev())
        assert [w.category for w in caught if issubclass(w.category, UserWarning)] == [jpeg.JpegFallbackWarning]     # (not gc's ResourceWarnings)
        assert got[2] == sources[2]
        mx, my = mcus_of(image[n], sampling[n])
        for k in (0, 1, 3):
            info = jpeg.parse(got[k])
            assert (info.restart_interval, info.segments.size) == (mx, my), (n, k)
            assert got[k].count(b'\xff\xdd\x00\x04') == 1 and info.dctabs == jpeg.parse(data[n]).dctabs and info.actabs == jpeg.parse(data[n]).actabs
            assert all(np.array_equal(a, b) for a, b in zip(info.qtabs, jpeg.parse(sources[k]).qtabs))
            assert np.array_equal(pixels(got[k]), pixels(sources[k])), (n, k)
        # the standard-table sources come back as the file PIL writes at one row
        if _turbo():
            assert got[1] == got[3] == pil_file(image[n], quality[n], sampling[n], restart_marker_rows=1)


def _turbo():
    from test_jpeg_enc_host import turbo
    return turbo()


def _truncated_case():
    """three sources of one geometry, the middle one cut in the middle of its scan -> (sources, the expected streams of the outer two)"""
    names, image, data, quality, sampling, interval = fixture()
    src = dict(_transcode_inputs())
    members = ['420_17x23_q75_noise_r1', '420_17x23_q75_smooth_r1', '420_17x23_q75_saturated_r1']
    files = [src[n] for n in members]
    at = len(files[1]) - 2 - len(plain_scan_of(files[1])) // 2
    files[1] = files[1][:at] + b'\xff\xd9'
    return files, [scan_of(data[members[0]]), scan_of(data[members[2]])]


def test_a_truncated_source_sets_its_decode_bits_and_leaves_its_neighbours_exact():
    import torch
    from spatialaudiogen_amd import _lib, jpeg
    files, want = _truncated_case()
    packed = jpeg.pack(files, [jpeg.parse(f) for f in files])
    stride = 4096
    out, sizes, status = jpeg.transcode_streams(packed, torch.as_tensor(packed.buffer).to(_dev()), 1, stride)
    out, sizes, status = out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()
    assert status[0] == 0 and status[2] == 0 and status[1] & 255 and not status[1] >> 8, status
    assert 'overrun' in jpeg.transcode_status_text(int(status[1]))
    for j, w in ((0, want[0]), (2, want[1])):
        assert sizes[j] == len(w) and out[j, :len(w)].tobytes() == w, j
    with pytest.raises(IOError, match='item 1'):
        jpeg.transcode_files(files, 1, _dev())
    # the capacity rule across the two status halves: a stride of 64 is too small for the noise frame only
    out, sizes, status = jpeg.transcode_streams(packed, torch.as_tensor(packed.buffer).to(_dev()), 1, 64)
    status, sizes = status.cpu().numpy(), sizes.cpu().numpy()
    assert status[0] == _lib.SAGEN_JPEG_ENC_ST_CAPACITY << 8 and sizes[0] == len(want[0]) and status[1] & 255


def test_transcode_of_a_plain_file_that_did_not_fit_is_redone_at_the_bound(monkeypatch):
    """transcode_files' own guess of the stride never falls short on small files, so the block call is given 64 bytes here: the 16 x 16
    noise file does not fit, the flat one does; the noise file is redone alone at the bound, and both files are those of the plain call."""
    from spatialaudiogen_amd import jpeg
    noise = np.random.RandomState(12).randint(0, 256, (16, 16, 3)).astype(np.uint8)
    files = [JE.encode(noise, 95, '4:2:0'), JE.encode(np.full_like(noise, 90), 95, '4:2:0')]
    want = jpeg.transcode_files(files, 1, _dev())
    real, calls = jpeg.transcode_streams, []

    def short(packed, staged, interval, stride):
        """the first call's streams are cut at 64 bytes, in rows of the stride that was asked for"""
        import torch
        calls.append((packed.n, stride))
        if len(calls) > 1:
            return real(packed, staged, interval, stride)
        out, sizes, status = real(packed, staged, interval, 64)
        wide = torch.zeros((packed.n, stride), dtype=torch.uint8, device=out.device)
        wide[:, :64] = out
        return wide, sizes, status
    monkeypatch.setattr(jpeg, 'transcode_streams', short)
    assert jpeg.transcode_files(files, 1, _dev()) == want
    assert [n for n, _ in calls] == [2, 1] and calls[1][1] >= len(plain_scan_of(want[0]))


def test_transcode_on_the_device_equals_the_twin():
    """The four kinds of source above in calls on the device and, through the bare C ABI on numpy buffers, on the CPU twin: sizes,
    status and every byte.  (Needs the device; through the twin alone it would compare the twin with itself.)"""
    import ctypes as C
    import torch
    from PIL import Image
    assert torch.cuda.is_available()
    from spatialaudiogen_amd import _lib, build, jpeg
    ensure_lib()
    names, image, data, quality, sampling, interval = fixture()
    src = dict(_transcode_inputs())
    l = C.CDLL(build.build_cpu_twin())
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith('sagen_jpeg_transcode'):
            getattr(l, name).restype, getattr(l, name).argtypes = res, args
    n = '420_48x64_q95_noise_r1'
    b = io.BytesIO()
    Image.fromarray(image[n]).save(b, 'JPEG', quality=95, optimize=True, subsampling='4:2:0')
    calls = [([src[n], b.getvalue(), data[n], src['420_48x64_q95_smooth_rrow']], 3), (_truncated_case()[0], 1), ([src['grey_48x64_q75_noise_r1']], 1),
             ([src['422_40x72_q75_saturated_r2'], data['422_40x72_q75_saturated_r2']], 0)]
    for files, R in calls:
        packed = jpeg.pack(files, [jpeg.parse(f) for f in files])
        w, h, comps, hs, vs = packed.geometry
        stride = 8192
        got = [t.cpu().numpy() for t in jpeg.transcode_streams(packed, torch.as_tensor(packed.buffer).to('cuda'), R, stride)]
        buf = np.zeros(packed.buffer.size + 64, np.uint8)
        base = (buf.ctypes.data + 63) // 64 * 64
        off = base - buf.ctypes.data
        buf[off:off + packed.buffer.size] = packed.buffer
        nf = packed.n
        out, sizes, status = np.zeros((nf, stride), np.uint8), np.full(nf, -1, np.int32), np.full(nf, -1, np.int32)
        need = l.sagen_jpeg_transcode_scratch_bytes(nf, w, h, comps, hs, vs, packed.n_hufftabs, R, stride)
        scratch = np.zeros(need // 8 + 2, np.float64)
        sc = (scratch.ctypes.data + 15) // 16 * 16
        assert l.sagen_jpeg_transcode(base + packed.bytes_at, packed.total_bytes, base + packed.frames_at, nf, base + packed.segments_at, packed.n_segments,
                                      base + packed.hufftabs_at, packed.n_hufftabs, w, h, comps, hs, vs, R, out.ctypes.data, stride, sizes.ctypes.data,
                                      status.ctypes.data, sc, need, None) == 0
        assert np.array_equal(got[1], sizes) and np.array_equal(got[2], status), (R, got[1], sizes, got[2], status)
        for f in range(nf):
            if status[f] == 0:
                assert np.array_equal(got[0][f, :sizes[f]], out[f, :sizes[f]]), (R, f)


def test_jpeg_restart_command_line(tmp_path, capsys):
    """python -m spatialaudiogen_amd.jpeg restart: every file of the folder with one segment per MCU row, the pixels PIL sees
    unchanged; the refusals in front of any file."""
    from PIL import Image
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling, interval = fixture()
    src, dst = str(tmp_path / 'in'), str(tmp_path / 'out')
    os.makedirs(src)
    rs = np.random.RandomState(3)
    for k in range(5):
        Image.fromarray(rs.randint(0, 256, (40, 56, 3)).astype(np.uint8)).save(os.path.join(src, '%06d.jpg' % k), quality=90, optimize=k % 2 == 1)
    jpeg.main(['restart', src, dst, '--block', '2'])
    said = capsys.readouterr().out
    before = sum(os.path.getsize(os.path.join(src, f)) for f in os.listdir(src))
    after = sum(os.path.getsize(os.path.join(dst, f)) for f in os.listdir(dst))
    assert 'wrote 5 files' in said and '%d bytes before, %d after' % (before, after) in said
    assert sorted(os.listdir(dst)) == sorted(os.listdir(src))
    for f in os.listdir(src):
        info = jpeg.parse(open(os.path.join(dst, f), 'rb').read())
        assert (info.restart_interval, info.segments.size) == (4, 3), f
        assert np.array_equal(np.asarray(Image.open(os.path.join(dst, f))), np.asarray(Image.open(os.path.join(src, f)))), f
    with pytest.raises(SystemExit) as e:
        jpeg.main(['restart', src, dst])
    assert '--overwrite' in str(e.value.code)
    jpeg.main(['restart', src, dst, '--blocks', '2', '--overwrite'])
    assert jpeg.parse(open(os.path.join(dst, '000000.jpg'), 'rb').read()).segments.size == 6
    for bad in (['restart', src, src], ['restart', str(tmp_path / 'none'), dst], ['restart', src, dst, '--rows', '0', '--overwrite']):
        with pytest.raises(SystemExit) as e:
            jpeg.main(bad)
        assert e.value.code not in (0, None)


def test_encoder_refuses_an_interval_dri_cannot_name():
    import torch
    from spatialaudiogen_amd import jpeg
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=_dev())
    with pytest.raises(ValueError, match='65535'):
        jpeg.JpegEncoder(_dev(), 75, restart_blocks=65536).encode(frames)
    with pytest.raises(ValueError):
        jpeg.JpegEncoder(_dev(), 75, restart_rows=-1)
    with pytest.raises(ValueError, match='65535'):
        jpeg.encode_streams(frames, jpeg.quality_tables(75), 2, 2, 4096, restart_interval=65536)
