"""What the media ops refuse, with which code and which message - pinned for BOTH libraries by one fixture.

The entry points of these ops are written once (csrc/op_entries.h) and compiled into libsagen_hip.so and into the CPU twin.  Every
call of the table below returns before any launch: a null operand, a size at its first illegal value, a support limit exceeded by
one, a scratch one byte short of its query, a misaligned pointer, the empty call (which returns 0 with every pointer null), and the
size queries in and out of range.  refusal_lines(lib) yields one line per call, in the manner of workspace_sizes() in test_abi.py;
tests/golden/op_refusals_v1.txt holds what libsagen_hip.so of the commit named in its first line answered, when each library
still had entry points of its own.  No GPU is needed: nothing here reaches a kernel.

Pointers are offsets into one 64-byte aligned numpy buffer; a misaligned one is 4 bytes further (2 or 1 where the rule itself asks
for 4 or 2 bytes).  Messages carry sizes only, never pointer values, so the lines are stable.

    python tests/test_op_refusals_host.py        prints the lines of the device library of the tree the file lies in
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'op_refusals_v1.txt')

_POOL = np.zeros(4096 + 64, np.uint8)
P = (_POOL.ctypes.data + 63) // 64 * 64          # a valid, 64-byte aligned address; no refused call follows it
OFF4, OFF2, OFF1 = P + 4, P + 2, P + 1
BIG40, BIG31 = (1 << 40) + 1, (1 << 31) + 1
_KEEP = []                                        # whatever a row points at stays alive


def _arr(values, dtype):
    a = np.ascontiguousarray(values, dtype=dtype)
    _KEEP.append(a)
    return a.ctypes.data


def _struct(cls, **kw):
    s = cls()
    for k, v in kw.items():
        setattr(s, k, v)
    _KEEP.append(s)
    return s


def _addr(s):
    return C.addressof(s)


def _projection(kind, **kw):
    from spatialaudiogen_amd._lib import SagenProjection
    faces = kw.pop('faces', None)
    s = _struct(SagenProjection, kind=kind, **kw)
    if kind in (1, 2):                            # cube maps: six 4 x 4 cells at the origin unless a row says otherwise
        for f in range(6):
            s.face[f].w = s.face[f].h = 4
        for f, fields in (faces or {}).items():
            for k, v in fields.items():
                setattr(s.face[f], k, v)
    return _addr(s)


def _flow_params(**kw):
    from spatialaudiogen_amd._lib import SagenFlowParams
    return _addr(_struct(SagenFlowParams, **dict(dict(levels=2, warps=1, iters=1, wrap=0, fuse=0, alpha=1.0), **kw)))


def _sources(pt_off=(0, 2, 3), nframes=(100, 120), duration=(1.0, 1.2)):
    return dict(pt_off=_arr(pt_off, np.int32), nframes=_arr(nframes, np.int64), duration=_arr(duration, np.float64))


def table(lib):
    """[(op, argument names, valid arguments, [(case, overrides)])]: a valid call would launch and is never made; every row overrides
    what makes it return early.  A case named empty* returns 0, every other one a negative code."""
    q = lambda name, *a: int(getattr(lib, name)(*a))
    null = lambda *names: [('null_' + n, {n: None}) for n in names]
    all_null = lambda names: {n: None for n in names}
    ops = []

    names = ('p', 'q', 'n_maps', 'nodes', 'cost', 'emd', 'not_converged', 'stream')
    ops.append(('sagen_eval_emd', names, dict(p=P, q=P, n_maps=2, nodes=8, cost=P, emd=P, not_converged=P, stream=None),
                null('p', 'q', 'cost', 'emd', 'not_converged') + [
                    ('n_maps_0', dict(n_maps=0)), ('nodes_0', dict(nodes=0)), ('nodes_97', dict(nodes=97)),
                    ('cost_misaligned', dict(cost=OFF4)), ('emd_misaligned', dict(emd=OFF4)), ('not_converged_misaligned', dict(not_converged=OFF2))]))

    names = ('x', 'n_hist', 'n', 'channels', 'taps', 'outputs', 'ntaps', 'rot', 'n_rot', 'rot_hop', 'pos0', 'zero_before', 'y', 'stream')
    ops.append(('sagen_render_fir', names,
                dict(x=P, n_hist=0, n=16, channels=4, taps=P, outputs=2, ntaps=8, rot=None, n_rot=0, rot_hop=0, pos0=0, zero_before=0, y=P, stream=None),
                null('x', 'taps', 'y') + [
                    ('n_hist_-1', dict(n_hist=-1)), ('n_0', dict(n=0)), ('channels_0', dict(channels=0)), ('outputs_0', dict(outputs=0)),
                    ('ntaps_0', dict(ntaps=0)), ('pos0_-1', dict(pos0=-1)), ('history_before_the_start', dict(n_hist=1, pos0=0)),
                    ('rot_n_rot_0', dict(rot=P, n_rot=0, rot_hop=1)), ('rot_hop_0', dict(rot=P, n_rot=1, rot_hop=0)),
                    ('channels_5', dict(channels=5)), ('outputs_33', dict(outputs=33)), ('ntaps_513', dict(ntaps=513)),
                    ('n_above_2^40', dict(n=BIG40)), ('x_misaligned', dict(x=OFF4))]))

    names = ('ambi', 'n_rows', 'channels', 'stride', 'window', 'sh', 'p', 'rms', 'scratch', 'scratch_bytes', 'stream')
    need = q('sagen_power_map_windows_scratch_bytes', 2, 4)
    ops.append(('sagen_power_map_windows', names,
                dict(ambi=P, n_rows=8, channels=4, stride=2, window=2, sh=P, p=2, rms=P, scratch=P, scratch_bytes=need, stream=None), [
                    ('n_rows_-1', dict(n_rows=-1)), ('stride_0', dict(stride=0)), ('window_0', dict(window=0)), ('p_0', dict(p=0)),
                    ('channels_5', dict(channels=5)),
                    ('empty_no_map_fits', dict(all_null(('ambi', 'sh', 'rms', 'scratch')), n_rows=2, scratch_bytes=0))] +
                null('ambi', 'sh', 'rms') + [
                    ('maps_above_2^31-1', dict(n_rows=1 << 31, stride=1, window=1)),
                    ('null_scratch', dict(scratch=None)), ('scratch_one_short', dict(scratch_bytes=need - 1)),
                    ('scratch_misaligned', dict(scratch=OFF4)), ('ambi_misaligned', dict(ambi=OFF4))]))

    names = ('maps', 'n_maps', 'map0', 'mh', 'mw', 'lut', 'frames', 'n_frames', 'frame0', 'h', 'w', 'frames_per_map', 'out', 'scratch',
             'scratch_bytes', 'stream')
    need = q('sagen_overlay_blend_scratch_bytes', 2, 1, 2, 3)
    ops.append(('sagen_overlay_blend', names,
                dict(maps=P, n_maps=2, map0=0, mh=1, mw=2, lut=P, frames=P, n_frames=3, frame0=0, h=1, w=2, frames_per_map=5, out=P, scratch=P,
                     scratch_bytes=need, stream=None), [
                    ('n_maps_-1', dict(n_maps=-1)), ('map0_-1', dict(map0=-1)), ('mh_0', dict(mh=0)), ('mw_0', dict(mw=0)),
                    ('n_frames_-1', dict(n_frames=-1)), ('frame0_-1', dict(frame0=-1)), ('h_0', dict(h=0)), ('w_0', dict(w=0)),
                    ('frames_per_map_0', dict(frames_per_map=0)),
                    ('empty_no_frames', dict(all_null(('maps', 'lut', 'frames', 'out', 'scratch')), n_frames=0, frame0=99, scratch_bytes=0))] +
                null('maps', 'lut', 'frames', 'out') + [
                    ('cur_map_not_given', dict(frame0=3)), ('prev_map_not_given', dict(map0=1)),
                    ('mw_1001', dict(mw=1001)), ('mh_4097', dict(mh=4097)), ('h_65536', dict(h=65536)), ('w_2^20+1', dict(w=(1 << 20) + 1)),
                    ('n_frames_65536', dict(n_frames=65536, frames_per_map=100000)),
                    ('null_scratch', dict(scratch=None)), ('scratch_one_short', dict(scratch_bytes=need - 1)),
                    ('scratch_misaligned', dict(scratch=OFF4)), ('lut_misaligned', dict(lut=OFF4))]))

    fill_rows = [('null_ctrl', dict(ctrl=None)), ('null_pt_off', dict(pt_off=None)), ('null_nframes', dict(nframes=None)),
                 ('null_duration', dict(duration=None)), ('n_sources_0', dict(n_sources=0)), ('rate_0', dict(rate=0.0)), ('t0_-1', dict(t0=-1)),
                 ('n_sources_65', dict(n_sources=65)), ('pt_off_negative', _sources(pt_off=(-1, 2, 3))),
                 ('pt_off_not_increasing', _sources(pt_off=(0, 0, 3))), ('nframes_0', _sources(nframes=(100, 0))),
                 ('duration_0', _sources(duration=(0.0, 1.2)))]

    names = ('ctrl', 'pt_off', 'nframes', 'duration', 'n_sources', 'rate', 't0', 'n', 'stride', 'dirs', 'n_dirs', 'unit', 'nearest', 'stream')
    ops.append(('sagen_source_track', names,
                dict(_sources(), ctrl=P, n_sources=2, rate=100.0, t0=0, n=10, stride=2, dirs=P, n_dirs=4, unit=P, nearest=P, stream=None), [
                    ('null_unit_and_nearest', dict(unit=None, nearest=None)), ('nearest_without_dirs', dict(dirs=None)),
                    ('n_0', dict(n=0)), ('stride_0', dict(stride=0)), ('n_dirs_0', dict(n_dirs=0)), ('n_dirs_4097', dict(n_dirs=4097)),
                    ('n_above_2^31/64', dict(n=(1 << 31) // 64 + 1))] + fill_rows + [('past_the_shortest_source', dict(n=51))]))

    names = ('signals', 'ld', 'ctrl', 'pt_off', 'nframes', 'duration', 'n_sources', 'rate', 'channels', 'distance_model', 'radius', 't0', 'n',
             'ambi', 'stream')
    ops.append(('sagen_encode_sources', names,
                dict(_sources(), signals=P, ld=120, ctrl=P, n_sources=2, rate=100.0, channels=4, distance_model=0, radius=0.0, t0=0, n=10, ambi=P,
                     stream=None),
                null('signals', 'ambi') + [
                    ('n_0', dict(n=0)), ('ld_0', dict(ld=0)), ('channels_0', dict(channels=0)), ('channels_5', dict(channels=5)),
                    ('n_above_2^31', dict(n=BIG31)), ('distance_model_2', dict(distance_model=2)),
                    ('distance_model_1_radius_0', dict(distance_model=1, radius=0.0))] + fill_rows + [
                    ('past_the_shortest_source', dict(n=101)), ('ld_shorter_than_a_source', dict(ld=119)), ('ambi_misaligned', dict(ambi=OFF4))]))

    names = ('signals', 'ld', 'ctrl', 'pt_off', 'nframes', 'duration', 'n_sources', 'rate', 'mode', 'dirs', 'hrir', 'n_dirs', 'ntaps',
             'zero_before', 't0', 'n', 'y', 'stream')
    ops.append(('sagen_binauralize_sources', names,
                dict(_sources(), signals=P, ld=120, ctrl=P, n_sources=2, rate=100.0, mode=1, dirs=P, hrir=P, n_dirs=4, ntaps=8, zero_before=0, t0=0,
                     n=10, y=P, stream=None),
                null('signals', 'y') + [
                    ('mode_2', dict(mode=2)), ('hrir_null_dirs', dict(dirs=None)), ('hrir_null_hrir', dict(hrir=None)),
                    ('n_0', dict(n=0)), ('ld_0', dict(ld=0)), ('n_dirs_0', dict(n_dirs=0)), ('ntaps_0', dict(ntaps=0)),
                    ('n_dirs_4097', dict(n_dirs=4097)), ('ntaps_513', dict(ntaps=513)), ('n_above_2^31', dict(n=BIG31))] + fill_rows + [
                    ('past_the_shortest_source', dict(n=101)), ('ld_shorter_than_a_source', dict(ld=119)), ('y_misaligned', dict(y=OFF4)),
                    ('mic_y_misaligned', dict(mode=0, dirs=None, hrir=None, n_dirs=0, ntaps=0, y=OFF4))]))

    names = ('src', 'n', 'src_h', 'src_w', 'src_proj', 'dst', 'dst_h', 'dst_w', 'dst_proj', 'rot', 'n_rot', 'supersample', 'scratch',
             'scratch_bytes', 'stream')
    er = _projection(0)
    ops.append(('sagen_reproject', names,
                dict(src=P, n=2, src_h=8, src_w=16, src_proj=er, dst=P, dst_h=8, dst_w=16, dst_proj=er, rot=None, n_rot=0, supersample=1,
                     scratch=None, scratch_bytes=0, stream=None), [
                    ('n_-1', dict(n=-1)), ('src_h_0', dict(src_h=0)), ('src_w_0', dict(src_w=0)), ('dst_h_0', dict(dst_h=0)), ('dst_w_0', dict(dst_w=0)),
                    ('empty_no_frames', dict(all_null(('src', 'src_proj', 'dst', 'dst_proj')), n=0))] +
                null('src', 'dst', 'src_proj', 'dst_proj') + [
                    ('null_rot', dict(n_rot=1)), ('supersample_0', dict(supersample=0)), ('supersample_9', dict(supersample=9)),
                    ('src_h_16385', dict(src_h=16385)), ('src_w_16385', dict(src_w=16385)), ('dst_h_16385', dict(dst_h=16385)),
                    ('dst_w_16385', dict(dst_w=16385)), ('n_65536', dict(n=65536)), ('n_rot_3', dict(rot=P, n_rot=3)),
                    ('unknown_kind', dict(src_proj=_projection(7))), ('view_as_source', dict(src_proj=_projection(3, hfov=1.0))),
                    ('rectangle_outside', dict(dst_proj=_projection(0, w=17, h=8))), ('view_hfov_0', dict(dst_proj=_projection(3, hfov=0.0))),
                    ('face_not_square', dict(src_proj=_projection(1, faces={0: dict(h=5)}))),
                    ('face_outside', dict(src_proj=_projection(2, faces={5: dict(x0=13)}))),
                    ('face_orient_8', dict(dst_proj=_projection(1, faces={2: dict(orient=8)}))),
                    ('rot_misaligned', dict(rot=OFF4, n_rot=1))]))

    names = ('frames', 'n_frames', 'h', 'w', 'p', 'flow', 'scratch', 'scratch_bytes', 'stream')
    need = q('sagen_optical_flow_scratch_bytes', 3, 16, 16, 2)
    ops.append(('sagen_optical_flow', names,
                dict(frames=P, n_frames=3, h=16, w=16, p=_flow_params(), flow=P, scratch=P, scratch_bytes=need, stream=None), [
                    ('n_frames_-1', dict(n_frames=-1)),
                    ('empty_no_frames', dict(all_null(('frames', 'p', 'flow', 'scratch')), n_frames=0, scratch_bytes=0)),
                    ('empty_one_frame', dict(all_null(('frames', 'p', 'flow', 'scratch')), n_frames=1, scratch_bytes=0))] +
                null('frames', 'p', 'flow', 'scratch') + [
                    ('warps_0', dict(p=_flow_params(warps=0))), ('warps_17', dict(p=_flow_params(warps=17))),
                    ('iters_0', dict(p=_flow_params(iters=0))), ('iters_1001', dict(p=_flow_params(iters=1001))),
                    ('fuse_-1', dict(p=_flow_params(fuse=-1))), ('fuse_9', dict(p=_flow_params(fuse=9))),
                    ('alpha_0', dict(p=_flow_params(alpha=0.0))), ('alpha_inf', dict(p=_flow_params(alpha=float('inf')))),
                    ('h_0', dict(h=0)), ('w_0', dict(w=0)), ('levels_0', dict(p=_flow_params(levels=0))), ('levels_9', dict(p=_flow_params(levels=9))),
                    ('h_4097', dict(h=4097, p=_flow_params(levels=1))), ('w_4097', dict(w=4097, p=_flow_params(levels=1))),
                    ('n_frames_65536', dict(n_frames=65536)), ('h_17_not_divisible', dict(h=17)), ('h_4_coarsest_too_small', dict(h=4)),
                    ('scratch_one_short', dict(scratch_bytes=need - 1)), ('scratch_misaligned', dict(scratch=OFF4))]))

    names = ('flow', 'n', 'h', 'w', 'rgb', 'limits', 'scratch', 'scratch_bytes', 'stream')
    need = q('sagen_flow_encode_scratch_bytes', 2, 8, 8)
    ops.append(('sagen_flow_encode', names, dict(flow=P, n=2, h=8, w=8, rgb=P, limits=P, scratch=P, scratch_bytes=need, stream=None), [
                    ('n_-1', dict(n=-1)), ('empty_no_frames', dict(all_null(('flow', 'rgb', 'limits', 'scratch')), n=0, scratch_bytes=0)),
                    ('h_0', dict(h=0)), ('w_0', dict(w=0)), ('h_4097', dict(h=4097)), ('w_4097', dict(w=4097)), ('n_65536', dict(n=65536))] +
                null('flow', 'rgb', 'limits', 'scratch') + [
                    ('scratch_one_short', dict(scratch_bytes=need - 1)), ('scratch_misaligned', dict(scratch=OFF2))]))

    names = ('x', 'x0', 'n_in', 'c_in', 'taps', 'L', 'M', 'H', 'T', 'mix', 'c_out', 'n0', 'n', 'y', 'stream')
    ops.append(('sagen_resample_fir', names,
                dict(x=P, x0=0, n_in=100, c_in=2, taps=P, L=2, M=1, H=8, T=9, mix=None, c_out=2, n0=0, n=10, y=P, stream=None), [
                    ('n_-1', dict(n=-1)), ('empty_no_rows', dict(all_null(('x', 'taps', 'y')), n=0))] + null('taps', 'y', 'x') + [
                    ('L_0', dict(L=0)), ('M_0', dict(M=0)), ('T_0', dict(T=0)), ('H_-1', dict(H=-1)), ('x0_-1', dict(x0=-1)), ('n_in_-1', dict(n_in=-1)),
                    ('n0_-1', dict(n0=-1)), ('c_in_0', dict(c_in=0)), ('c_out_0', dict(c_out=0)), ('c_out_3_without_mix', dict(c_out=3)),
                    ('T_8_not_the_ceiling', dict(T=8)), ('c_in_65', dict(c_in=65, c_out=65)), ('c_out_65', dict(c_out=65, mix=P)),
                    ('T_4097', dict(L=1, H=2048, T=4097)), ('L_2^20+1', dict(L=(1 << 20) + 1, H=0, T=1)), ('M_2^20+1', dict(M=(1 << 20) + 1)),
                    ('table_above_64MiB', dict(L=1 << 20, H=4 << 20, T=9)),
                    ('x0_above_2^40', dict(x0=BIG40)), ('n_in_above_2^40', dict(n_in=BIG40)), ('n0_above_2^40', dict(n0=BIG40)),
                    ('n_above_2^40', dict(n=BIG40))]))

    names = ('x', 'n', 'channels', 'channel', 'first', 'hop', 'length', 'count', 'rms', 'stream')
    ops.append(('sagen_window_rms', names, dict(x=P, n=100, channels=2, channel=1, first=0, hop=10, length=10, count=5, rms=P, stream=None), [
                    ('count_-1', dict(count=-1)), ('empty_no_windows', dict(all_null(('x', 'rms')), count=0))] + null('x', 'rms') + [
                    ('n_-1', dict(n=-1)), ('channels_0', dict(channels=0)), ('channel_-1', dict(channel=-1)), ('channel_2_of_2', dict(channel=2)),
                    ('length_0', dict(length=0)), ('hop_-1', dict(hop=-1)), ('first_-1', dict(first=-1)), ('n_above_2^40', dict(n=BIG40)),
                    ('channels_2^20+1', dict(channels=(1 << 20) + 1)), ('length_101', dict(length=101)), ('first_91', dict(first=91)),
                    ('count_11_past_the_rows', dict(count=11)), ('count_2^31', dict(count=1 << 31, hop=0))]))

    names = ('bytes', 'total_bytes', 'frames', 'n', 'segments', 'n_segments', 'qtabs', 'n_qtabs', 'hufftabs', 'n_hufftabs', 'w', 'h', 'components',
             'hs', 'vs', 'out', 'status', 'scratch', 'scratch_bytes', 'stream')
    pointers = ('bytes', 'frames', 'segments', 'qtabs', 'hufftabs', 'out', 'status', 'scratch')
    need = q('sagen_jpeg_decode_scratch_bytes', 2, 16, 16, 3, 2, 2, 4)
    ops.append(('sagen_jpeg_decode', names,
                dict(bytes=P, total_bytes=64, frames=P, n=2, segments=P, n_segments=2, qtabs=P, n_qtabs=2, hufftabs=P, n_hufftabs=4, w=16, h=16,
                     components=3, hs=2, vs=2, out=P, status=P, scratch=P, scratch_bytes=need, stream=None), [
                    ('empty_no_frames', dict(all_null(pointers), n=0, scratch_bytes=0)), ('n_-1', dict(n=-1)), ('w_0', dict(w=0)), ('h_0', dict(h=0)),
                    ('components_2', dict(components=2)), ('hs_3', dict(hs=3)), ('grey_subsampled', dict(components=1)),
                    ('w_16385', dict(w=16385)), ('h_16385', dict(h=16385)), ('n_65536', dict(n=65536)),
                    ('output_above_2^31-1', dict(n=65535, w=1024, h=1024))] + null(*pointers) + [
                    ('total_bytes_-4', dict(total_bytes=-4)), ('total_bytes_6', dict(total_bytes=6)), ('total_bytes_2^31', dict(total_bytes=1 << 31)),
                    ('n_segments_1', dict(n_segments=1)), ('n_qtabs_0', dict(n_qtabs=0)), ('n_hufftabs_0', dict(n_hufftabs=0)),
                    ('n_hufftabs_65537', dict(n_hufftabs=65537)), ('n_qtabs_65537', dict(n_qtabs=65537)),
                    ('bytes_misaligned', dict(bytes=OFF2)), ('frames_misaligned', dict(frames=OFF4)), ('segments_misaligned', dict(segments=OFF2)),
                    ('qtabs_misaligned', dict(qtabs=OFF1)), ('status_misaligned', dict(status=OFF2)), ('scratch_misaligned', dict(scratch=OFF4)),
                    ('scratch_one_short', dict(scratch_bytes=need - 1))]))

    names = ('frames', 'n', 'w', 'h', 'components', 'hs', 'vs', 'qtabs', 'out', 'stride', 'sizes', 'status', 'scratch', 'scratch_bytes', 'stream')
    pointers = ('frames', 'qtabs', 'out', 'sizes', 'status', 'scratch')
    need = q('sagen_jpeg_encode_scratch_bytes', 2, 16, 16, 3, 2, 2, 1024)
    ops.append(('sagen_jpeg_encode', names,
                dict(frames=P, n=2, w=16, h=16, components=3, hs=2, vs=2, qtabs=P, out=P, stride=1024, sizes=P, status=P, scratch=P,
                     scratch_bytes=need, stream=None), [
                    ('empty_no_frames', dict(all_null(pointers), n=0, scratch_bytes=0)), ('n_-1', dict(n=-1)), ('w_0', dict(w=0)), ('h_0', dict(h=0)),
                    ('components_2', dict(components=2)), ('w_16385', dict(w=16385)), ('n_65536', dict(n=65536)),
                    ('stride_0', dict(stride=0)), ('stride_6', dict(stride=6)), ('stride_2^28+4', dict(stride=(1 << 28) + 4))] + null(*pointers) + [
                    ('out_misaligned', dict(out=OFF2)), ('sizes_misaligned', dict(sizes=OFF2)), ('status_misaligned', dict(status=OFF2)),
                    ('qtabs_misaligned', dict(qtabs=OFF1)), ('scratch_misaligned', dict(scratch=OFF4)),
                    ('scratch_one_short', dict(scratch_bytes=need - 1))]))
    return ops


# the size queries: (function, argument lists), in range first (the reprojection stages nothing: 0 either way), then out of range: 0
QUERIES = [
    ('sagen_power_map_windows_scratch_bytes', [(2, 4), (1, 9), (0, 4), (2, 5)]),
    ('sagen_overlay_blend_scratch_bytes', [(2, 1, 2, 3), (3, 90, 180, 7), (0, 1, 2, 3), (2, 0, 2, 3), (2, 1, 0, 3), (2, 1, 2, 0)]),
    ('sagen_reproject_scratch_bytes', [(1, 8, 8, 1), (0, 0, 0, 0)]),
    ('sagen_optical_flow_scratch_bytes', [(3, 16, 16, 2), (1, 16, 16, 2), (3, 0, 16, 2), (3, 16, 16, 0), (3, 16, 16, 9), (3, 4097, 16, 1),
                                          (65536, 16, 16, 1), (3, 17, 16, 2), (3, 4, 16, 2)]),
    ('sagen_flow_encode_scratch_bytes', [(2, 8, 8), (0, 8, 8)]),
    ('sagen_jpeg_decode_scratch_bytes', [(2, 16, 16, 3, 2, 2, 4), (0, 16, 16, 3, 2, 2, 4), (2, 16, 16, 3, 2, 2, 0), (2, 16, 16, 3, 2, 2, 65537),
                                         (2, 0, 16, 3, 2, 2, 4), (2, 16, 16, 2, 1, 1, 4), (2, 16385, 16, 3, 2, 2, 4)]),
    ('sagen_jpeg_encode_scratch_bytes', [(2, 16, 16, 3, 2, 2, 1024), (0, 16, 16, 3, 2, 2, 1024), (2, 16, 16, 3, 2, 2, 0), (2, 16, 16, 3, 2, 2, 6),
                                         (2, 16, 16, 3, 2, 2, (1 << 28) + 4), (2, 0, 16, 3, 2, 2, 1024)]),
    ('sagen_jpeg_encode_max_bytes', [(16, 16, 3, 2, 2), (0, 16, 3, 2, 2), (16, 16, 2, 1, 1)]),
]


def refusal_lines(lib):
    """'<op> <case> <rc> <message>' per call of the table, '<query> <arguments> <value>' per size query: what the golden file holds."""
    lines = []
    for op, names, valid, rows in table(lib):
        fn = getattr(lib, op)
        for case, over in rows:
            args = dict(valid, **over)
            rc = fn(*[args[k] for k in names])
            assert (rc == 0) == case.startswith('empty'), (op, case, rc, lib.sagen_last_error())
            lines.append(('%s %s %d %s' % (op, case, rc, lib.sagen_last_error().decode() if rc else '')).rstrip())
    for name, cases in QUERIES:
        for a in cases:
            lines.append('%s %s %d' % (name, ','.join(str(x) for x in a), int(getattr(lib, name)(*a))))
    return lines


def _bind(l):
    from spatialaudiogen_amd import _lib
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(l, name):
            getattr(l, name).restype, getattr(l, name).argtypes = res, args
    return l


@pytest.fixture(scope='module')
def device_lib():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope='module')
def twin_lib():
    from spatialaudiogen_amd import build
    return _bind(C.CDLL(build.build_cpu_twin()))


def golden():
    text = open(GOLDEN).read().split('\n')
    assert text[0].startswith('# ') and re.search(r'\b[0-9a-f]{40}\b', text[0]), 'the first line names the commit the lines come from'
    return [l for l in text[1:] if l]


def test_the_twin_refuses_as_the_device_library_of_the_fixture_did(twin_lib):
    assert refusal_lines(twin_lib) == golden()


def test_the_device_library_refuses_as_before(device_lib):
    assert refusal_lines(device_lib) == golden()


def test_every_refusal_of_the_shared_entry_points_is_reached():
    """Each fail(...) statement of csrc/op_entries.h is the message of at least one line of the fixture."""
    text = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'op_entries.h')).read()
    formats = re.findall(r'\bfail\([A-Za-z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text)
    assert len(formats) >= 60
    messages = [l.split(' ', 3)[3] for l in golden() if len(l.split(' ', 3)) == 4]
    for f in formats:
        fmt = ''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', f))
        pattern = '.*'.join(re.escape(part) for part in re.split(r'%(?:ld|zu|d|g|s)', fmt))
        assert any(re.fullmatch(pattern, m) for m in messages), 'no row of the table reaches: ' + fmt


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from spatialaudiogen_amd import _lib
    print('\n'.join(refusal_lines(_lib.lib())))
