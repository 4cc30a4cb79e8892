"""Op-level Python surface over the C ABI — the counterparts of the reference's layer wrappers
(pyutils/tflib/wrappers/core.py: conv_2d :156-220, deconv_2d :96-153, fully_connected :43-93) and
of myutils.stft / istft (myutils.py:119-211).  Tensors are torch CUDA fp32, NHWC like the TF graph.
torch is only the owner of device memory and streams here; all arithmetic is in libsagen_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _twin():
    _lib.lib()
    return _lib.IS_CPU_TWIN


def _stream():
    if _twin():          # libsagen_cpu.so (SAGEN_LIB): host pointers, no stream
        return None
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, name):
    if isinstance(t, torch.Tensor) and t.dtype == torch.float64 and name == 'stats':
        return t
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_cuda != _twin()):
        raise TypeError('%s must be a %s float32 tensor' % (name, 'host (the CPU twin is loaded)' if _twin() else 'CUDA'))
    return t.contiguous()


def default_device(device=None):
    """torch.device(device); None: where the library computes - 'cuda', or 'cpu' under the CPU twin.  Loads the library either way."""
    twin = _twin()
    return torch.device(device if device is not None else ('cpu' if twin else 'cuda'))


def select_device(gpu):
    """What a command line does once every refusal is behind it: load the library and make `gpu` the current device (the CPU twin has none)."""
    if not _twin():
        torch.cuda.set_device(gpu)


def _scratch(nbytes, dev):
    return torch.empty((int(nbytes) + 255) // 256 * 64, dtype=torch.float32, device=dev)


def _scratch64(nbytes, dev):
    """nbytes rounded up to 16, in 8-byte elements: the alignment the media ops' entry points check"""
    return torch.empty((int(nbytes) + 15) // 16 * 2, dtype=torch.float64, device=dev)


def fetch_rows(out, longest):
    """out[:, :longest] on the host, through a pinned buffer"""
    if out.device.type != 'cuda':
        return out[:, :longest].numpy()
    pinned = torch.empty((out.shape[0], longest), dtype=torch.uint8, pin_memory=True)
    pinned.copy_(out[:, :longest], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return pinned.numpy()


def encode_with_retry(run, n, stride, bound, capacity, wrap, fatal=0, fatal_error=None, label=lambda k: 'frame %d' % k):
    """The protocol of the encoders that write n byte streams of unknown length into rows of `stride` bytes (jpeg.JpegEncoder, png.PngEncoder,
    jpeg.transcode_files): run(slice, stride) -> (out [k, stride] uint8, sizes [k] int32, status [k] int32) on the device, nothing
    synchronised.  One run of the whole block at `stride`, one copy of sizes + status, one copy of the streams cut at the longest; an item
    with the `capacity` bit did not fit and is run again, by itself, at `bound`, the stride that cannot be too small.
    An item with a bit of the `fatal` mask raises fatal_error(k, status), in the block call before anything is fetched.  Returns
    [wrap(stream bytes, k)]; label(k) names item k where a status persists at the bound."""
    out, sizes, status = run(slice(0, n), stride)
    both = torch.stack([sizes, status], 0).cpu().numpy()                      # the one copy of both
    sizes, status = both[0], both[1]
    for k in np.flatnonzero(status & fatal):
        raise fatal_error(int(k), int(status[k]))
    longest = int(min(sizes.max(), stride))
    data = fetch_rows(out, longest) if longest else np.zeros((n, 0), np.uint8)
    files = [wrap(data[k, :sizes[k]].tobytes(), k) for k in range(n)]
    for k in np.flatnonzero(status & capacity):
        k = int(k)
        o, sz, st = run(slice(k, k + 1), bound)
        sz, st = int(sz.cpu()[0]), int(st.cpu()[0])
        if st & fatal:
            raise fatal_error(k, st)
        if st:
            raise RuntimeError('%s: status %d at the stride that cannot be too small' % (label(k), st))
        files[k] = wrap(fetch_rows(o, sz)[0].tobytes(), k)
    return files


def stft_mag(audio, f0, f1, c0=None, c1=None):
    """myutils.stft (myutils.py:119-147) + crop + tf.abs (model.py:166-178).
    audio [B, n]; returns (mag [B,f1-f0,1024], spec [B,c1-c0,513,2] or None)."""
    audio = _f32(audio, 'audio')
    B, n = audio.shape
    mag = torch.empty(B, f1 - f0, 1024, dtype=torch.float32, device=audio.device)
    spec = None
    if c0 is not None:
        spec = torch.empty(B, c1 - c0, 513, 2, dtype=torch.float32, device=audio.device)
    check(_lib.lib().sagen_stft_mag(_ptr(audio), B, n, f0, f1, _ptr(mag), c0 or 0, c1 or 0, _ptr(spec), _stream()))
    return mag, spec


def conv_2d(x, weights, stride=1, padding='SAME', biases=None, relu=False, in_scale=None, in_shift=None,
            return_bn_stats=False, out=None, stats_out=None, planes_scratch=True):
    """tfw.conv_2d minus batch-norm (core.py:156-220).  x [B,H,W,Cin]; weights HWIO.
    With return_bn_stats the raw-output statistics for training-mode BN come back too.  out / stats_out: optional tensors to write
    into ([B,Ho,Wo,cout] float32, [2*cout] float64).  planes_scratch=False: a scratch of the size callers allocated before the
    activation planes existed (the packed filter alone) - the library then runs the fp32-activation kernels."""
    x, weights = _f32(x, 'x'), _f32(weights, 'weights')
    B, H, W, Cin = x.shape
    kh, kw, cin2, cout = weights.shape
    assert cin2 == Cin
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    pad = {'VALID': 0, 'SAME': 1}[padding]
    if pad:
        Ho, Wo = -(-H // sh), -(-W // sw)
    else:
        Ho, Wo = (H - kh) // sh + 1, (W - kw) // sw + 1
    l = _lib.lib()
    y = _out(out, (B, Ho, Wo, cout), x, 'out')
    scratch = _scratch(conv_2d_scratch_bytes(B, H, W, kh, kw, Cin, cout, planes_scratch), x.device)
    stats = None
    if stats_out is not None and not return_bn_stats:
        raise ValueError('stats_out needs return_bn_stats=True')
    if return_bn_stats:
        n_stats = int(l.sagen_bn_stats_floats(B, Ho, Wo, cout)) // 2
        if stats_out is None:
            stats = torch.zeros(n_stats, dtype=torch.float64, device=x.device)
        elif not (stats_out.dtype == torch.float64 and stats_out.device == x.device and tuple(stats_out.shape) == (n_stats,) and stats_out.is_contiguous()):
            raise TypeError('stats_out must be a contiguous float64 tensor of shape (%d,) on %s' % (n_stats, x.device))
        else:
            stats = stats_out
    check(l.sagen_conv2d(_ptr(x), B, H, W, Cin, _ptr(weights), kh, kw, cout, sh, sw, pad, _ptr(biases), int(relu),
                         _ptr(in_scale), _ptr(in_shift), _ptr(y), _ptr(stats), _ptr(scratch), scratch.numel() * 4, _stream()))
    return (y, stats) if return_bn_stats else y


def conv_2d_scratch_bytes(B, H, W, kh, kw, Cin, cout, planes=True):
    """The scratch conv_2d allocates: sagen_conv2d_scratch_bytes, or with planes=False sagen_conv2d_min_scratch_bytes - the packed
    filter alone, the size from before the activation planes, which sagen_conv2d still accepts (include/sagen.h)."""
    l = _lib.lib()
    if planes or _twin():
        return int(l.sagen_conv2d_scratch_bytes(B, H, W, kh, kw, Cin, cout))
    return int(l.sagen_conv2d_min_scratch_bytes(B, H, W, kh, kw, Cin, cout))


def bn_finalize(stats, shape, gamma, beta, eps=1e-3):
    """contrib batch_norm, is_training=True (core.py:6,209-210): -> (scale, shift)."""
    B, Ho, Wo, C_ = shape
    scale = torch.empty(C_, dtype=torch.float32, device=stats.device)
    shift = torch.empty(C_, dtype=torch.float32, device=stats.device)
    check(_lib.lib().sagen_bn_finalize(_ptr(stats), B, Ho, Wo, C_, _ptr(_f32(gamma, 'gamma')), _ptr(_f32(beta, 'beta')),
                                       eps, _ptr(scale), _ptr(shift), _stream()))
    return scale, shift


def bn_apply_relu(x, scale=None, shift=None, residual=None):
    x = _f32(x, 'x')
    y = torch.empty_like(x)
    C_ = x.shape[-1]
    check(_lib.lib().sagen_bn_apply_relu(_ptr(x), _ptr(scale), _ptr(shift), _ptr(residual), _ptr(y), x.numel() // C_, C_, _stream()))
    return y


def maxpool3x3s2(x, scale=None, shift=None):
    x = _f32(x, 'x')
    B, H, W, C_ = x.shape
    y = torch.empty(B, (H + 1) // 2, (W + 1) // 2, C_, dtype=torch.float32, device=x.device)
    check(_lib.lib().sagen_maxpool3x3s2(_ptr(x), _ptr(scale), _ptr(shift), _ptr(y), B, H, W, C_, _stream()))
    return y


def fully_connected(x, weights, biases=None, relu=False, out=None):
    """tfw.fully_connected (core.py:43-93): acts on the last axis.  out: optional tensor to write into."""
    x, weights = _f32(x, 'x'), _f32(weights, 'weights')
    K, N = weights.shape
    M = x.numel() // K
    l = _lib.lib()
    y = _out(out, tuple(x.shape[:-1]) + (N,), x, 'out')
    scratch = _scratch(l.sagen_fc_scratch_bytes(M, K, N), x.device)
    check(l.sagen_fc(_ptr(x), M, K, _ptr(weights), N, _ptr(biases), int(relu), _ptr(y), _ptr(scratch), scratch.numel() * 4, _stream()))
    return y


def deconv_2d(x, weights, stride, biases=None, relu=False, out=None):
    """tfw.deconv_2d (core.py:96-153), VALID.  weights [kh,kw,Cout,Cin].  out: optional tensor to write into."""
    x, weights = _f32(x, 'x'), _f32(weights, 'weights')
    B, H, W, Cin = x.shape
    kh, kw, cout, cin2 = weights.shape
    assert cin2 == Cin
    sh, sw = stride
    l = _lib.lib()
    y = _out(out, (B, H * sh + kh - sh, W * sw + kw - sw, cout), x, 'out')
    scratch = _scratch(l.sagen_deconv2d_scratch_bytes(kh, kw, Cin, cout, sh, sw), x.device)
    check(l.sagen_deconv2d(_ptr(x), B, H, W, Cin, _ptr(weights), kh, kw, cout, sh, sw, _ptr(biases), int(relu), _ptr(y),
                           _ptr(scratch), scratch.numel() * 4, _stream()))
    return y


def mask_istft_mix(dmask, spec, coeffs):
    """sigmoid mask x STFT -> myutils.istft -> crop -> decoder sum (model.py:326-347, 421-434).
    dmask [B,28,1024,K]; spec [B,28,513,2]; coeffs [B,3,3,K+1] -> [B,4800,3]."""
    dmask, spec, coeffs = _f32(dmask, 'dmask'), _f32(spec, 'spec'), _f32(coeffs, 'coeffs')
    B, ntr = dmask.shape[0], dmask.shape[3]
    l = _lib.lib()
    out = torch.empty(B, 4800, 3, dtype=torch.float32, device=dmask.device)
    scratch = _scratch(l.sagen_mask_istft_mix_scratch_bytes(B), dmask.device)
    check(l.sagen_mask_istft_mix(_ptr(dmask), _ptr(spec), _ptr(coeffs), B, ntr, _ptr(out), _ptr(scratch), scratch.numel() * 4, _stream()))
    return out


def power_map(ambi_wyzx, sh_matrix):
    """AmbiDecoder.decode('projection') + per-direction RMS (decoder.py:24-28, distance.py:41-52)."""
    a, sh = _f32(ambi_wyzx, 'ambi'), _f32(sh_matrix, 'sh')
    T, P = a.shape[0], sh.shape[0]
    rms = torch.empty(P + 24 + (P % 2), dtype=torch.float32, device=a.device)
    check(_lib.lib().sagen_power_map(_ptr(a), T, _ptr(sh), P, _ptr(rms), _stream()))
    return rms[:P]


def power_map_batched(ambi_wyzx, sh_matrix):
    """One RMS map per chunk (SphericalAmbisonicsVisualizer.loop_frames, distance.py:41-59): ambi [n_chunks, T, 4] -> [n_chunks, P]."""
    a, sh = _f32(ambi_wyzx, 'ambi'), _f32(sh_matrix, 'sh')
    n, T, P = a.shape[0], a.shape[1], sh.shape[0]
    rms = torch.empty(n, P, dtype=torch.float32, device=a.device)
    moments = torch.empty(n * 10, dtype=torch.float64, device=a.device)
    check(_lib.lib().sagen_power_map_batched(_ptr(a), n, T, _ptr(sh), P, _ptr(rms), _ptr(moments), _stream()))
    return rms


def power_map_windows(ambi, sh_matrix, stride, window, out=None):
    """One RMS map per `window` samples of ambi[::stride] (SphericalAmbisonicsVisualizer over myutils.py:252's ambix[::5];
    include/sagen.h: sagen_power_map_windows): ambi [n_rows, 4 or 9], sh [P, channels] -> [n_maps, P] with
    n_maps = len(ambi[::stride]) // window.  out: optional [n_maps, P] tensor to write into."""
    a, sh = _f32(ambi, 'ambi'), _f32(sh_matrix, 'sh')
    if a.dim() != 2 or sh.dim() != 2 or sh.shape[1] != a.shape[1]:
        raise ValueError('power_map_windows: ambi [rows, C] and sh [P, C] expected')
    n_rows, C_, P = a.shape[0], a.shape[1], sh.shape[0]
    n_maps = (-(-n_rows // int(stride))) // int(window)
    l = _lib.lib()
    rms = _out(out, (n_maps, P), a, 'out')
    scratch = torch.empty((int(l.sagen_power_map_windows_scratch_bytes(n_maps, C_)) + 7) // 8 + 1, dtype=torch.float64, device=a.device)
    check(l.sagen_power_map_windows(_ptr(a), n_rows, C_, int(stride), int(window), _ptr(sh), P, _ptr(rms), _ptr(scratch), scratch.numel() * 8, _stream()))
    return rms


def overlay_blend(maps, map0, lut, frames, frame0, frames_per_map):
    """myutils.py:255-279 for a run of frames (include/sagen.h: sagen_overlay_blend): maps [n_maps, mh, mw] raw rms maps in image
    orientation from absolute map index map0 on, lut [256, 3] float64, frames [n_frames, h, w, 3] uint8 from absolute frame index
    frame0 on -> the blended uint8 frames."""
    maps = _f32(maps, 'maps')
    dev_ok = lambda t: isinstance(t, torch.Tensor) and t.is_cuda != _twin()
    if not (dev_ok(lut) and lut.dtype == torch.float64 and tuple(lut.shape) == (256, 3)):
        raise TypeError('lut must be a [256, 3] float64 tensor on the maps\' device')
    if not (dev_ok(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
        raise TypeError('frames must be a [n, h, w, 3] uint8 tensor on the maps\' device')
    if maps.dim() != 3:
        raise ValueError('overlay_blend: maps [n_maps, mh, mw] expected')
    frames, lut = frames.contiguous(), lut.contiguous()
    n_maps, mh, mw = maps.shape
    n, h, w = frames.shape[:3]
    l = _lib.lib()
    out = torch.empty_like(frames)
    scratch = torch.empty((int(l.sagen_overlay_blend_scratch_bytes(n_maps, mh, mw, n)) + 7) // 8 + 2, dtype=torch.float64, device=maps.device)
    check(l.sagen_overlay_blend(_ptr(maps), n_maps, int(map0), mh, mw, _ptr(lut), _ptr(frames), n, int(frame0), h, w, int(frames_per_map),
                                _ptr(out), _ptr(scratch), scratch.numel() * 8, _stream()))
    return out


def reproject(frames, src_proj, dst_hw, dst_proj, rot=None, supersample=1, out=None):
    """Reproject 360-degree frames (include/sagen.h: sagen_reproject; scraping/utils.py:91-144, preprocess.py:51-52 and vrProjector
    in the reference): frames [n, h, w, 3] uint8, src_proj / dst_proj _lib.SagenProjection descriptors (project.py builds them),
    dst_hw the destination frame's (height, width), rot None, [3, 3] or [n, 3, 3] float64 on the frames' device (world = rot . head)
    -> [n, dst_h, dst_w, 3] uint8.  out: optional destination to write into (pixels outside the destination's rectangles keep
    their bytes; a fresh destination starts at zero)."""
    dev_ok = lambda t: isinstance(t, torch.Tensor) and t.is_cuda != _twin()
    if not (dev_ok(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
        raise TypeError('frames must be a [n, h, w, 3] uint8 tensor on %s' % ('the host (the CPU twin is loaded)' if _twin() else 'the device'))
    frames = frames.contiguous()
    n, h, w = frames.shape[:3]
    dh, dw = int(dst_hw[0]), int(dst_hw[1])
    n_rot = 0
    if rot is not None:
        if not (dev_ok(rot) and rot.dtype == torch.float64 and rot.device == frames.device and tuple(rot.shape[-2:]) == (3, 3) and rot.dim() in (2, 3)):
            raise TypeError('rot must be a [3, 3] or [n, 3, 3] float64 tensor on the frames\' device')
        rot = rot.contiguous()
        n_rot = 1 if rot.dim() == 2 else rot.shape[0]
    if out is None:
        out = torch.zeros((n, dh, dw, 3), dtype=torch.uint8, device=frames.device)
    elif not (out.dtype == torch.uint8 and out.device == frames.device and tuple(out.shape) == (n, dh, dw, 3) and out.is_contiguous()):
        raise TypeError('out must be a contiguous uint8 tensor of shape %s on %s' % ((n, dh, dw, 3), frames.device))
    l = _lib.lib()
    nbytes = int(l.sagen_reproject_scratch_bytes(n, dh, dw, int(supersample)))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=frames.device) if nbytes else None
    check(l.sagen_reproject(_ptr(frames), n, h, w, C.addressof(src_proj), _ptr(out), dh, dw, C.addressof(dst_proj), _ptr(rot), n_rot,
                            int(supersample), _ptr(scratch), nbytes, _stream()))
    return out


def optical_flow(frames, params=None):
    """Dense optical flow between consecutive frames (include/sagen.h: sagen_optical_flow; in place of the reference's offline
    FlowNet2 pass, scraping/preprocess.py:156-204): frames [n, h, w, 3] uint8, params a _lib.SagenFlowParams (flow.FlowParams.struct()
    builds one; None: levels 5, warps 3, iters 30, wrap, alpha 8) -> [max(n - 1, 0), h, w, 2] float32, flow k from frame k to k + 1."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda != _twin() and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
        raise TypeError('frames must be a [n, h, w, 3] uint8 tensor on %s' % ('the host (the CPU twin is loaded)' if _twin() else 'the device'))
    if params is None:
        params = _lib.SagenFlowParams(5, 3, 30, 1, 0, 8.)
    if not isinstance(params, _lib.SagenFlowParams):
        raise TypeError('params must be a _lib.SagenFlowParams (flow.FlowParams(...).struct())')
    frames = frames.contiguous()
    n, h, w = frames.shape[:3]
    if not 1 <= params.levels <= 8:
        raise ValueError('levels takes 1..8, got %d' % params.levels)
    if h % (1 << (params.levels - 1)) or w % (1 << (params.levels - 1)):
        raise ValueError('frames of %dx%d cannot be halved %d times (levels %d)' % (h, w, params.levels - 1, params.levels))
    out = torch.empty((max(n - 1, 0), h, w, 2), dtype=torch.float32, device=frames.device)
    if n <= 1:
        return out
    l = _lib.lib()
    nbytes = int(l.sagen_optical_flow_scratch_bytes(n, h, w, params.levels))
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=frames.device)
    check(l.sagen_optical_flow(_ptr(frames), n, h, w, C.addressof(params), _ptr(out), _ptr(scratch), nbytes, _stream()))
    return out


def flow_encode(flow):
    """The flow folder's byte coding (include/sagen.h: sagen_flow_encode; scraping/preprocess.py:183-196): flow [n, h, w, 2] float32
    -> (rgb [n, h, w, 3] uint8: angle + pi, 0, magnitude within the frame's limits; limits [n, 2] float32: the rows of
    flow_limits.npy)."""
    if not (isinstance(flow, torch.Tensor) and flow.is_cuda != _twin() and flow.dtype == torch.float32 and flow.dim() == 4 and flow.shape[3] == 2):
        raise TypeError('flow must be a [n, h, w, 2] float32 tensor on %s' % ('the host (the CPU twin is loaded)' if _twin() else 'the device'))
    flow = flow.contiguous()
    n, h, w = flow.shape[:3]
    if h < 1 or w < 1:
        raise ValueError('flow frames of %dx%d' % (h, w))
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=flow.device)
    limits = torch.empty((n, 2), dtype=torch.float32, device=flow.device)
    if n == 0:
        return rgb, limits
    l = _lib.lib()
    nbytes = int(l.sagen_flow_encode_scratch_bytes(n, h, w))
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=flow.device)
    check(l.sagen_flow_encode(_ptr(flow), n, h, w, _ptr(rgb), _ptr(limits), _ptr(scratch), nbytes, _stream()))
    return rgb, limits


def _f64(t, name):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_cuda != _twin()):
        raise TypeError('%s must be a %s float64 tensor' % (name, 'host (the CPU twin is loaded)' if _twin() else 'CUDA'))
    return t.contiguous()


def resample_fir(x, x0, taps, L, M, H, n0, n, mix=None):
    """Rational polyphase FIR (include/sagen.h: sagen_resample_fir; resample.design builds the table): x [n_in, C_in] float32 = the
    stream's rows x0 .., taps [L, T] float64, mix [C_out, C_in] float64 or None -> y [n, C_out] float32 = the outputs n0 .. n0 + n - 1.
    Rows outside the buffer count as zero."""
    x, taps = _f32(x, 'x'), _f64(taps, 'taps')
    if x.dim() != 2 or taps.dim() != 2 or taps.shape[0] != int(L):
        raise ValueError('resample_fir: x [rows, C_in] and taps [L, T] expected')
    c_in = c_out = x.shape[1]
    if mix is not None:
        mix = _f64(mix, 'mix')
        if mix.dim() != 2 or mix.shape[1] != c_in:
            raise ValueError('resample_fir: mix [C_out, %d] expected' % c_in)
        c_out = mix.shape[0]
    y = torch.empty(max(int(n), 0), c_out, dtype=torch.float32, device=x.device)
    check(_lib.lib().sagen_resample_fir(_ptr(x), int(x0), x.shape[0], c_in, _ptr(taps), int(L), int(M), int(H), taps.shape[1], _ptr(mix),
                                        c_out, int(n0), int(n), _ptr(y), _stream()))
    return y


def window_rms(x, channel, first, hop, length, count):
    """RMS of strided windows of one channel (include/sagen.h: sagen_window_rms; compute_audio_pow, scraping/preprocess.py:146-153):
    x [n, C] float32 -> [count] float64, window i = rows first + i hop .. + length - 1."""
    x = _f32(x, 'x')
    if x.dim() != 2:
        raise ValueError('window_rms: x [rows, C] expected')
    out = torch.empty(max(int(count), 0), dtype=torch.float64, device=x.device)
    check(_lib.lib().sagen_window_rms(_ptr(x), x.shape[0], x.shape[1], int(channel), int(first), int(hop), int(length), int(count),
                                      _ptr(out), _stream()))
    return out


def eval_mel_env(pred, target):
    """myutils.compute_lsd_dist / compute_envelope_dist (myutils.py:96-116) per window: pred / target [B, 4800, C] ->
    (mel_lsd [B, C], env_mse [B, C])."""
    pred, target = _f32(pred, 'pred'), _f32(target, 'target')
    B, _, C_ = pred.shape
    l = _lib.lib()
    mel = torch.empty(B, C_, dtype=torch.float32, device=pred.device)
    env = torch.empty(B, C_, dtype=torch.float32, device=pred.device)
    scratch = _scratch(l.sagen_eval_mel_env_scratch_bytes(B, C_), pred.device)
    check(l.sagen_eval_mel_env(_ptr(pred), _ptr(target), B, C_, _ptr(mel), _ptr(env), _ptr(scratch), scratch.numel() * 4, _stream()))
    return mel, env


def eval_emd(p_maps, q_maps, cost, not_converged=None):
    """emd/dir, emd/dir2 (distance.py:100-143) of map pairs p / q [n, P] on cost [P, P] (fp64 device tensor,
    ambisonics.angular_distance) -> [n, 2] fp64.  not_converged: an int32 device counter to add to (a fresh one is checked here)."""
    p, q = _f32(p_maps, 'p_maps'), _f32(q_maps, 'q_maps')
    n, P = p.shape
    if not (isinstance(cost, torch.Tensor) and cost.dtype == torch.float64 and cost.shape == (P, P)):
        raise TypeError('cost must be a [%d, %d] float64 tensor' % (P, P))
    out = torch.empty(n, 2, dtype=torch.float64, device=p.device)
    own = not_converged is None
    nc = torch.zeros(1, dtype=torch.int32, device=p.device) if own else not_converged
    check(_lib.lib().sagen_eval_emd(_ptr(p), _ptr(q.contiguous()), n, P, _ptr(cost.contiguous()), _ptr(out), _ptr(nc), _stream()))
    if own and int(nc.item()):
        raise RuntimeError('eval_emd: %d EMD problems hit the solver\'s augmentation cap' % int(nc.item()))
    return out


def assemble_wyzx(audio, ambi_yzx, snd_contx=48000):
    """deploy.py:143-152: prepend W = mono[snd_contx/2 : snd_contx/2 + snd_dur]."""
    audio, ambi_yzx = _f32(audio, 'audio'), _f32(ambi_yzx, 'ambi')
    B, n = audio.shape[0], audio.shape[1]
    dur = ambi_yzx.shape[1]
    out = torch.empty(B, dur, 4, dtype=torch.float32, device=audio.device)
    check(_lib.lib().sagen_assemble_wyzx(_ptr(audio), _ptr(ambi_yzx), _ptr(out), B, n, snd_contx, dur, _stream()))
    return out


def render_fir(x, n_hist, taps, rot=None, rot_hop=4800, pos0=0, zero_before=0):
    """The rotated FIR matrix of the renderings (include/sagen.h: sagen_render_fir; render.py builds the taps): x [n_hist + n, C] =
    n_hist rows of history then the n new rows at absolute positions pos0 .., taps [O, C, K], rot [n_rot, C, C] or None -> y [n, O];
    outputs at absolute positions < zero_before are zero."""
    x, taps = _f32(x, 'x'), _f32(taps, 'taps')
    if x.dim() != 2 or taps.dim() != 3 or taps.shape[1] != x.shape[1]:
        raise ValueError('render_fir: x [rows, C] and taps [O, C, K] expected')
    n = x.shape[0] - int(n_hist)
    O, C_, K = taps.shape
    n_rot = 0
    if rot is not None:
        rot = _f32(rot, 'rot')
        if rot.dim() != 3 or tuple(rot.shape[1:]) != (C_, C_):
            raise ValueError('render_fir: rot [n_rot, C, C] expected')
        n_rot = rot.shape[0]
    y = torch.empty(max(n, 0), O, dtype=torch.float32, device=x.device)
    check(_lib.lib().sagen_render_fir(_ptr(x), int(n_hist), n, C_, _ptr(taps), O, K, _ptr(rot), n_rot, int(rot_hop), int(pos0),
                                      int(zero_before), _ptr(y), _stream()))
    return y


# ---- moving point sources (include/sagen.h: sagen_source_track / sagen_encode_sources / sagen_binauralize_sources) ------------------
class SourceTable(object):
    """The flat arrays the three entries take: ctrl [sum P, 3] float64 on the device, and pt_off / nframes / duration on the host.
    control_points: per source a [P >= 1, 3] array of (phi, nu, r); lengths: per source the signal length N; nframes =
    int((N / float(rate)) * rate) as position.py:78-82 computes it."""

    def __init__(self, control_points, lengths, rate, device):
        import numpy as np
        pts = [np.asarray(p, np.float64).reshape(-1, 3) for p in control_points]
        if not pts or len(pts) != len(lengths) or any(len(p) < 1 for p in pts):
            raise ValueError('SourceTable: one [P >= 1, 3] control-point array and one length per source expected')
        self.n_sources, self.rate = len(pts), float(rate)
        self.pt_off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
        self.duration = np.array([int(n) / float(rate) for n in lengths], np.float64)
        self.nframes = np.array([int(d * rate) for d in self.duration], np.int64)
        self.ctrl = torch.as_tensor(np.concatenate(pts, 0)).contiguous().to(device)

    def args(self):
        host = lambda a: C.c_void_p(a.ctypes.data)
        return (_ptr(self.ctrl), host(self.pt_off), host(self.nframes), host(self.duration), self.n_sources, self.rate)


def _f64_dirs(dirs, table):
    if not (isinstance(dirs, torch.Tensor) and dirs.dtype == torch.float64 and dirs.dim() == 2 and dirs.shape[1] == 3
            and dirs.device == table.ctrl.device):
        raise TypeError('dirs must be a [D, 3] float64 tensor on the device of the sources')
    return dirs.contiguous()


def source_track(table, t0, n, stride=1, dirs=None, unit=True):
    """Direction (unit [n, S, 3] float64) and / or nearest index in dirs [D, 3] (nearest [n, S] int32) of the samples
    t0 + i stride, i < n, of every source of a SourceTable."""
    dev = table.ctrl.device
    u = torch.empty(int(n), table.n_sources, 3, dtype=torch.float64, device=dev) if unit else None
    near = None
    if dirs is not None:
        dirs = _f64_dirs(dirs, table)
        near = torch.empty(int(n), table.n_sources, dtype=torch.int32, device=dev)
    check(_lib.lib().sagen_source_track(*(table.args() + (int(t0), int(n), int(stride), _ptr(dirs), 0 if dirs is None else dirs.shape[0],
                                                       _ptr(u), _ptr(near), _stream()))))
    return u, near


def _source_signals(signals, table):
    signals = _f32(signals, 'signals')
    if signals.dim() != 2 or signals.shape[0] != table.n_sources or signals.device != table.ctrl.device:
        raise ValueError('signals [S = %d, ld] expected, on the device of the sources' % table.n_sources)
    return signals


def encode_sources(signals, table, channels, t0, n, distance_model=False, radius=1.):
    """ambi [n, channels] = sum_s g_s sig_s[t - d_s] Y(u_s(t)) for t in [t0, t0 + n) (AmbiEncoder.encode / encode_frame;
    distance_model: encode_v2 per sample)."""
    signals = _source_signals(signals, table)
    ambi = torch.empty(max(int(n), 0), int(channels), dtype=torch.float32, device=signals.device)
    check(_lib.lib().sagen_encode_sources(*((_ptr(signals), signals.shape[1]) + table.args() + (int(channels), int(bool(distance_model)),
                                                                                               float(radius), int(t0), int(n), _ptr(ambi), _stream()))))
    return ambi


def binauralize_sources(signals, table, mode, t0, n, dirs=None, hrir=None, zero_before=0):
    """y [n, 2] for t in [t0, t0 + n): mode 'mic' (VirtualStereoMic.binauralize_frame) or 'hrir' (Convolvotron; dirs [D, 3] float64,
    hrir [D, 2, K] float32, outputs below zero_before written as 0)."""
    signals = _source_signals(signals, table)
    if mode not in ('mic', 'hrir'):
        raise ValueError("binauralize_sources: mode 'mic' or 'hrir' expected")
    D = K = 0
    if mode == 'hrir':
        dirs, hrir = _f64_dirs(dirs, table), _f32(hrir, 'hrir')
        if hrir.dim() != 3 or hrir.shape[0] != dirs.shape[0] or hrir.shape[1] != 2:
            raise ValueError('binauralize_sources: hrir [D, 2, K] expected')
        D, K = hrir.shape[0], hrir.shape[2]
    else:
        dirs = hrir = None
    y = torch.empty(max(int(n), 0), 2, dtype=torch.float32, device=signals.device)
    check(_lib.lib().sagen_binauralize_sources(*((_ptr(signals), signals.shape[1]) + table.args() + (
        _lib.SAGEN_SOURCES_HRIR if mode == 'hrir' else _lib.SAGEN_SOURCES_MIC, _ptr(dirs), _ptr(hrir), D, K, int(zero_before), int(t0), int(n), _ptr(y),
        _stream()))))
    return y


# ---- backward, op level (the gradients tf.gradients builds for the wrappers above; include/sagen.h) -----------------------
def _out(out, shape, like, name):
    """The caller's output tensor (tests prefill it to see every element written) or a fresh one."""
    if out is None:
        return torch.empty(*shape, dtype=torch.float32, device=like.device)
    if not (out.dtype == torch.float32 and out.device == like.device and tuple(out.shape) == tuple(shape) and out.is_contiguous()):
        raise TypeError('%s must be a contiguous float32 tensor of shape %s on %s' % (name, tuple(shape), like.device))
    return out


def wgrad(g, d, kh, kw, stride=(1, 1), origin=(0, 0), split=True, out=None):
    """dw[th,tw,cg,cd] = sum_{b,i,j} G[b, i*sh+th+h0, j*sw+tw+w0, :] (x) D[b,i,j,:].  conv_2d: G = x, D = dy, origin = -pad_before
    -> HWIO; deconv_2d: G = dy, D = x -> [kh,kw,Cout,Cin]; fully_connected: 2-D G [M,K], D [M,N] -> [K,N]."""
    g, d = _f32(g, 'g'), _f32(d, 'd')
    if g.dim() == 2:
        g, d = g[:, None, None, :], d[:, None, None, :]
    B, HG, WG, CG = g.shape
    _, HD, WD, CD = d.shape
    l = _lib.lib()
    dw = _out(out, (kh, kw, CG, CD), g, 'out')
    scratch = _scratch(l.sagen_wgrad_scratch_bytes(kh, kw, CG, CD), g.device) if split else None
    check(l.sagen_wgrad(_ptr(g), B, HG, WG, CG, _ptr(d), HD, WD, CD, kh, kw, stride[0], stride[1], origin[0], origin[1], _ptr(dw),
                        _ptr(scratch), scratch.numel() * 4 if split else 0, _stream()))
    return dw


def conv_2d_bwd_data(dy, weights, in_hw, stride=1, padding='SAME', out=None):
    """Input gradient of conv_2d: dy [B,Ho,Wo,Cout], weights HWIO -> dx [B,H,W,Cin]."""
    dy, weights = _f32(dy, 'dy'), _f32(weights, 'weights')
    B, Ho, Wo, cout = dy.shape
    kh, kw, cin, cout2 = weights.shape
    assert cout2 == cout
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    H, W = in_hw
    l = _lib.lib()
    dx = _out(out, (B, H, W, cin), dy, 'out')
    scratch = _scratch(l.sagen_conv2d_bwd_data_scratch_bytes(kh, kw, cin, cout, sh, sw), dy.device)
    check(l.sagen_conv2d_bwd_data(_ptr(dy), B, Ho, Wo, cout, _ptr(weights), kh, kw, cin, sh, sw, {'VALID': 0, 'SAME': 1}[padding], H, W,
                                  _ptr(dx), _ptr(scratch), scratch.numel() * 4, _stream()))
    return dx


def bn_bwd(g, y, stats, gamma, beta, act=None, g2=None, eps=1e-3, want_dz=False, out=None):
    """Training-mode batch-norm backward at the raw conv output y [.., C] (stats from conv_2d(return_bn_stats=True)):
    dz = (g + g2) * (act > 0) -> (dy, dgamma, dbeta[, dz]).  out: optional (dy, dgamma, dbeta[, dz]) tensors to write into."""
    g, y = _f32(g, 'g'), _f32(y, 'y')
    C_ = y.shape[-1]
    npix = y.numel() // C_
    if out is not None and len(out) != (4 if want_dz else 3):
        raise TypeError('out must be (dy, dgamma, dbeta%s)' % (', dz' if want_dz else ''))
    out = out or (None,) * 4
    dy = _out(out[0], y.shape, y, 'out[0]')
    dz = _out(out[3], y.shape, y, 'out[3]') if want_dz else None
    dgamma = _out(out[1], (C_,), y, 'out[1]')
    dbeta = _out(out[2], (C_,), y, 'out[2]')
    scratch = torch.empty((int(_lib.lib().sagen_bn_bwd_scratch_bytes(C_)) + 7) // 8, dtype=torch.float64, device=y.device)
    check(_lib.lib().sagen_bn_bwd(_ptr(g), _ptr(g2), _ptr(act), _ptr(y), _ptr(stats), _ptr(_f32(gamma, 'gamma')), _ptr(_f32(beta, 'beta')), eps,
                                  npix, C_, _ptr(dy), _ptr(dz), _ptr(dgamma), _ptr(dbeta), _ptr(scratch), scratch.numel() * 8, _stream()))
    return (dy, dgamma, dbeta, dz) if want_dz else (dy, dgamma, dbeta)


def maxpool3x3s2_bwd(y0, stats, gamma, beta, pooled, g, g2=None, eps=1e-3):
    """Backward of maxpool3x3s2(relu(bn(y0))) to the BN output: y0 [B,H,W,C] raw conv output, pooled / g [B,Ho,Wo,C]."""
    y0 = _f32(y0, 'y0')
    B, H, W, C_ = y0.shape
    dz = torch.empty_like(y0)
    check(_lib.lib().sagen_maxpool3x3s2_bwd(_ptr(y0), _ptr(stats), _ptr(_f32(gamma, 'gamma')), _ptr(_f32(beta, 'beta')), eps, _ptr(_f32(pooled, 'pooled')),
                                            _ptr(_f32(g, 'g')), _ptr(g2), _ptr(dz), B, H, W, C_, _stream()))
    return dz


def mask_istft_mix_bwd(dmask, spec, coeffs, dpred):
    """Adjoint of mask_istft_mix: dpred [B,4800,3] -> (d_dmask [B,28,1024,K], d_coeffs [B,3,3,K+1])."""
    dmask, spec, coeffs, dpred = _f32(dmask, 'dmask'), _f32(spec, 'spec'), _f32(coeffs, 'coeffs'), _f32(dpred, 'dpred')
    B, ntr = dmask.shape[0], dmask.shape[3]
    l = _lib.lib()
    dd = torch.empty_like(dmask)
    dc = torch.empty_like(coeffs)
    scratch = _scratch(l.sagen_mask_istft_mix_bwd_scratch_bytes(B, ntr), dmask.device)
    check(l.sagen_mask_istft_mix_bwd(_ptr(dmask), _ptr(spec), _ptr(coeffs), _ptr(dpred), B, ntr, _ptr(dd), _ptr(dc), _ptr(scratch),
                                     scratch.numel() * 4, _stream()))
    return dd, dc
