"""W2XYZ — the deploy driver: same surface as the reference class (deploy.py:41-152) on the HIP path.

    model = W2XYZ(model_dir)                      # reads <model_dir>/train-params.txt + weights
    ambi = model.deploy(input_folder, 0., 10.)    # -> ndarray [N*4800, 4]  (W, Y, Z, X)

Host-side only: window arithmetic, batching in groups of 10 with zero-padded last group
(deploy.py:112-139 — the padding is part of the result because batch-norm runs on batch statistics),
H2D staging and the final [mono | prediction] assembly.  All tensor arithmetic runs in
libsagen_hip.so through SptAudioGen.inference_ops.  With decode='device' (--decode device) neither the
frames nor the audio windows pass through the host: feeder.DeviceFrames decodes the jpg files on the
device, feeder.DeviceAudio keeps the wav pieces there as stored, and every batch is assembled there;
only the files' bytes are staged.
"""
import os
import numpy as np

from .definitions import AUDIO, VIDEO, FLOW, NO_SEPARATION
from .model import SptAudioGen, SptAudioGenParams


def load_params(model_dir):
    """train-params.txt parser with the reference's type coercions and legacy defaults
    (myutils.py:40-85)."""
    params = {}
    with open(os.path.join(model_dir, 'train-params.txt')) as f:
        for l in f:
            if ':' in l:
                params[l.split(':')[0]] = l.strip().split(':')[1].strip()
    for k in ['encoders', 'separation']:
        params[k] = params[k].lower()
    for k in ('ambi_order', 'audio_rate', 'video_rate'):
        params[k] = int(params[k])
    params['context'] = float(params['context'])
    params['sample_dur'] = float(params.get('sample_dur', 0.1))
    params['encoders'] = [enc.strip()[1:-1] for enc in params['encoders'][1:-1].split(',')]
    params['num_sep_tracks'] = int(params.get('num_sep_tracks', '64'))
    params['fft_window'] = float(params.get('fft_window', '0.025'))

    def int_list(key, default):
        s = params.get(key, default)
        return [int(v.strip()) for v in s[1:-1].split(',')] if len(s[1:-1]) > 0 else []
    params['context_units'] = int_list('context_units', '[64, 128, 128]')
    params['freq_mask_units'] = int_list('freq_mask_units', '[]')
    params['loc_units'] = int_list('loc_units', '[256, 256]')

    class Struct(object):
        def __init__(self, **entries):
            self.__dict__.update(entries)
    return Struct(**params)


def require_first_order(ambi_order, tool):
    """The deploy, evaluate and train command lines run first-order models only: the reference's deploy.py:69,127 feeds a one-channel
    placeholder whatever the order, the evaluation's power maps are first-order spherical harmonics, and the training step implements
    order 1.  An order-2 model runs through SptAudioGen.inference_ops / evaluation_ops."""
    if int(ambi_order) != 1:
        raise SystemExit('%s: ambi_order %d is not supported by this command (first order only); a second-order model runs through '
                         'SptAudioGen.inference_ops / evaluation_ops' % (tool, int(ambi_order)))


def window_times(chunks_t, deploy_start, deploy_duration):
    """feeder.py:228-231 filters + deploy.py:106-107 shift (float64 arithmetic kept as written)."""
    ts = list(chunks_t)
    if deploy_start > 0.5:
        ts = [t for t in ts if t >= deploy_start]
    if deploy_duration is not None:
        ts = [t for t in ts if t < deploy_start + deploy_duration]
    if not ts:
        return []
    dt = ts[0] - deploy_start
    return [t - dt for t in ts]


def audio_window(audio, t, context, size, rate):
    """AudioReader.get (feeder.py:64-90) on one contiguous array: `size` samples for the window at time t, zero
    padded before/after.  The padding is derived from start_frame = int((t - context/2) * rate), but the
    samples are read from int(start)*rate + int((start - int(start)) * rate) (feeder.py:81) — one sample
    earlier whenever the fractional part truncates differently (e.g. start = 1.2 -> 57599, not 57600).  Kept:
    it is what the reference feeds the network.  audio: [n_samples, C]."""
    start_time = t - context / 2
    start_frame = int(start_time * rate)
    num_frames = int(int(np.ceil(audio.shape[0] / float(rate))) * rate)      # AudioReader.num_frames = n_files * rate
    pad_before = pad_after = 0
    if start_frame < 0:
        pad_before = abs(start_frame)
        size -= pad_before
        start_time, start_frame = 0., 0
    if start_frame + size > num_frames:
        pad_after = start_frame + size - num_frames
        size -= pad_after
    read_start = int(start_time) * int(rate) + int((start_time - int(start_time)) * rate)
    chunk = audio[read_start:read_start + max(size, 0)]
    if pad_before or pad_after:
        chunk = np.concatenate([np.zeros((pad_before, audio.shape[1]), audio.dtype), chunk,
                                np.zeros((pad_after, audio.shape[1]), audio.dtype)], 0)
    return chunk


def frame_index(t, video_rate):
    """VideoReader.get_by_index (feeder.py:121)."""
    return max(int(t * video_rate), 0)


class ClipArrays(object):
    """An in-memory clip with SampleReader's interface (feeder.py:164-265): the arrays a reader would decode
    from <folder>/ambix, /video, /flow.  audio [n, C>=1] float; video/flow [n_frames, 224, 448, 3] already
    preprocessed (x/255-0.5, myutils.py:88-89; flow de-quantised, feeder.py:147-161)."""

    def __init__(self, audio, video=None, flow=None, audio_rate=48000, video_rate=10, chunks_t=None, duration=0.1,
                 context=1.0, start_time=0.5, sample_duration=None, frames=None):
        self.audio, self.video, self.flow = audio, video, flow
        self.frames = frames        # the decoded uint8 frames [n_frames, H, W, 3] (W2XYZ.deploy_and_overlay paints on these), or None
        self.audio_rate, self.video_rate, self.context = audio_rate, video_rate, context
        self.audio_size = int(duration * audio_rate) + int(context * audio_rate) - 1
        if chunks_t is None:   # audio_pow.lst times (scraping/preprocess.py:146-153), one 1-s wav chunk per second
            n_files = int(np.ceil(audio.shape[0] / float(audio_rate)))
            chunks_t = [float('%.12g' % (i / 10. + 0.5)) for i in range((n_files - 1) * 10)]
        if start_time > 0.5:                                             # feeder.py:228-231
            chunks_t = [t for t in chunks_t if t >= start_time]
        if sample_duration is not None:
            chunks_t = [t for t in chunks_t if t < start_time + sample_duration]
        self.chunks_t = chunks_t
        self.head = -1

    def windowed(self, start_time, sample_duration):
        return ClipArrays(self.audio, self.video, self.flow, self.audio_rate, self.video_rate, None, 0.1, self.context,
                          start_time, sample_duration, self.frames)

    def get(self):
        self.head += 1
        if self.head >= len(self.chunks_t):
            return None
        t = self.chunks_t[self.head]
        out = {'id': 'clip ' + str(t), 'ambix': audio_window(self.audio, t, self.context, self.audio_size, self.audio_rate)}
        fi = frame_index(t, self.video_rate)
        if self.video is not None:
            out['video'] = self.video[fi][np.newaxis]
        if self.flow is not None:
            out['flow'] = self.flow[fi][np.newaxis]
        return out


class W2XYZ(object):
    batch_size = 10            # deploy.py:50
    duration = 0.1             # deploy.py:49
    on_saturation = 'rerun'    # fp16x2 guard (SptAudioGen.inference_ops_checked): 'rerun' on bf16 planes | 'raise'
    # batches per forward call (round 6, include/sagen.h: grouped launch): `groups` consecutive batches of 10 windows run as ONE launch per
    # layer, each batch with its own batch-norm statistics - the output is bit-identical to groups = 1 (deploy.py:141 runs one batch
    # per sess.run); batches that do not fill a group (the clip's tail, a zero-padded partial batch) run one at a time
    groups = 1

    # where the frames of a clip FOLDER are decoded and batched: 'host' (PIL in the reader, numpy batches, one H2D copy per batch) or
    # 'device' (feeder.DeviceFrames: the files' bytes go up once, jpeg.py decodes, sagen_assemble_frames builds every batch there; the
    # audio windows likewise, feeder.DeviceAudio / sagen_assemble_audio over the wav pieces as stored).
    # The model sees the same bits either way; a ClipArrays source holds decoded arrays already and ignores this
    decode = 'host'

    def __init__(self, model_dir=None, params=None, variables=None, device=None, decode='host', entropy='lane'):
        if decode not in ('host', 'device'):
            raise ValueError("decode must be 'host' or 'device', not %r" % (decode,))
        from .frames import check_entropy
        check_entropy(None, decode, entropy)
        self.decode, self.entropy = decode, entropy      # entropy: the device decoder's 'lane' or 'split' (jpeg.JpegDecoder)
        if params is None:
            params = load_params(model_dir)
        self.params = params
        num_sep = params.num_sep_tracks if params.separation != NO_SEPARATION else 1
        net_params = SptAudioGenParams(sep_num_tracks=num_sep, ctx_feats_fc_units=params.context_units,
                                       loc_fc_units=params.loc_units, sep_freq_mask_fc_units=params.freq_mask_units,
                                       sep_fft_window=params.fft_window)
        self.model = SptAudioGen(ambi_order=params.ambi_order, audio_rate=params.audio_rate,
                                 video_rate=params.video_rate, context=params.context,
                                 sample_duration=self.duration, encoders=params.encoders,
                                 separation=params.separation, params=net_params, device=device)
        self.audio_size = self.model.snd_dur + self.model.snd_contx - 1
        self.video_size = int(self.duration * params.video_rate)
        if variables is None:
            variables = self._load_variables(model_dir)
        self.model.load_variables(variables)

    @staticmethod
    def _load_variables(model_dir):
        """Weights: the TF1 checkpoint of the model directory (tensor-bundle reader, checkpoint.py), or an
        .npz keyed by the TF variable names."""
        fn = os.path.join(model_dir, 'variables.npz')
        if os.path.exists(fn):
            with np.load(fn) as z:
                return {k: z[k] for k in z.files}
        from .checkpoint import latest_checkpoint, load_checkpoint
        prefix = latest_checkpoint(model_dir)
        if prefix is None:
            raise IOError('no checkpoint (or variables.npz) found in %s' % model_dir)
        return load_checkpoint(prefix)

    def _reader(self, source, deploy_start, deploy_duration, frames=True):
        """frames=False: the reader decodes no frames (decode='device' takes only its window times: the frames come from
        feeder.DeviceFrames, the audio windows from feeder.DeviceAudio)."""
        p = self.params
        if isinstance(source, ClipArrays):
            return source.windowed(deploy_start, deploy_duration)
        from .feeder import SampleReader
        # img_prep=None: frames stay the uint8 the JPEG decoder produced; x/255 - 0.5 (myutils.py:88-89) runs on the device
        # (sagen_forward_u8), bit-identical to img_prep_fcn() + float32 cast, at a quarter of the H2D bytes
        return SampleReader(source, ambi_order=p.ambi_order, audio_rate=p.audio_rate, video_rate=p.video_rate,
                            context=p.context, duration=self.duration, return_video=frames and VIDEO in p.encoders,
                            img_prep=None, return_flow=frames and FLOW in p.encoders, start_time=deploy_start,
                            sample_duration=deploy_duration, skip_silence_thr=None, shuffle=False,
                            random_rotations=False, skip_rate=None)                   # deploy.py:91-105

    def deploy(self, input_folder, deploy_start=0., deploy_duration=10., prefetch=True):
        """deploy.py:90-152.  `input_folder` is a clip directory (or a ClipArrays).  Returns
        [n_windows*snd_dur, 4] = W,Y,Z,X."""
        return self._deploy(input_folder, deploy_start, deploy_duration, prefetch, None)[0]

    def deploy_and_render(self, input_folder, deploy_start=0., deploy_duration=10., renderer=None, prefetch=True):
        """deploy() plus the rendering the reference's --save_video path ends in (myutils.py:285-294; binauralizer.py): every forward
        call's W,Y,Z,X rows go through renderer.process (render.Renderer) on the device, in stream order, before the copy to the
        host.  Returns (ambi [N, 4] - the bits deploy() returns -, rendered [N, renderer.outputs])."""
        if renderer is None or renderer.channels != 4:
            raise ValueError('deploy_and_render needs a render.Renderer over 4 channels (W,Y,Z,X)')
        renderer.reset()
        return self._deploy(input_folder, deploy_start, deploy_duration, prefetch, renderer)

    def deploy_and_overlay(self, input_folder, deploy_start=0., deploy_duration=10., overlay=None, renderer=None, prefetch=True, encoder=None):
        """deploy() plus the picture the reference's --save_video --overlay_map path ends in (myutils.py:246-279): every forward
        call's W,Y,Z,X rows and the frames of its windows go through overlay.process (overlay.Overlay) on the device, before the
        copy to the host.  Frame F of the overlay is the frame the feeder selects for output window F (frame_index(t_F,
        video_rate), one per 0.1 s window), read as decoded from <input_folder>/video - also for a model that has no video
        encoder - or from ClipArrays.frames.  Returns (ambi [N, 4] - the bits deploy() returns -, frames [5 (n_maps - 1), H, W, 3]
        uint8) and, with a renderer, its rendering as a third item.  With an encoder (png.PngEncoder on the model's device) every forward
        call's painted frames are encoded before they leave the device, and the frames item is the list of the files' bytes, one
        complete PNG per frame, in order."""
        if overlay is None or overlay.channels != 4:
            raise ValueError('deploy_and_overlay needs an overlay.Overlay over 4 channels (W,Y,Z,X)')
        if renderer is not None and renderer.channels != 4:
            raise ValueError('deploy_and_overlay: the render.Renderer must take 4 channels (W,Y,Z,X)')
        if self.duration * self.params.video_rate != 1:
            raise ValueError('deploy_and_overlay needs one frame per output window (duration %g s x video_rate %g != 1)'
                             % (self.duration, self.params.video_rate))
        overlay.reset()
        if renderer is not None:
            renderer.reset()
        ambi, rendered, painted = self._deploy(input_folder, deploy_start, deploy_duration, prefetch, renderer, overlay, encoder)
        return (ambi, painted) if renderer is None else (ambi, painted, rendered)

    def _overlay_frames(self, source, reader):
        """frame(t) -> the decoded uint8 frame of window time t, for deploy_and_overlay."""
        rate = self.params.video_rate
        if isinstance(source, ClipArrays):
            if source.frames is None:
                raise ValueError('deploy_and_overlay: the ClipArrays holds no decoded frames (frames=...)')
            return lambda t: np.asarray(source.frames[frame_index(t, rate)])
        from .feeder import JpgFrames
        jpgs = JpgFrames(os.path.join(source, 'video'), rate)
        return lambda t: jpgs.frame(frame_index(t, rate))

    def _deploy(self, input_folder, deploy_start, deploy_duration, prefetch, renderer, overlay=None, encoder=None):
        import torch
        from . import ops
        from .feeder import BatchPrefetcher, frames_to_float
        p, m = self.params, self.model
        on_device = self.decode == 'device' and not isinstance(input_folder, ClipArrays)
        reader = self._reader(input_folder, deploy_start, deploy_duration, frames=not on_device)
        if not reader.chunks_t:
            empty = np.zeros((0, 4), np.float32), np.zeros((0, renderer.outputs if renderer else 0), np.float32)
            return empty if overlay is None else empty + ([] if encoder is not None else np.zeros((0, 0, 0, 3), np.uint8),)
        dt = reader.chunks_t[0] - deploy_start                           # deploy.py:106-107
        reader.chunks_t = [t - dt for t in reader.chunks_t]
        use_v, use_f = VIDEO in p.encoders, FLOW in p.encoders
        frame_of = self._overlay_frames(input_folder, reader) if overlay is not None and not on_device else None
        vdev = fdev = adev = None
        if on_device:       # the frames the window table references, and only those, decoded once and kept on the device; the wav pieces as stored
            from .feeder import DeviceFrames, DeviceAudio
            if self.video_size != 1:
                raise ValueError("decode='device' needs one frame per window (duration %g s x video_rate %g != 1)" % (self.duration, p.video_rate))
            adev = DeviceAudio(os.path.join(input_folder, 'ambix'), p.audio_rate, p.ambi_order, device=m.device)
            wanted = [frame_index(t, p.video_rate) for t in reader.chunks_t]
            if use_v or overlay is not None:
                vdev = DeviceFrames(os.path.join(input_folder, 'video'), 'video', device=m.device, rate=p.video_rate, entropy=self.entropy)
                vdev.ensure(min(wanted), max(wanted) + 1)
            if use_f:
                fdev = DeviceFrames(os.path.join(input_folder, 'flow'), 'flow', device=m.device, rate=p.video_rate, entropy=self.entropy)
                fdev.ensure(min(wanted), max(wanted) + 1)

        def next_chunk():
            if not on_device:
                return reader.get()
            reader.head += 1                                             # the reader's walk over chunks_t, without cutting a window
            if reader.head >= len(reader.chunks_t):
                return None
            return {'t': reader.chunks_t[reader.head]}

        def batches():                                                   # deploy.py:112-139
            while True:
                batch = []
                for _ in range(self.batch_size):
                    chunk = next_chunk()
                    if chunk is None:
                        break
                    if on_device:                                        # the frame SampleReader.sample_at would decode
                        chunk['index'] = frame_index(reader.chunks_t[reader.head], p.video_rate)
                    if frame_of is not None:
                        chunk['frame'] = frame_of(reader.chunks_t[reader.head])
                    batch.append(chunk)
                if not batch:
                    return
                n = len(batch)
                out = {'n': n}
                if not on_device:
                    audio = np.zeros((self.batch_size, self.audio_size, 1), np.float32)   # zero rows = deploy.py:125-127
                    audio[:n] = np.stack([b['ambix'] for b in batch], 0)[:, :, :1]
                    out['audio'] = audio
                if frame_of is not None:
                    out['frames'] = np.stack([b['frame'] for b in batch], 0)
                if on_device:
                    out['index'] = [b['index'] for b in batch]               # (lists: times and indices instead of arrays, nothing to pin)
                    out['times'] = [b['t'] for b in batch]
                for key, on in (('video', use_v), ('flow', use_f)):
                    if on and not on_device:
                        clip = np.stack([b[key] for b in batch], 0)
                        if clip.dtype == np.uint8 and n == self.batch_size:
                            out[key] = clip                                   # decoded frames as they are (sagen_forward_u8)
                        else:                       # a partial batch is padded with 0.0 AFTER normalisation: float frames
                            x = np.zeros((self.batch_size, 1, 224, 448, 3), np.float32)
                            x[:n] = frames_to_float(clip)
                            out[key] = x
                yield out

        src = BatchPrefetcher(batches(), depth=2 * max(1, self.groups), pin=True) if prefetch else batches()
        outs, rendered, painted = [], [], []
        G = max(1, int(self.groups))
        mg = self._grouped_model(G) if G > 1 else None

        def run(net, bs):               # one forward call over the batches `bs` (len(bs) == net.groups), results appended in order
            cat = lambda k: torch.cat([torch.as_tensor(b[k]) for b in bs], 0).to(m.device, non_blocking=True) if k in bs[0] else None
            if on_device:               # the rules of batches(): full batches give uint8 video, a partial one float frames padded with 0.0
                idx = [i for b in bs for i in b['index']]
                full = all(b['n'] == self.batch_size for b in bs)
                if not full and len(bs) != 1:
                    raise RuntimeError('a partial batch in a group of %d' % len(bs))
                pad = None if full else self.batch_size
                # the mono windows [B, 52799, 1], zero windows behind a partial batch included: one launch over the resident clip
                a_dev = adev.batch([t for b in bs for t in b['times']], p.context, self.audio_size, pad_to=pad)[0]
                v_dev = vdev.batch(idx, pad_to=pad, as_float=not full) if use_v else None
                f_dev = fdev.batch(idx, pad_to=pad) if use_f else None
            else:
                a_dev, v_dev, f_dev = cat('audio'), cat('video'), cat('flow')
            # deploy.py:141 - with the fp16x2 guard: a batch whose trunk planes clamped anything is re-run on bf16 planes
            pred = net.inference_ops_checked(a_dev, v_dev, f_dev, on_saturation=self.on_saturation)
            wyzx = ops.assemble_wyzx(a_dev[:, :, 0].contiguous(), pred, m.snd_contx)   # deploy.py:143-152
            rows = [wyzx[i * self.batch_size:i * self.batch_size + b['n']].reshape(b['n'] * m.snd_dur, 4) for i, b in enumerate(bs)]
            if renderer is not None:    # one call for everything this forward produced, in stream order, only the valid windows of a partial batch
                valid = rows[0] if len(rows) == 1 else (wyzx.reshape(-1, 4) if all(b['n'] == self.batch_size for b in bs) else torch.cat(rows, 0))
                rendered.append(renderer.process(valid).cpu().numpy())
            if overlay is not None:     # the same rows, and the frames of exactly these windows
                valid = rows[0] if len(rows) == 1 else torch.cat(rows, 0)
                if on_device:
                    frames = vdev.batch(idx)[:, 0]
                else:
                    frames = torch.cat([torch.as_tensor(b['frames']) for b in bs], 0).to(m.device, non_blocking=True)
                done = overlay.process(valid, frames)
                if encoder is not None:     # the files instead of the pixels: compressed before they cross the bus
                    painted.extend(encoder.encode(done, first=len(painted)) if done.shape[0] else [])
                else:
                    painted.append(done.cpu().numpy())
            for r in rows:
                outs.append(r.cpu().numpy())

        pending = []
        groupable = lambda b: b['n'] == self.batch_size and all(b[k].dtype == pending[0][k].dtype for k in ('video', 'flow') if k in b)
        for b in src:
            if G > 1 and (not pending or groupable(b)):
                pending.append(b)
                if len(pending) == G:
                    run(mg, pending)
                    pending = []
                continue
            for q in pending:           # a batch that cannot join the group (partial / other frame type): everything in order, singly
                run(m, [q])
            pending = []
            run(m, [b])
        for q in pending:
            run(m, [q])
        result = np.concatenate(outs, 0), (np.concatenate(rendered, 0) if renderer is not None else None)
        if overlay is None:
            return result
        if encoder is not None:
            return result + (painted,)
        painted = [f for f in painted if f.shape[0]]
        return result + (np.concatenate(painted, 0) if painted else np.zeros((0, 0, 0, 3), np.uint8),)

    def _grouped_model(self, G):
        """A second facade over the SAME device variables whose native contexts carry G batches per call (SptAudioGen(groups=G))."""
        if getattr(self, '_mg', None) is None or self._mg.groups != G:
            m = self.model
            self._mg = SptAudioGen(ambi_order=m.ambi_order, audio_rate=m.snd_rate, video_rate=m.vid_rate, context=m.context,
                                   sample_duration=m.duration, encoders=m.encoders, separation=m.separation, params=m.params,
                                   device=m.device, groups=G)
            self._mg.load_variables(m._variables)
        return self._mg


def parse_arguments(argv=None):
    """deploy.py:14-38 (the ffmpeg muxing of the 360 video is outside this path; the ambisonic wav is written, and --render adds the
    audio the reference's --save_video path ends in, rendered on the device: render.py)."""
    import argparse
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, conflict_handler='resolve')
    parser.add_argument('model_dir', help='Directory containing model snapshot.')
    parser.add_argument('input_folder', default='', help='Folder with input sample.')
    parser.add_argument('--deploy_start', default=0., type=float)
    parser.add_argument('--deploy_duration', default=10., type=float)
    parser.add_argument('--output_fn', default='output.wav', help='Output 4-channel (W,Y,Z,X) wav.')
    parser.add_argument('--gpu', type=int, default=0, help='GPU id')
    parser.add_argument('--groups', type=int, default=1,
                        help='batches of 10 windows per forward call (grouped launch: one launch per layer for all of them, each batch with '
                             'its own batch-norm statistics; output bit-identical to 1)')
    from .render import add_render_arguments
    add_render_arguments(parser)

    class Decode(argparse.Action):
        """This command decodes two things, and --decode names both, as it does in render (the ambisonic decoder) and in project / flow /
        overlay (where the frames are decoded): the value says which one is meant, and the flag may be given once for each."""

        def __call__(self, parser, namespace, value, option_string=None):
            setattr(namespace, 'frame_decode' if value in ('host', 'device') else 'decode', value)
    parser.add_argument('--decode', action=Decode, choices=('host', 'device', 'projection', 'pseudoinv'), default=None,
                        help="host | device: where the clip's frames are decoded and batched (default host: PIL in the reader threads; device: "
                             "the files' bytes go to the device, jpeg.py decodes and every batch is assembled there; same output, bit for bit).  "
                             'projection | pseudoinv: the decoder of --render ears (default pseudoinv) / speakers (default projection)')
    parser.set_defaults(frame_decode='host')
    from .frames import ENTROPY_HELP
    parser.add_argument('--entropy', default='lane', choices=['lane', 'split'], help=ENTROPY_HELP)
    parser.add_argument('--render_fn', default=None, help='Output wav of --render.')
    parser.add_argument('--overlay_dir', default=None, metavar='DIR',
                        help='paint the sound-direction heat map over the frames of <input_folder>/video and write them here as %%06d.png (overlay.py)')
    parser.add_argument('--save_maps', default=None, metavar='FILE.npz', help='with --overlay_dir: also write the raw power maps')
    parser.add_argument('--overwrite', action='store_true', help='replace frames already in --overlay_dir')
    parser.add_argument('--encode', default='host', choices=['host', 'device'],
                        help='with --overlay_dir: where the frames are compressed: host (PIL, one thread) or device (png.py: the files\' bytes come '
                             'back instead of the pixels; other bytes, the same pixels)')
    args = parser.parse_args(argv)
    if args.deploy_duration <= 0:
        args.deploy_duration = None
    if (args.render is None) != (args.render_fn is None):
        parser.error('--render and --render_fn come together')
    if args.save_maps and not args.overlay_dir:
        parser.error('--save_maps needs --overlay_dir')
    if args.encode == 'device' and not args.overlay_dir:
        parser.error('--encode device needs --overlay_dir')
    return args


def main(argv=None):
    """deploy.py:155-198 up to save_wav."""
    import torch
    from .feeder import save_wav
    from . import render
    args = parse_arguments(argv)
    from .frames import check_entropy
    check_entropy('deploy', args.frame_decode, args.entropy)
    params = load_params(args.model_dir)
    require_first_order(params.ambi_order, 'deploy')
    render.check_render_arguments(args, 4, 'deploy')
    rendering = render.rendering_from_arguments(args, 4, params.audio_rate, 'deploy') if args.render else None   # host only (HRIR files, refusals)
    if args.overlay_dir:
        from . import frames, overlay
        frames.prepare_output_dir(args.overlay_dir, args.overwrite, 'deploy')
    torch.cuda.set_device(args.gpu)
    renderer = render.Renderer(*rendering) if rendering else None
    model = W2XYZ(args.model_dir, decode=args.frame_decode, entropy=args.entropy)
    model.groups = max(1, args.groups)
    painted = None
    if args.overlay_dir:
        ov = overlay.Overlay(4, audio_rate=params.audio_rate, video_rate=params.video_rate)
        writer = frames.FrameWriter(args.overlay_dir, 'png', args.encode, ov.device)
        res = model.deploy_and_overlay(args.input_folder, args.deploy_start, args.deploy_duration, ov, renderer, encoder=writer.encoder)
        ambi_pred, painted = res[0], res[1]
        rendered = res[2] if renderer is not None else None
    elif renderer is None:
        ambi_pred = model.deploy(args.input_folder, args.deploy_start, args.deploy_duration)
    else:
        ambi_pred, rendered = model.deploy_and_render(args.input_folder, args.deploy_start, args.deploy_duration, renderer)
    save_wav(args.output_fn, ambi_pred, model.params.audio_rate)
    print('wrote %s: %d samples x 4 channels (ACN W,Y,Z,X / SN3D)' % (args.output_fn, ambi_pred.shape[0]))
    if renderer is not None:
        if args.normalize is not None:
            rendered = render.normalize_peak(rendered, args.normalize)
        save_wav(args.render_fn, rendered, model.params.audio_rate)
        print('wrote %s: %d samples x %d channels (%s)' % (args.render_fn, rendered.shape[0], rendered.shape[1], args.render))
    if painted is not None:
        if args.encode == 'device':
            writer.write_files(painted)
        else:
            writer.write(torch.as_tensor(painted))
        count = len(painted)
        if args.save_maps:
            np.savez(args.save_maps, maps=ov.maps().cpu().numpy())
        print('wrote %d frames to %s (%d maps of %dx%d)' % (count, args.overlay_dir, ov.maps().shape[0], ov.map_shape[0], ov.map_shape[1]))


if __name__ == '__main__':
    main()
