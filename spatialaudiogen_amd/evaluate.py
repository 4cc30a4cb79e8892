"""Evaluation driver — the on-graph part of the reference's eval.py (eval.py:29-232) on the HIP path, sharded over
GPUs.

    torchrun --nproc-per-node 8 -m spatialaudiogen_amd.evaluate <model_dir> <db_dir> --subset_fn <list.txt>

Per clip: every 10th 0.1 s window (`skip_rate=10`, feeder.py:379), batches of 16 (eval.py:44), input = W channel with
1 s of context, target = Y,Z,X of the centre 0.1 s (eval.py:68-72), channel masks per clip (feeder.py:312-314,
`meta/audio_layouts.txt`).  Each rank owns a contiguous block of clips (whole batches stay on one GPU because
batch-norm runs on batch statistics; batches are cut from ONE global window order, so results do not depend on the number
of ranks); per-sample metric rows are written by rank 0 to `eval-detailed.txt` in the
reference's format, and the global means come from ONE all-reduce of float64 sums + count (RCCL).

By default the file holds the 18 on-graph columns (METRIC_KEYS).  With --all_metrics it holds all 28 columns of eval.py:125-132
(ALL_METRIC_KEYS, the reference's order): the metrics the reference computes on the host per sample - mel-LSD (librosa,
myutils.py:96-106), envelope distance (scipy.signal.hilbert, myutils.py:109-116) and EMD between directional RMS maps (pyemd,
distance.py:100-143) - are computed on the device too (sagen_eval_mel_env, sagen_eval_emd: exact fp64 EMD-hat), and only
per-sample scalars come back to the host.
"""
import os
from collections import OrderedDict

import numpy as np

from .definitions import VIDEO, FLOW, NO_SEPARATION
from .dist import init_process_group, shard_range, MetricReducer

BATCH_SIZE = 16            # eval.py:44
SKIP_RATE = 10             # feeder.py:379 (for_eval)
METRIC_KEYS = ['amplitude/predicted', 'amplitude/gt',
               'mse/avg', 'mse/X', 'mse/Y', 'mse/Z', 'stft/avg', 'stft/X', 'stft/Y', 'stft/Z',
               'lsd/avg', 'lsd/X', 'lsd/Y', 'lsd/Z', 'snr/avg', 'snr/X', 'snr/Y', 'snr/Z']    # eval.py:125-133 (on-graph subset)
ALL_METRIC_KEYS = ['amplitude/predicted', 'amplitude/gt',
                   'mse/avg', 'mse/X', 'mse/Y', 'mse/Z', 'stft/avg', 'stft/X', 'stft/Y', 'stft/Z',
                   'lsd/avg', 'lsd/X', 'lsd/Y', 'lsd/Z', 'mel_lsd/avg', 'mel_lsd/X', 'mel_lsd/Y', 'mel_lsd/Z',
                   'snr/avg', 'snr/X', 'snr/Y', 'snr/Z', 'env_mse/avg', 'env_mse/X', 'env_mse/Y', 'env_mse/Z',
                   'emd/dir', 'emd/dir2']                                                      # eval.py:125-132 (--all_metrics)
EMD_ANGULAR_RES = 30.0     # eval.py:190


def read_layouts(fn):
    """meta/audio_layouts.txt: '<id> WXYZ|WXY' -> channel mask over (W, Y, Z, X) (feeder.py:312-314)."""
    masks = {'WXYZ': np.array([1., 1., 1., 1.]), 'WXY': np.array([1., 1., 0., 1.])}
    out = {}
    if fn and os.path.exists(fn):
        for l in open(fn).read().splitlines():
            if l.strip():
                out[l.split()[0]] = masks[l.split()[1]]
    return out


def window_plan(db_dir, clip_ids):
    """The GLOBAL evaluation order: clips in list order, within a clip every SKIP_RATE-th window of audio_pow.lst in time
    order.  Only the (small) lists are read.  Returns [(clip_id, t)].

    The reference fills one TF queue from 4 racing reader threads (feeder.py:372-410) and dequeues 16 at a time, so its
    batch composition is not reproducible; because batch-norm runs on batch statistics the composition is part of the
    result, and this driver therefore fixes it: batch b = windows [16 b, 16 b + 16) of this order - for ANY number of ranks."""
    from .feeder import read_pow_list, select_times
    plan = []
    for yid in clip_ids:
        times, powers = read_pow_list(os.path.join(db_dir, yid, 'audio_pow.lst'))
        plan.extend((yid, t) for t in select_times(times, powers, skip_rate=SKIP_RATE))
    return plan


def batch_shard(n_windows, rank, world, partial_batch='drop'):
    """Whole batches per rank: (first_batch, end_batch, n_batches).  The trailing partial batch is dropped like the
    reference's queue drops it (dequeue_many blocks, eval.py:140-143 / feeder.py:412-419 stop with up to 31 samples
    queued) or, with partial_batch='pad', evaluated zero-padded as the LAST batch."""
    n_batches = n_windows // BATCH_SIZE + (1 if partial_batch == 'pad' and n_windows % BATCH_SIZE else 0)
    lo, hi = shard_range(n_batches, rank, world)
    return lo, hi, n_batches


class Evaluator(object):
    def __init__(self, net, params, power_maps=False, all_metrics=False):
        self.net, self.params = net, params
        self.ss = int(params.audio_rate * params.context) // 2
        self.t = int(params.audio_rate * 0.1)
        self.rows, self.ids = [], []
        self.power_maps = power_maps
        self.maps = []                    # per sample (pred map, gt map) [7,12] each (eval.py:190: ang_res=30)
        self._sh = None
        self.all_metrics = all_metrics    # + mel_lsd, env_mse, emd (ALL_METRIC_KEYS rows)
        self._cost = None

    def run_batches(self, batches, grouped_net):
        """`len(batches)` FULL batches (each (ids, ambix [16,52799,4], video, flow, masks), frames of one dtype) as ONE grouped forward
        call (round 6: SptAudioGen(groups=G): a launch per layer for all of them, every batch with its own batch-norm statistics - the
        predictions are bit-identical to run_batch's) followed by ONE metrics launch over all their windows (per-sample values)."""
        import torch
        dev = self.net.device
        cat = lambda k: None if batches[0][k] is None else torch.cat([torch.as_tensor(b[k]) for b in batches], 0).to(dev)
        a = cat(1)
        pred = grouped_net.inference_ops_checked(a[:, :, :1].contiguous(), cat(2), cat(3), on_saturation='raise')
        m = torch.as_tensor(np.concatenate([b[4].astype(np.float32) for b in batches], 0)).to(dev)
        self._finish([i for b in batches for i in b[0]], a, pred, m, a.shape[0])

    def run_batch(self, ids, ambix, video, flow, masks):
        """ambix [n<=16, 52799, 4]; masks [n, 4].  n < 16 only for the optional zero-padded final batch: its padded
        windows are dropped from the metrics but do enter the batch-norm statistics."""
        import torch
        n = ambix.shape[0]
        from .feeder import frames_to_float
        if n != BATCH_SIZE and video is not None:
            video = frames_to_float(video)              # the padding windows are 0.0 AFTER normalisation: no uint8 pixel maps to it
        pad = lambda x: x if x is None or n == BATCH_SIZE else np.concatenate([x, np.zeros((BATCH_SIZE - n,) + x.shape[1:], x.dtype)], 0)
        dev = self.net.device
        a = torch.as_tensor(pad(ambix)).to(dev)
        # (fp16x2 guard: a batch whose trunk planes clamped anything is re-run on bf16 planes - SptAudioGen.inference_ops_checked)
        pred = self.net.inference_ops_checked(a[:, :, :1].contiguous(), pad(video), pad(flow))
        m = torch.as_tensor(pad(masks.astype(np.float32))).to(dev)
        self._finish(ids, a, pred, m, n)

    def run_views(self, ids, mono, target, video, flow, masks, net=None, full=None):
        """The device feed's forward call: the windows come as the views the op wrote (mono [N,52799,1], target [N,4800,3], both on the
        device; N = 16 x the net's groups, a partial batch already padded with zero windows), masks [n <= N, 4] of the real windows.
        net: the grouped facade for more than one batch (run_batches' rules), None for one batch (run_batch's)."""
        import torch
        n, N = masks.shape[0], mono.shape[0]
        m = np.zeros((N, 4), np.float32)
        m[:n] = masks
        if net is None:
            pred = self.net.inference_ops_checked(mono, video, flow)
        else:
            pred = net.inference_ops_checked(mono, video, flow, on_saturation='raise')
        self._finish_views(ids, mono, target, pred, torch.as_tensor(m).to(self.net.device), n, full)

    def _finish(self, ids, a, pred, m, n):
        """metrics + rows of the first n windows of a forward's worth of windows (a [N,52799,4] on the device, pred [N,4800,3], m [N,4])"""
        self._finish_views(ids, a[:, :, :1], a[:, self.ss:self.ss + self.t, 1:].contiguous(), pred, m, n, a)

    def _finish_views(self, ids, mono, target, pred, m, n, full=None):
        """_finish on the views themselves: mono [N,52799,1] (or full [N,52799,4], whose channel 0 it is), target [N,4800,3] contiguous"""
        import torch
        a = full if full is not None else mono
        _, stft_ps, lsd_ps, mse_ps, snr_ps = self.net.evaluation_ops(pred, target, None, m[:, 1:])
        amp_p = pred.abs().amax(dim=(1, 2)); amp_g = target.abs().amax(dim=(1, 2))
        per = torch.stack([amp_p, amp_g], 1).cpu().numpy()
        S = [x.cpu().numpy() for x in (mse_ps, stft_ps, lsd_ps, snr_ps)]
        maps = None
        if self.power_maps or self.all_metrics:
            maps = self._power_maps(a, pred, target, m, n)
        if self.all_metrics:
            from . import ops
            mel, env = ops.eval_mel_env(pred, target)         # unmasked, as eval.py:174,182 pass pred / gt
            emd = self._emd(*maps, n)
            # eval.py:125-132 order: mse, stft, lsd, mel_lsd, snr, env_mse (each avg, X, Y, Z), then emd/dir, emd/dir2
            S = S[:3] + [mel[:n].cpu().numpy()] + S[3:] + [env[:n].cpu().numpy()]
        for i in range(n):
            row = [per[i, 0], per[i, 1]]
            for k, arr in enumerate(S):         # eval.py:155-171 appends the RAW per-sample values (no x5e3 / x100)
                v = arr[i]
                snr = k == (4 if self.all_metrics else 3)                                 # snr/avg is a nanmean (eval.py:168)
                avg = float(np.nanmean(v)) if snr and np.isfinite(v).any() else float(np.mean(v))
                row += [avg, float(v[2]), float(v[0]), float(v[1])]   # avg, X, Y, Z  (channels are Y,Z,X)
            if self.all_metrics:
                row += [float(emd[i, 0]), float(emd[i, 1])]
            self.rows.append(row)
            self.ids.append(ids[i])

    def _power_maps(self, a, pred, target, m, n):
        """Directional RMS maps of the masked WYZX prediction / ground truth of every sample - the inputs of the
        reference's EMD metric (eval.py:147-149,188-191 -> distance.py:41-59,133-143; one 0.1 s frame per sample, 30 degree
        mesh), computed on the device by sagen_power_map_batched.  Returns the device maps [N, 84] (prediction, ground truth);
        with power_maps the first n of each are kept on the host, [n, 7, 12] in eval.py's (flipud) orientation."""
        import torch
        from . import ops
        from .ambisonics import sh_matrix, mesh_shape
        if self._sh is None:
            self._sh = torch.as_tensor(sh_matrix(EMD_ANGULAR_RES), dtype=torch.float32, device=pred.device)
        mono = a[:, self.ss:self.ss + self.t, :1]
        out = []
        for x in (pred, target):
            wyzx = (torch.cat([mono, x], 2) * m[:, None, :]).contiguous()
            out.append(ops.power_map_batched(wyzx, self._sh))
            if self.power_maps:
                self.maps.append(out[-1][:n].reshape((n,) + mesh_shape(EMD_ANGULAR_RES)).flip(1).cpu().numpy())
        return out

    def _emd(self, p_maps, q_maps, n):
        """emd/dir, emd/dir2 per sample (eval.py:188-193) of the first n map pairs, on the device (sagen_eval_emd) -> [n, 2] host.
        The maps stay in the device's row order: the reference's flipud is a reflection of the elevation grid, which is symmetric,
        so the distances do not change."""
        import torch
        from . import ops
        from .ambisonics import angular_distance
        if self._cost is None:
            self._cost = torch.as_tensor(angular_distance(EMD_ANGULAR_RES), dtype=torch.float64, device=p_maps.device)
            self._not_converged = torch.zeros(1, dtype=torch.int32, device=p_maps.device)
        emd = ops.eval_emd(p_maps[:n], q_maps[:n], self._cost, self._not_converged).cpu().numpy()
        bad = int(self._not_converged.item())
        if bad:
            raise RuntimeError('EMD: %d problems hit the exact solver\'s augmentation cap (sagen_eval_emd): their values are not the optimum' % bad)
        return emd


class _ReaderCache(object):
    """SampleReaders of the most recently used clips (consecutive windows usually come from the same clip)."""

    def __init__(self, make, keep=2):
        self.make, self.keep, self.items = make, keep, OrderedDict()

    def get(self, yid):
        if yid in self.items:
            self.items.move_to_end(yid)
        else:
            self.items[yid] = self.make(yid)
            while len(self.items) > self.keep:
                self.items.popitem(last=False)
        return self.items[yid]


class DeviceFeed(object):
    """evaluate --decode device: the inputs of one forward call made on the device from the clip folders.

    Audio: the clips' wav pieces stay resident as stored (feeder.DeviceAudio, the most recently used clips), and the mono input and
    the target rows of a call are written by sagen_assemble_audio - one launch per run of consecutive windows of one clip, into slices
    of the call's two tensors; the padding windows of a partial batch ride on the last launch.  The whole windows are never built:
    the metrics and the power maps read channel 0 and the centre rows of the others only.
    Frames: evaluate takes every 10th window, so a resident range of frames (feeder.DeviceFrames.ensure) would decode ten times too
    many; exactly the files the call's windows name, of whatever clips, go through ONE JpegDecoder.decode per folder kind.  Video
    goes in as decoded (uint8); flow through sagen_assemble_frames mode 2 with the scale_lo rows of those frames; a zero-padded
    partial batch through modes 1 / 2 with padding indices (0.0 after normalisation)."""

    def __init__(self, db_dir, params, device, keep=2, entropy='lane'):
        import torch
        from .feeder import DeviceAudio, flow_table, video_table
        from .jpeg import JpegDecoder
        self.db_dir, self.params, self.device = db_dir, params, device
        self.use_v, self.use_f = VIDEO in params.encoders, FLOW in params.encoders
        self.size = int(0.1 * params.audio_rate) + int(params.context * params.audio_rate) - 1      # SampleReader.audio_size
        self.ss, self.t = int(params.audio_rate * params.context) // 2, int(params.audio_rate * 0.1)
        self.audio = _ReaderCache(lambda yid: DeviceAudio(os.path.join(db_dir, yid, 'ambix'), params.audio_rate, params.ambi_order,
                                                          device=device), keep)
        self.decoder = JpegDecoder(device, entropy=entropy) if self.use_v or self.use_f else None
        self._tables = {k: torch.as_tensor(np.ascontiguousarray(f(), dtype=np.float32)).to(device)
                        for k, f in (('video', video_table), ('flow', flow_table)) if (self.use_v if k == 'video' else self.use_f)}
        self._scale_lo = _ReaderCache(self._load_scale_lo, keep)

    def _load_scale_lo(self, yid):
        from .feeder import flow_scale_lo
        return flow_scale_lo(np.load(os.path.join(self.db_dir, yid, 'flow', 'flow_limits.npy')))

    def call(self, wins, total):
        """wins [(clip id, t)] in order, total >= len(wins) windows in the call -> (ids, mono [total,52799,1], target [total,4800,3],
        video, flow): what SampleReader.sample_at + the stacking of evaluate() + Evaluator.run_batch's padding make on the host."""
        import torch
        from .deploy import frame_index
        from .feeder import frames_batch
        p, n = self.params, len(wins)
        mono = torch.empty((total, self.size, 1), dtype=torch.float32, device=self.device)
        target = torch.empty((total, self.t, 3), dtype=torch.float32, device=self.device)
        a = 0
        while a < n:                                                    # runs of consecutive windows of one clip
            b = a + 1
            while b < n and wins[b][0] == wins[a][0]:
                b += 1
            stop = total if b == n else b                               # the padding windows ride on the last launch
            self.audio.get(wins[a][0]).batch([t for _, t in wins[a:b]], p.context, self.size, pad_to=stop - a, want=('mono', 'target'),
                                             t_off=self.ss, t_len=self.t, out={'mono': mono[a:stop], 'target': target[a:stop]})
            a = b
        frames = {}
        for kind, on in (('video', self.use_v), ('flow', self.use_f)):
            if not on:
                frames[kind] = None
                continue
            index = [frame_index(t, p.video_rate) for _, t in wins]
            decoded = self.decoder.decode([os.path.join(self.db_dir, yid, kind, '%06d.jpg' % i) for (yid, _), i in zip(wins, index)])
            if kind == 'video' and total == n:
                frames[kind] = decoded[:, None]                         # [n, 1, H, W, 3] uint8 as decoded (sagen_forward_u8)
                continue
            scale_lo = None
            if kind == 'flow':
                scale_lo = torch.as_tensor(np.ascontiguousarray(np.stack([self._scale_lo.get(yid)[i] for (yid, _), i in zip(wins, index)], 0))).to(self.device)
            frames[kind] = frames_batch(decoded, self._tables[kind], 2 if kind == 'flow' else 1, pad_to=total, scale_lo=scale_lo)
        return ['%s %s' % (yid, t) for yid, t in wins], mono, target, frames['video'], frames['flow']


def evaluate(model_dir, db_dir, subset_fn=None, layouts_fn=None, variables=None, params=None, overwrite=True,
             partial_batch='drop', power_maps=False, groups=1, all_metrics=False, decode='host', entropy='lane'):
    """decode: 'host' (SampleReader: numpy windows, PIL frames, one upload per batch) or 'device' (DeviceFeed); the rows written are the
    same, line for line."""
    import torch
    from .deploy import load_params, W2XYZ
    from .feeder import SampleReader
    if decode not in ('host', 'device'):
        raise ValueError("decode must be 'host' or 'device', not %r" % (decode,))
    from .frames import check_entropy
    check_entropy(None, decode, entropy)                     # ('split' belongs to the device decoder)
    rank, world = init_process_group()
    if torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)) % torch.cuda.device_count())
    params = params or load_params(model_dir)
    w2 = W2XYZ(model_dir, params=params, variables=variables)
    net = w2.model
    feed = DeviceFeed(db_dir, params, net.device, entropy=entropy) if decode == 'device' else None
    ids = [l.strip() for l in open(subset_fn)] if subset_fn else sorted(os.listdir(db_dir))
    ids = [i for i in ids if i and os.path.isdir(os.path.join(db_dir, i))]
    layouts = read_layouts(layouts_fn)
    plan = window_plan(db_dir, ids)
    lo, hi, n_batches = batch_shard(len(plan), rank, world, partial_batch)
    readers = _ReaderCache(lambda yid: SampleReader(
        os.path.join(db_dir, yid), ambi_order=params.ambi_order, audio_rate=params.audio_rate, video_rate=params.video_rate,
        context=params.context, duration=0.1, return_video=VIDEO in params.encoders, img_prep=None,      # frames stay uint8 (sagen_forward_u8)
        return_flow=FLOW in params.encoders, skip_silence_thr=None, shuffle=False, random_rotations=False,
        skip_rate=SKIP_RATE))                                              # feeder.py:373-396 (for_eval)
    ev = Evaluator(net, params, power_maps=power_maps, all_metrics=all_metrics)
    keys = ALL_METRIC_KEYS if all_metrics else METRIC_KEYS
    # groups > 1 (round 6): `groups` consecutive FULL batches of the rank's shard per forward call (W2XYZ._grouped_model: the same
    # device variables, grouped native contexts) - per-sample rows unchanged; a zero-padded partial batch and the shard's tail run singly
    w2.groups = max(1, int(groups))
    gnet = w2._grouped_model(w2.groups) if w2.groups > 1 else None
    pending = []
    masks_of = lambda wins: np.stack([layouts.get(yid, np.ones(4)) for yid, _ in wins], 0)

    def host_item(wins):
        samples = [readers.get(yid).sample_at(t) for yid, t in wins]
        def stack(k):
            if k not in samples[0]:
                return None
            x = np.stack([smp[k] for smp in samples], 0)
            return x if (k == 'video' and x.dtype == np.uint8) else x.astype(np.float32)
        return ([smp['id'] for smp in samples], stack('ambix'), stack('video'), stack('flow'), masks_of(wins))

    def run_single(item):
        if feed is None:
            return ev.run_batch(*item)
        ids_, mono, target, video, flow = feed.call(item, BATCH_SIZE)             # (an item of the device feed is its windows)
        ev.run_views(ids_, mono, target, video, flow, masks_of(item))

    def run_group(items):
        if feed is None:
            return ev.run_batches(items, gnet)
        wins = [w for q in items for w in q]
        ids_, mono, target, video, flow = feed.call(wins, len(wins))
        ev.run_views(ids_, mono, target, video, flow, masks_of(wins), net=gnet)

    def flush(force_single=False):
        if pending and (force_single or len(pending) < w2.groups):
            for q in pending:
                run_single(q)
        elif pending:
            run_group(pending)
        del pending[:]
    for b in range(lo, hi):
        wins = plan[b * BATCH_SIZE:(b + 1) * BATCH_SIZE]
        item = host_item(wins) if feed is None else wins
        full = len(wins) == BATCH_SIZE and (feed is not None or item[2] is None or item[2].dtype == np.uint8)
        if gnet is None or not full:
            flush(force_single=True)
            run_single(item)
            continue
        pending.append(item)
        if len(pending) == w2.groups:
            flush()
    flush(force_single=True)

    # global means (np.mean over every sample, eval.py:223): ONE all-reduce of per-key sums (+ finite-only sums / counts) + sample count
    red = MetricReducer(keys, device=net.device if world > 1 and torch.cuda.is_available() and
                        torch.distributed.get_backend() != 'gloo' else None)
    rows = np.asarray(ev.rows, np.float64).reshape(-1, len(keys))
    red.add_rows(rows)
    means, count = red.reduce()
    # per-sample rows to rank 0 (eval.py:210-215 file format); ranks hold consecutive batch ranges, so rank order = global order
    all_ids, all_rows = [ev.ids], [rows]
    if world > 1:
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, (ev.ids, rows))
        all_ids, all_rows = [g[0] for g in gathered], [g[1] for g in gathered]
    if rank == 0:
        eval_fn = os.path.join(model_dir, 'eval-detailed.txt')
        assert overwrite or not os.path.exists(eval_fn), 'Evaluation file already exists.'
        with open(eval_fn, 'w') as f:
            f.write('SampleID | {}\n'.format(' '.join(keys)))
            for ids_r, rows_r in zip(all_ids, all_rows):
                for sid, row in zip(ids_r, rows_r):
                    f.write('{} | {}\n'.format(sid, ' '.join(str(v) for v in row)))
        short = {k: c for k, c in red.finite_counts.items() if c < count}
        if short:        # the means above are np.mean over all samples (eval.py:223): a non-finite sample shows there; say how many
            print('EVAL | non-finite per-sample values: ' + ', '.join('%s %d/%d finite (finite-only mean %.6g)' % (k, c, count, red.finite_means[k])
                                                                     for k, c in sorted(short.items())))
        ev_sat = getattr(net, 'saturation_events', [])
        if ev_sat:
            print('EVAL | fp16x2 guard: %d batches clamped activation-plane elements (%d in all) and were re-run on bf16 planes'
                  % (len(ev_sat), sum(c for _, c in ev_sat)))
        dropped = len(plan) - count
        if dropped:
            print('EVAL | %d trailing windows (a partial batch of %d) were not evaluated' % (dropped, BATCH_SIZE))
    evaluate.last_maps = ev.maps
    return OrderedDict((k, means[k]) for k in keys), count


def arg_parser():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('model_dir')
    ap.add_argument('db_dir', help='directory of preprocessed clip folders (params.db_dir in the reference)')
    ap.add_argument('--subset_fn', default=None)
    ap.add_argument('--layouts_fn', default='meta/audio_layouts.txt')
    ap.add_argument('--overwrite', action='store_true')
    ap.add_argument('--groups', type=int, default=1,
                    help='batches of 16 windows per forward call (grouped launch: one launch per layer for all of them, own batch-norm statistics per batch; rows unchanged)')
    ap.add_argument('--partial_batch', choices=['drop', 'pad'], default='drop',
                    help="trailing windows that do not fill a batch of 16: 'drop' (the reference's queue never dequeues them) or 'pad' with zero windows")
    ap.add_argument('--power_maps', action='store_true',
                    help='also compute the per-sample directional RMS maps of prediction and ground truth on the device (the inputs of the '
                         "reference's EMD metric, eval.py:188-191) and save this rank's maps to <model_dir>/eval-powermaps-rank<r>.npz")
    ap.add_argument('--all_metrics', action='store_true',
                    help="write all 28 columns of the reference's eval.py (ALL_METRIC_KEYS): adds mel_lsd, env_mse and emd/dir, emd/dir2, "
                         'computed on the device')
    ap.add_argument('--decode', choices=['host', 'device'], default='host',
                    help="where the windows and frames of a batch are made: 'host' (numpy windows, PIL frames, one upload per batch) or 'device' "
                         "(the clips' wav pieces stay on the device and sagen_assemble_audio cuts input and target there; the frame files' bytes go "
                         'up and jpeg.py decodes them); the same rows, line for line.  A decode call costs the same whatever it holds: measured, device is slower than '
                         'host below --groups 4 and faster from there on (README)')
    from .frames import ENTROPY_HELP
    ap.add_argument('--entropy', choices=['lane', 'split'], default='lane', help=ENTROPY_HELP)
    return ap


def main(argv=None):
    args = arg_parser().parse_args(argv)
    from .deploy import load_params, require_first_order
    from .frames import check_entropy
    check_entropy('evaluate', args.decode, args.entropy)
    require_first_order(load_params(args.model_dir).ambi_order, 'evaluate')
    means, count = evaluate(args.model_dir, args.db_dir, args.subset_fn, args.layouts_fn, overwrite=args.overwrite,
                            partial_batch=args.partial_batch, power_maps=args.power_maps, groups=args.groups,
                            all_metrics=args.all_metrics, decode=args.decode, entropy=args.entropy)
    if args.power_maps and evaluate.last_maps:
        maps = evaluate.last_maps                      # [pred, gt, pred, gt, ...] per batch, each [n, 7, 12]
        np.savez(os.path.join(args.model_dir, 'eval-powermaps-rank%d.npz' % int(os.environ.get('RANK', 0))),
                 pred=np.concatenate(maps[0::2], 0), gt=np.concatenate(maps[1::2], 0))
    if int(os.environ.get('RANK', 0)) == 0:
        print('EVAL | %d samples' % count)
        for k, v in means.items():
            print('EVAL | \t %s %f' % (k, v))


if __name__ == '__main__':
    main()
