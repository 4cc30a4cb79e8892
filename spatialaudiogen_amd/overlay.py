"""Paint the sound-direction heat map over the 360-degree frames, on the device: the visual half of the reference's output stage
(myutils.gen_360video(overlay_map=True), myutils.py:246-279, over SphericalAmbisonicsVisualizer, pyutils/ambisonics/
distance.py:16-59).

    python -m spatialaudiogen_amd.overlay IN_AMBIX.wav FRAMES_DIR OUT_DIR [--angular_res 5] [--save_maps FILE.npz] [--overwrite] [--encode {host,device}]

IN_AMBIX.wav holds 4 or 9 channels (ACN / SN3D, orders 1 and 2), FRAMES_DIR the frames %06d.jpg at 10 per second; OUT_DIR receives
%06d.png.  What is computed (include/sagen.h: sagen_power_map_windows, sagen_overlay_blend; csrc/overlay.hip):

    d = ambix[::5]; one RMS map per 4800 samples of d (0.5 s) on the 5-degree mesh (37 x 72 nodes), 'projection' decoding, flipped
    upside down: the top row is +90 degrees elevation, the left column +175 degrees azimuth
    n = (map - map.min()) / (map.max() - map.min() + 0.005)                       per map
    for each consecutive pair (prev, cur) and i = 0..4:   v = (1 - i/5) n_prev + (i/5) n_cur;  v = max(v 2 - 0.7, 0)
        colour = YlOrRd256[min(int(v 255), 255)];  dir = resize(colour, (H, W)) 255;  alpha = resize(v, (H, W)) 0.6
        frame 5 (index of prev) + i  <-  uint8(alpha dir + (1 - alpha) frame)

Two quirks of the reference are kept: the first map is only ever `prev` (nothing is blended with beta < 0 before it), and
5 (n_maps - 1) frames are written - the frames of the last half second, and any frame past the audio, are not.
"""
import numpy as np

from . import ambisonics

# ColorBrewer YlOrRd, 9 classes (colorbrewer2.org; the anchors matplotlib's 'YlOrRd' colormap interpolates)
YLORRD9 = ((255, 255, 204), (255, 237, 160), (254, 217, 118), (254, 178, 76), (253, 141, 60), (252, 78, 42), (227, 26, 28), (189, 0, 38),
           (128, 0, 38))


def ylorrd_table():
    """[256, 3] float64 = plt.cm.YlOrRd(np.linspace(0, 1, 256))[:, :3] (myutils.py:253) without matplotlib: a
    LinearSegmentedColormap of N = 256 entries samples the piecewise-linear curve through the nine anchors (at k / 8) at
    linspace(0, 1, 256), and looking it up at linspace(0, 1, 256) returns the entries in order."""
    anchors = np.asarray(YLORRD9, np.float64) / 255.
    x = np.linspace(0., 1., 256)
    return np.stack([np.interp(x, np.linspace(0., 1., 9), anchors[:, k]) for k in range(3)], 1)


def overlay_sh(order, angular_res=5.0):
    """[P, C] harmonics of spherical_mesh(angular_res) with the elevation rows REVERSED, so that a map computed with them is
    np.flipud(rms) (distance.py:52) already - the image: row 0 is +90 degrees elevation."""
    phi, nu = ambisonics.spherical_mesh(angular_res)
    phi, nu = phi[::-1], nu[::-1]
    return ambisonics.sh_matrix_at(phi.reshape(-1), nu.reshape(-1), order)


def emitted_frames(n_rows, n_frames, audio_rate=48000, video_rate=10, decimate=5, frames_per_map=5):
    """(n_maps, frames written) for a stream of n_rows audio rows and n_frames frames (myutils.py:252-266, distance.py:29-30)."""
    window = int(frames_per_map / float(video_rate) * (audio_rate / float(decimate)))
    n_maps = (-(-int(n_rows) // decimate)) // window
    return n_maps, max(0, min(int(n_frames), frames_per_map * (n_maps - 1)))


class Overlay(object):
    """A stream overlay: process(ambi_rows [n, C] float32, frames [k, H, W, 3] uint8) -> the finished uint8 frames, all on the
    device.  Each argument is the next piece of its stream, of any length (None or empty: nothing new).  Between calls it keeps,
    on the device, the audio rows that do not fill a map window yet, the raw maps, and the frames whose `cur` map does not
    exist yet; it returns every frame that can be finished, in order, so the concatenation of its outputs does not depend on how
    the streams were cut (a map depends on its own window, a frame on its own two maps).

    As in the reference the first map is only ever `prev`, and no more than frames_per_map (n_maps - 1) frames are ever
    returned: frames past that stay pending."""

    def __init__(self, channels, audio_rate=48000, video_rate=10, angular_res=5.0, decimate=5, frames_per_map=5, device=None):
        if channels not in (4, 9):
            raise ValueError('%d channels is not first- or second-order ambisonics (4 or 9)' % channels)
        import torch
        from . import ops
        self.device = ops.default_device(device)
        self.channels, self.decimate, self.frames_per_map = int(channels), int(decimate), int(frames_per_map)
        # SphericalAmbisonicsVisualizer(ambix[::5], rate / 5., 5. / fps, 5.): window_frames = int(window * rate) (distance.py:29)
        self.window = int(frames_per_map / float(video_rate) * (audio_rate / float(decimate)))
        if self.window < 1 or self.decimate < 1 or self.frames_per_map < 1:
            raise ValueError('Overlay: the map window is empty')
        self.map_shape = ambisonics.mesh_shape(angular_res)
        order = {4: 1, 9: 2}[self.channels]
        self.sh = torch.as_tensor(overlay_sh(order, angular_res).astype(np.float32)).contiguous().to(self.device)
        self.lut = torch.as_tensor(ylorrd_table()).contiguous().to(self.device)
        self.reset()

    def reset(self):
        self._audio = None          # rows from a window boundary on (fewer than one window's worth)
        self._skip = 0              # rows of the NEXT pieces that belong to the stride step of a finished window
        self._maps = []             # raw maps [k, mh, mw], in order
        self._n_maps = 0
        self._frames = None         # frames not finished yet, from absolute index _frame0 on
        self._frame0 = 0

    def maps(self):
        """The raw maps seen so far [n, mh, mw] (image orientation), on the device."""
        import torch
        if not self._maps:
            return torch.empty((0,) + tuple(self.map_shape), dtype=torch.float32, device=self.device)
        if len(self._maps) > 1:
            self._maps = [torch.cat(self._maps, 0)]
        return self._maps[0]

    def _take_audio(self, rows):
        import torch
        from . import ops
        if rows.dim() != 2 or rows.shape[1] != self.channels or rows.dtype != torch.float32:
            raise ValueError('process() takes float32 [n, %d] ambisonic rows' % self.channels)
        if self._skip:
            drop = min(self._skip, rows.shape[0])
            rows, self._skip = rows[drop:], self._skip - drop
        if rows.shape[0] == 0:
            return
        buf = rows if self._audio is None else torch.cat([self._audio, rows], 0)
        span = self.window * self.decimate                      # rows from one window's first sample to the next window's
        n_new = (-(-buf.shape[0] // self.decimate)) // self.window
        if n_new:
            m = ops.power_map_windows(buf, self.sh, self.decimate, self.window)
            self._maps.append(m.reshape((n_new,) + tuple(self.map_shape)))
            self._n_maps += n_new
            used = n_new * span
            if used > buf.shape[0]:                             # the last window's last sample is in, the rest of its stride step is not
                self._skip, buf = used - buf.shape[0], buf[:0]
            else:
                buf = buf[used:]
        self._audio = buf.clone() if buf.shape[0] else None

    def process(self, ambi_rows=None, frames=None):
        import torch
        from . import ops
        if ambi_rows is not None and ambi_rows.shape[0]:
            self._take_audio(ambi_rows)
        if frames is not None and frames.shape[0]:
            if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
                raise ValueError('process() takes uint8 [k, H, W, 3] frames')
            if self._frames is not None and tuple(frames.shape[1:]) != tuple(self._frames.shape[1:]):
                raise ValueError('frames of %dx%d after frames of %dx%d' % (frames.shape[1], frames.shape[2], self._frames.shape[1], self._frames.shape[2]))
            self._frames = frames if self._frames is None or self._frames.shape[0] == 0 else torch.cat([self._frames, frames], 0)
        if self._frames is None:
            return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
        fpm = self.frames_per_map
        ready = min(self._frames.shape[0], fpm * (self._n_maps - 1) - self._frame0)
        if ready <= 0:
            return self._frames[:0]
        first, last = self._frame0 // fpm, (self._frame0 + ready - 1) // fpm + 1
        out = ops.overlay_blend(self.maps()[first:last + 1], first, self.lut, self._frames[:ready], self._frame0, fpm)
        self._frames = self._frames[ready:].clone()             # (keeps the frame size for the check above even when empty)
        self._frame0 += ready
        return out


# ---- command line ---------------------------------------------------------------------------------------------------------------
def parse_arguments(argv=None):
    import argparse
    from .frames import add_frame_arguments
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('input_fn', help='Input ambisonics file (ACN / SN3D, 4 or 9 channels).')
    parser.add_argument('frames_dir', help='Folder of the frames %%06d.jpg, 10 per second.')
    parser.add_argument('output_dir', help='Folder for the blended frames %%06d.png.')
    parser.add_argument('--angular_res', type=float, default=5., help='mesh step of the maps in degrees')
    parser.add_argument('--save_maps', default=None, metavar='FILE.npz', help='also write the raw maps [n, rows, columns]')
    add_frame_arguments(parser, block=50, encode_help="where the output frames are compressed: host (PIL, one thread) or device (png.py: the files' "
                                                      "bytes come back instead of the pixels; other bytes, the same pixels)")
    return parser.parse_args(argv)


def main(argv=None):
    import torch
    from . import frames as F
    from .feeder import load_wav
    args = parse_arguments(argv)
    F.check_entropy('overlay', args.decode, args.entropy)
    data, rate = load_wav(args.input_fn)
    if data.shape[1] not in (4, 9):
        raise SystemExit('overlay: %d channels is not first- or second-order ambisonics (4 or 9)' % data.shape[1])
    if args.block < 1 or not args.angular_res > 0:
        raise SystemExit('overlay: --block and --angular_res take positive values')
    names = F.frame_names(args.frames_dir)
    F.check_frame_sizes(names, 'overlay')
    F.prepare_output_dir(args.output_dir, args.overwrite, 'overlay')        # every refusal is behind us
    # only the frames that will be written are decoded, a block at a time: the host holds --block frames whatever the clip's length
    names = names[:emitted_frames(data.shape[0], len(names), audio_rate=rate)[1]]
    from . import ops
    ops.select_device(args.gpu)
    ov = Overlay(data.shape[1], audio_rate=rate, angular_res=args.angular_res)
    ov.process(torch.as_tensor(data.astype(np.float32)).to(ov.device), None)
    reader, writer = F.FrameReader(ov.device, args.decode, args.entropy), F.FrameWriter(args.output_dir, 'png', args.encode, ov.device)
    written = 0
    for i in range(0, len(names), args.block):
        out = ov.process(None, reader.read(names[i:i + args.block]))
        writer.write(out, written)
        written += out.shape[0]
    if args.save_maps:
        np.savez(args.save_maps, maps=ov.maps().cpu().numpy())
    print('wrote %d frames to %s (%d maps of %dx%d)' % (written, args.output_dir, ov.maps().shape[0], ov.map_shape[0], ov.map_shape[1]))


if __name__ == '__main__':
    main()
