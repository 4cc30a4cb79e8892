"""frames.py on the host (no library, no device): the output folder's rules under each tool's arguments, the folder listing, the size
check, the writer's refusals and its PIL path, and ops.encode_with_retry - the encode / fetch / retry-at-the-bound protocol of
JpegEncoder, PngEncoder and transcode_files - driven by a fake encoder on CPU tensors that records its calls."""
import io
import os

import numpy as np
import pytest

from spatialaudiogen_amd import frames as F

# (tool, keyword arguments) as overlay.main, deploy.main, project.main and flow.main call prepare_output_dir
RULES = {'overlay': {}, 'deploy': {}, 'project': dict(extensions=('.png', '.jpg')),
         'flow': dict(extensions=('.png', '.jpg'), extras=('flow_limits.npy',), refuse_any=True)}


def _fill(folder, names):
    os.makedirs(folder, exist_ok=True)
    for n in names:
        with open(os.path.join(folder, n), 'wb') as f:
            f.write(b'x')


@pytest.mark.parametrize('tool', sorted(RULES))
def test_prepare_output_dir_makes_a_missing_folder_and_takes_an_empty_one(tmp_path, tool):
    out = str(tmp_path / 'a' / 'out')
    F.prepare_output_dir(out, False, tool, **RULES[tool])
    assert os.listdir(out) == []
    F.prepare_output_dir(out, False, tool, **RULES[tool])
    assert os.listdir(out) == []


def test_prepare_output_dir_rules_of_each_tool(tmp_path):
    held = ['000000.png', '000001.jpg', 'flow_limits.npy', 'notes.txt']
    # tool -> (what it refuses on, alone in the folder; what --overwrite removes of `held`)
    refuses = {'overlay': ['000000.png'], 'deploy': ['000000.png'], 'project': ['000000.png', '000001.jpg'],
               'flow': ['000000.png', '000001.jpg', 'flow_limits.npy', 'notes.txt']}
    removes = {'overlay': ['000000.png'], 'deploy': ['000000.png'], 'project': ['000000.png', '000001.jpg'],
               'flow': ['000000.png', '000001.jpg', 'flow_limits.npy']}
    for tool in sorted(RULES):
        for name in held:
            out = str(tmp_path / tool / name)
            _fill(out, [name])
            if name in refuses[tool]:
                with pytest.raises(SystemExit) as e:
                    F.prepare_output_dir(out, False, tool, **RULES[tool])
                want = '%s: %s is not empty (--overwrite)' if tool == 'flow' else '%s: %s already holds frames (--overwrite)'
                assert str(e.value) == want % (tool, out)
            else:
                F.prepare_output_dir(out, False, tool, **RULES[tool])
            assert os.listdir(out) == [name]                             # refused or not: nothing is removed without --overwrite
        out = str(tmp_path / tool / 'all')
        _fill(out, held)
        F.prepare_output_dir(out, True, tool, **RULES[tool])
        assert sorted(os.listdir(out)) == sorted(set(held) - set(removes[tool]))
    # the stray file that project and overlay leave alone is what flow refuses on
    assert 'notes.txt' not in refuses['project'] + refuses['overlay'] and 'notes.txt' in refuses['flow']


def _jpg(path, h, w, value=0):
    from PIL import Image
    Image.fromarray(np.full((h, w, 3), value, np.uint8)).save(path)


def test_frame_names_stop_at_the_first_gap(tmp_path):
    folder = str(tmp_path)
    assert F.frame_names(folder) == []
    for k in (0, 1, 3):
        _jpg(os.path.join(folder, '%06d.jpg' % k), 8, 8)
    _jpg(os.path.join(folder, 'other.jpg'), 8, 8)
    assert F.frame_names(folder) == [os.path.join(folder, '%06d.jpg' % k) for k in (0, 1)]


def test_check_frame_sizes_and_frame_size(tmp_path):
    names = [str(tmp_path / ('%06d.jpg' % k)) for k in range(3)]
    _jpg(names[0], 24, 48)
    _jpg(names[1], 24, 48, 90)
    F.check_frame_sizes(names[:2], 'flow')
    assert F.frame_size(names[0]) == (48, 24)
    assert F.load_frames(names[:2]).shape == (2, 24, 48, 3)
    _jpg(names[2], 16, 24)
    with pytest.raises(SystemExit) as e:
        F.check_frame_sizes(names, 'project')
    assert str(e.value) == 'project: %s is 24x16, the first frame 48x24 (all frames must have one size)' % names[2]


def test_frame_writer_refusals(tmp_path):
    out = str(tmp_path / 'never_made')
    text = 'restart_rows takes 0 or a positive number of MCU rows and belongs to jpg (restart_rows=%d fmt=%s)'
    for fmt, rows in (('png', 1), ('jpg', -1), ('png', -2)):
        for encode in ('host', 'device'):
            with pytest.raises(ValueError) as e:
                F.FrameWriter(out, fmt, encode, restart_rows=rows)
            assert str(e.value) == text % (rows, fmt)
    for fmt, rows in (('png', 0), ('jpg', 0), ('jpg', 2)):
        assert F.FrameWriter(out, fmt, 'host', restart_rows=rows).encoder is None
    assert not os.path.exists(out)


@pytest.mark.parametrize('rows', [0, 1])
def test_host_writer_round_trip(tmp_path, rows):
    import torch
    from PIL import Image
    frames = np.random.RandomState(3).randint(0, 256, (3, 24, 48, 3)).astype(np.uint8)
    out = str(tmp_path)
    F.FrameWriter(out, 'jpg', restart_rows=rows).write(torch.as_tensor(frames), 4)
    if not rows:
        F.FrameWriter(out, 'png').write(torch.as_tensor(frames[:2]), 1)
        F.FrameWriter(out, 'png').write(torch.as_tensor(frames[2:]), 3)
    assert sorted(os.listdir(out)) == sorted(['%06d.jpg' % k for k in (4, 5, 6)] + ([] if rows else ['%06d.png' % k for k in (1, 2, 3)]))
    for k in range(3):
        want = io.BytesIO()
        Image.fromarray(frames[k]).save(want, 'JPEG', quality=95, **(dict(restart_marker_rows=1) if rows else {}))
        with open(os.path.join(out, '%06d.jpg' % (4 + k)), 'rb') as f:
            got = f.read()
        assert got == want.getvalue() and (b'\xff\xdd\x00\x04' in got) == bool(rows), k
        if not rows:
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, '%06d.png' % (1 + k)))), frames[k]), k
    F.FrameWriter(out, 'png', 'device').write_files([b'abc', b'de'], 7)
    assert open(os.path.join(out, '000008.png'), 'rb').read() == b'de'


# ---- encode, fetch, retry at the bound ----------------------------------------------------------------------------------------------
CAPACITY, FATAL = 1, 2
LABEL = lambda k: 'frame %d' % (10 + k)       # as the encoders name a frame: offset by `first`


class FakeEncoder(object):
    """run(part, stride) as the encoders' device calls answer: the head of each stream that fits, its full size, the capacity bit where
    it does not fit, and whatever `extra` adds to an item's status."""

    def __init__(self, streams, extra=None, always_full=False):
        self.streams, self.extra, self.always_full, self.calls = streams, extra or {}, always_full, []

    def __call__(self, part, stride):
        import torch
        self.calls.append((part.start, part.stop, stride))
        items = list(range(len(self.streams)))[part]
        out = torch.full((len(items), stride), 0xAA, dtype=torch.uint8)
        sizes, status = torch.zeros(len(items), dtype=torch.int32), torch.zeros(len(items), dtype=torch.int32)
        for j, k in enumerate(items):
            s = self.streams[k]
            out[j, :min(len(s), stride)] = torch.as_tensor(np.frombuffer(s[:stride], np.uint8).copy())
            sizes[j] = len(s)
            status[j] = (CAPACITY if len(s) > stride or self.always_full else 0) | self.extra.get(k, 0)
        return out, sizes, status


def _streams():
    rng = np.random.RandomState(5)
    return [rng.randint(0, 256, n).astype(np.uint8).tobytes() for n in (3, 40, 16, 0, 33)]


def _wrap(stream, k):
    return b'<%d ' % k + stream + b'>'


def test_retry_runs_the_block_once_and_each_item_that_did_not_fit_at_the_bound():
    from spatialaudiogen_amd import ops
    streams = _streams()
    fake = FakeEncoder(streams)
    files = ops.encode_with_retry(fake, 5, 16, 64, CAPACITY, _wrap, label=LABEL)
    assert fake.calls == [(0, 5, 16), (1, 2, 64), (4, 5, 64)]
    assert files == [_wrap(s, k) for k, s in enumerate(streams)]
    fake = FakeEncoder(streams)                                          # nothing to retry: one call
    assert ops.encode_with_retry(fake, 5, 64, 64, CAPACITY, _wrap) == files and fake.calls == [(0, 5, 64)]
    fake = FakeEncoder([b'', b''])                                       # nothing to fetch
    assert ops.encode_with_retry(fake, 2, 16, 64, CAPACITY, _wrap) == [b'<0 >', b'<1 >'] and fake.calls == [(0, 2, 16)]


def test_a_fatal_status_raises_before_anything_is_fetched(monkeypatch):
    from spatialaudiogen_amd import ops
    fetched = []
    real = ops.fetch_rows
    monkeypatch.setattr(ops, 'fetch_rows', lambda out, longest: fetched.append(longest) or real(out, longest))
    fake = FakeEncoder(_streams(), extra={3: FATAL, 4: FATAL})
    with pytest.raises(ValueError) as e:
        ops.encode_with_retry(fake, 5, 16, 64, CAPACITY, _wrap, fatal=FATAL, fatal_error=lambda k, st: ValueError('frame %d: status %d' % (10 + k, st)),
                              label=LABEL)
    assert str(e.value) == 'frame 13: status 2' and fetched == [] and fake.calls == [(0, 5, 16)]
    fake = FakeEncoder(_streams())                                       # (and the fetches are seen when there are some)
    ops.encode_with_retry(fake, 5, 16, 64, CAPACITY, _wrap, fatal=FATAL, fatal_error=None)
    assert fetched == [16, 40, 33]


def test_a_status_that_persists_at_the_bound_is_an_error():
    from spatialaudiogen_amd import ops
    fake = FakeEncoder(_streams(), always_full=True)
    with pytest.raises(RuntimeError) as e:
        ops.encode_with_retry(fake, 5, 16, 64, CAPACITY, _wrap, label=LABEL)
    assert str(e.value) == 'frame 10: status 1 at the stride that cannot be too small' and fake.calls == [(0, 5, 16), (0, 1, 64)]
