"""The degenerate inputs real clips open and close with - silence, constant frames, a still camera, one frame repeated - defined once
for tests/test_degenerate_host.py (the two CPU references on them, no GPU) and tests/test_gpu_degenerate.py (the HIP path on them).

Every case starts from weights.synth_inputs(B, encoders, SEED) and replaces parts of it.  Frames are handed over as the uint8 a decoder
produces; their float form is u8 / 255 - 0.5 (myutils.py:88-89), which `frames_float` computes exactly as the feeder does.

The bar of a compared tensor is   max(the project's bar for it, FACTOR * e32)   where e32 is the error of the plain fp32 CPU reference
(oracle.torch_ref.TorchRef, float32) against the fp64 one on that tensor and input: the device's own error never enters its bar.
FACTOR = 4: two fp32 evaluations with different summation orders draw the same error distribution and scatter by a small factor; a lost
digit (10 x) still fails."""
import contextlib

import numpy as np

from spatialaudiogen_amd.weights import variable_specs, init_weights, synth_inputs

WEIGHT_SEED, SEED = 11, 77
FACTOR = 4.0
REF_THREADS = 16                         # intra-op threads of the CPU references (see references())
ABS_TOL, REL_TOL = 1e-4, 1e-3            # the output's bars (tests/test_gpu_model.py)
TRUNK_TOL = 1e-4                         # relative, <stream>_encoder/conv5_2 (test_audio_video)
BOTTLENECK_TOL = 2e-4                    # relative, bottleneck (test_audio_video)

A, AV, AVF = ('audio',), ('audio', 'video'), ('audio', 'video', 'flow')

# name -> (family, encoders, batch sizes).  B = 10 is deploy's batch: the black-frame error grows with B.
CASES = {
    'silent':         ('silence', A, (2, 5)),
    'silent_window':  ('silence', AV, (2, 5)),
    'quiet':          ('silence', A, (2, 5)),
    'clipped':        ('silence', A, (2, 5)),
    'black':          ('constant', AV, (2, 5, 10)),
    'white':          ('constant', AV, (2, 5)),
    'grey':           ('constant', AV, (2, 5)),
    'one_black':      ('constant', AV, (2, 5)),
    'dark_lsb':       ('constant', AV, (2, 5)),
    'repeat':         ('constant', AV, (2, 5)),
    'still':          ('still', AVF, (2, 5)),
    'one_still':      ('still', AVF, (2, 5)),
    'all':            ('all', AVF, (2, 5, 10)),
    'all_one_window': ('all', AVF, (2, 5)),
}

# families on which plain fp32 keeps the project's bar with room to spare (measured below 1e-5 absolute on the output): there the
# project's bar must hold unchanged, i.e. FACTOR * e32 may not be what decides any bar
PROJECT_BAR_HOLDS = ('silent', 'silent_window', 'quiet', 'clipped', 'repeat')

# fp32-reference output error (absolute RMS against fp64) measured on the CPU for (case, B) with WEIGHT_SEED / SEED; the host module
# holds e32 within a factor of 3 of these either way (the value depends on the torch build's summation order), so that a change of a
# reference cannot silently loosen a GPU bar.  All of them at REF_THREADS intra-op threads (see ref_threads()).
E32_MEASURED = {
    ('silent', 2): 3.48e-08, ('silent', 5): 3.54e-08, ('silent_window', 2): 3.71e-06, ('silent_window', 5): 2.09e-06,
    ('quiet', 2): 2.76e-08, ('quiet', 5): 2.77e-08, ('clipped', 2): 1.54e-07, ('clipped', 5): 1.36e-07,
    ('black', 2): 6.9e-05, ('black', 5): 0.000177, ('black', 10): 0.00079, ('white', 2): 6.45e-05,
    ('white', 5): 8.35e-05, ('grey', 2): 1.46e-05, ('grey', 5): 2.11e-05, ('one_black', 2): 4.08e-05,
    ('one_black', 5): 3.25e-05, ('dark_lsb', 2): 1.31e-05, ('dark_lsb', 5): 1.46e-05, ('repeat', 2): 1.27e-06,
    ('repeat', 5): 2.61e-06, ('still', 2): 2.81e-05, ('still', 5): 8.21e-05, ('one_still', 2): 5.79e-06,
    ('one_still', 5): 7.84e-06, ('all', 2): 0.000132, ('all', 5): 0.000185, ('all', 10): 0.000448,
    ('all_one_window', 2): 1.97e-05, ('all_one_window', 5): 2.82e-05,
}


def case_ids(host_only=False):
    """[(name, B)] of the table; the host module leaves the B = 10 cases to the GPU module"""
    return [(n, b) for n, (_, _, bs) in CASES.items() for b in bs if not (host_only and b > 5)]


_WEIGHTS, _RANDOM = {}, {}


def weights(encoders):
    """the variables every case runs with (made once per encoder set: do not write to them)"""
    encoders = tuple(encoders)
    if encoders not in _WEIGHTS:
        _WEIGHTS[encoders] = init_weights(variable_specs(list(encoders)), seed=WEIGHT_SEED, mode='test')
    return _WEIGHTS[encoders]


def frames_u8(video):
    """the uint8 frames a float32 video of synth_inputs stands for (exact: synth_inputs rounds to integers before x / 255 - 0.5)"""
    u8 = np.round((video.astype(np.float64) + 0.5) * 255.0).astype(np.uint8)
    assert np.array_equal(frames_float(u8), video)
    return u8


def frames_float(u8):
    return (u8.astype(np.float64) / 255. - 0.5).astype(np.float32)


def random_batch(B, encoders, seed=SEED):
    """{'audio', 'video' (uint8), 'flow'} of synth_inputs, the entries the encoders need"""
    key = (B, tuple(encoders), seed)
    if key not in _RANDOM:
        inp = synth_inputs(B, list(encoders), seed=seed)
        out = {'audio': inp['audio']}
        if 'video' in encoders:
            out['video'] = frames_u8(inp['video'])
        if 'flow' in encoders:
            out['flow'] = inp['flow']
        _RANDOM[key] = out
    return {k: v.copy() for k, v in _RANDOM[key].items()}


def make(name, B):
    """The inputs of one case: {'audio' float32 [B,52799,1], 'video' uint8 [B,1,224,448,3], 'flow' float32 [B,1,224,448,3]}
    (the entries its encoders need).  The window that a one-window case replaces is window 1: neither the first nor, at B = 5, the last."""
    _, enc, _ = CASES[name]
    inp = random_batch(B, enc)
    a, v, f = inp['audio'], inp.get('video'), inp.get('flow')
    k = 1
    if name == 'silent':
        a[:] = 0
    elif name == 'silent_window':
        a[k] = 0
    elif name == 'quiet':
        a *= np.float32(1e-4)
    elif name == 'clipped':
        a[:] = np.sign(a)
    elif name == 'black':
        v[:] = 0
    elif name == 'white':
        v[:] = 255
    elif name == 'grey':
        v[:] = 128
    elif name == 'one_black':
        v[k] = 0
    elif name == 'dark_lsb':
        v[:] = np.random.Generator(np.random.PCG64(SEED + 1)).integers(0, 2, size=v.shape).astype(np.uint8)
    elif name == 'repeat':
        v[:] = v[0]
    elif name == 'still':
        f[:] = 0
    elif name == 'one_still':
        f[k] = 0
    elif name == 'all':
        a[:] = 0; v[:] = 0; f[:] = 0
    elif name == 'all_one_window':
        a[k] = 0; v[k] = 0; f[k] = 0
    else:
        raise KeyError(name)
    return inp


@contextlib.contextmanager
def ref_threads():
    """e32 is a property of the fp32 reference's summation order, and torch's CPU reductions split their sums by the intra-op thread
    count: on black frames at B = 5 the float32 reference's output error is 9e-5 with 32 threads, 1.8e-4 with 16 and 5.8e-3 with one.
    The reference that defines the bars is therefore TorchRef at REF_THREADS threads, whatever the machine has."""
    import torch
    before = torch.get_num_threads()
    torch.set_num_threads(REF_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(before)


def torch_ref(P, encoders, inp, dtype):
    """(output ndarray, {intermediate name: ndarray in the device's NHWC / row layout}) of oracle.torch_ref.TorchRef in `dtype`"""
    import torch
    from oracle.torch_ref import TorchRef
    ref = TorchRef(P, list(encoders), dtype=dtype)
    v = frames_float(inp['video']) if 'video' in inp else None
    out = ref.forward(inp['audio'], v, inp.get('flow')).numpy().astype(np.float64)
    ends = {'bottleneck': ref.ends['bottleneck'].numpy().astype(np.float64),
            'localization/coeffs': ref.ends['localization/coeffs'].numpy().astype(np.float64)}
    for e in encoders[1:]:
        ends[e + '_encoder/conv5_2'] = ref.ends[e + '_encoder/conv5_2'].permute(0, 2, 3, 1).numpy().astype(np.float64)
    return out, ends


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def references(P, encoders, inp):
    """fp64 reference and the fp32 reference's errors against it:
    (out64, ends64, e32_abs of the output, {name: e32 relative RMS of that intermediate})"""
    import torch
    with ref_threads():
        out64, ends64 = torch_ref(P, encoders, inp, torch.float64)
        out32, ends32 = torch_ref(P, encoders, inp, torch.float32)
    e32_rel = {k: rms(ends32[k] - ends64[k]) / max(rms(ends64[k]), 1e-30) for k in ends64}
    return out64, ends64, rms(out32 - out64), e32_rel
