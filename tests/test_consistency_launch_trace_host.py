"""The launch trace of data-consistent sampling, across trees: which device launches every consistency mode issues -- in
``VolumeInference`` (joint, blend and crop), ``Imagen.sample`` and ``ElucidatedImagen.sample(sampler='dpmpp2m')`` -- in which order, with
which scalars, on which buffers and with which draws.  The other host tests of the family compare two traces of ONE tree (a keyword
absent against ``None``, a profile against the uniform one, a dispatch row by row against its restatement); this one compares the tree
with the one before it, which is what a change that moves the Python above the kernels has to be held to.

The recorder is tests/launch_trace.py, the stubs are those of tests/test_volume_launch_trace_host.py (the 40 x 36 x 44 volume, 16^3
windows, three-step denoisers, two samples, self-conditioning on) and tests/test_edm_sampler_trace_host.py; ``Imagen`` is the
two-U-Net stub of tests/test_volume_joint_host.py at four steps.  ``ops`` is replaced in ``inference``, ``imagen_pytorch3D`` and
``elucidated_imagen``, as in every other host test: the samplers hand the consistency plan the ``ops`` they launch through.  The
digest covers device launches only: the host-only helpers (``HOST_ONLY``: the union of the ``HOST_ONLY`` tuples of the profile, noise,
tile and tile-noise host tests, the slab's helpers and the replication) are answered by the real functions and leave no record and
no buffer tag, since which module calls them, and when, is free.  Everything else is recorded as in those modules: launches with
their bound arguments, buffers by storage tag and offset, draw numbers, ``sample`` / ``x0`` / ``finish`` / ``state_space`` calls, and the keyword dict a sampler call of
the blend and crop modes receives (an operator object by type, cell, rows and a digest of its table).

tests/golden/consistency_launch_trace.json holds, per case, the count per op name and the SHA-256 of the canonical JSON of the trace
(``min_value`` records removed, as in the volume module).  It was recorded from commit 8550115 -- the last one with the admission
rules written out in five preambles and the step ladder in three loops -- with this file's ``__main__``
(``python -m tests.test_consistency_launch_trace_host DIR GOLDEN``) before any source was edited, and is the behaviour the move to one
consistency plan had to keep: it is not to be regenerated from later code.  A digest that differs means launches, arguments, order,
buffers or draws changed; set ``DIQT_LAUNCH_TRACE_DUMP=<dir>`` to write the full traces there (a mismatch writes them to a temporary
directory by itself) and diff them against a dump of the older tree."""
import collections
import hashlib
import json
import os

import pytest
import torch

from tests import launch_trace as LT
from tests import test_edm_sampler_trace_host as E
from tests import test_volume_launch_trace_host as V
from tests import volume_joint_tile_noise_reference as TN
from tests import volume_joint_tile_reference as TR
from tests.test_volume_joint_host import _imagen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'consistency_launch_trace.json')

HOST_ONLY = ('consistency_cell', 'cell_profile', 'cell_norm', 'consistency_noise_sigma', 'consistency_noise_schedule',
             'consistency_noise_dispatch', 'tile_operator', 'tile_noise_operator', 'tile_noise_plan', 'tile_noise_schedule',
             'tile_noise_tables', 'slab_profile', 'slab_plan', 'slab_lds', 'tile_noise_lds', 'cell_replicate')
JOINT = ('volume_joint_consistent_step', 'volume_joint_consistent_profile_step', 'volume_joint_consistent_tile_step',
         'volume_joint_consistent_noise_step', 'volume_joint_consistent_tile_noise_step', 'volume_joint_consistent_slab_step')
PROJECT = ('cell_project', 'cell_project_profile', 'tile_project', 'slab_project')
PROJECT_NOISE = ('cell_project_noise', 'tile_project_noise')


class Ops(LT.RecordingOps):
    """``launch_trace.RecordingOps`` whose host-only helpers are the real functions, unrecorded."""

    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self._real, name)
        return super().__getattr__(name)


def _describe_operator(v):
    out = {'operator': type(v).__name__, 'cell': list(v.cell), 'm': int(v.m),
           'table': hashlib.sha256(v.table.contiguous().numpy().tobytes()).hexdigest()[:16]}
    if hasattr(v, 'row_noise'):
        out['row_noise'] = [LT.f32(s) for s in v.row_noise.tolist()]
    return out


class Recorder(LT.Recorder):
    def describe(self, v, role):
        from diffusioniqt_amd import ops
        return _describe_operator(v) if isinstance(v, ops.TileOperator) else super().describe(v, role)


class EDMRecorder(E.EDMRecorder):
    def describe(self, v, role):
        from diffusioniqt_amd import ops
        return _describe_operator(v) if isinstance(v, ops.TileOperator) else super().describe(v, role)


_into = lambda key: (lambda a: a['out'] if a.get('out') is not None else torch.zeros_like(a[key]))
_both = lambda a: (a['out'] if a['out'] is not None else torch.zeros_like(a['x0']),
                   a['out_noise'] if a['out_noise'] is not None else torch.zeros_like(a['noise']))
PROJECTIONS = {**{name: _into('x0') for name in PROJECT}, **{name: _both for name in PROJECT_NOISE}}

# ---- the modes --------------------------------------------------------------------------------------------------------------------------------
# VolumeInference: cell (2, 2, 2) on the 40 x 36 x 44 volume, raw units (mean 300, std 200; the stub's state_space has slope 2)
A222 = TR.stack_matrix((2, 2, 2), (0, 1, 2))
SIG222 = [100 * s for s in TN.stack_sigma((2, 2, 2), (0, 1, 2), (0.05, 0.2, 0.1)).tolist()]
PZ4 = [0.25, 1.0, 1.0, 0.25]
VOLUME_MODES = {
    'cell': lambda: dict(consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2))),
    'profile': lambda: dict(consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)), consistency_profile=((1, 2), (1, 1), (3, 1))),
    'operator': lambda: dict(consistency=(torch.full((12, 20, 18, 22), 300.0), (2, 2, 2)), consistency_operator=A222),
    'slab': lambda: dict(consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)), consistency_slab=(PZ4, [1.0, 0.5], [0.75, 1.0])),
}
VOLUME_NOISE_MODES = {
    'noise-large': lambda: dict(VOLUME_MODES['cell'](), consistency_noise=40.0),
    'noise-tiny': lambda: dict(VOLUME_MODES['cell'](), consistency_noise=1e-9),
    'rownoise-large': lambda: dict(VOLUME_MODES['operator'](), consistency_row_noise=SIG222),
    'rownoise-tiny': lambda: dict(VOLUME_MODES['operator'](), consistency_row_noise=1e-9),
}
# the one-call samplers: cell (2, 2, 4) on 16^3 cubes, state units
A224 = TR.stack_matrix((2, 2, 4), (0, 2))
SIG224 = TN.stack_sigma((2, 2, 4), (0, 2), (0.2, 0.6)).tolist()
SAMPLER_MODES = {
    'cell': {},
    'profile': dict(consistency_profile=((1, 2), (1, 1), (1, 3, 3, 0))),
    'operator': dict(consistency_operator=A224),
    'slab': dict(consistency_slab=(PZ4, [1.0, 1.0], [1.0, 2.0, 2.0, 1.0])),
}
SAMPLER_NOISE_MODES = {
    'noise-large': dict(consistency_noise=0.2),
    'noise-tiny': dict(consistency_noise=1e-12),
    'rownoise-large': dict(consistency_operator=A224, consistency_row_noise=SIG224),
    'rownoise-tiny': dict(consistency_operator=A224, consistency_row_noise=1e-12),
}


# ---- VolumeInference ----------------------------------------------------------------------------------------------------------------------------
VOLUME_RETURNS = {
    **V.RETURNS,
    'tile_backproject': lambda a: torch.full((40, 36, 44), 300.0),
    'slab_workspace': lambda a: (LT.zeros((2 * 40 + 20) * 18 * 22), LT.zeros(20, 18, 22)),
    'volume_joint_slab_coeffs': lambda a: a['coef'],
    **{name: (lambda a: (a['out'], a['x0_out'])) for name in JOINT},
}


def keyword_sampler(rec):
    """``sample_fn`` of the crop and blend modes: records every keyword it is handed, and asks an anchored source for two draws."""
    def sample(x, noise=None, **kw):
        if noise is not None:
            noise(x.shape), noise(x.shape)
        return rec.record('sample', {'x': x, 'noise': noise, **dict(sorted(kw.items()))}, torch.zeros_like(x))
    return sample


def volume_case(base, mode, fn=None):
    def run():
        from diffusioniqt_amd import inference
        rec, case, kw = Recorder(), V.CASES[base], mode()
        vol = torch.from_numpy(case['vol']())
        rec.tag(vol, 'vol'), rec.tag(kw['consistency'][0], 'meas')
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(V.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, 2 * x - 1), raising=False)
            mp.setattr(inference, 'ops', Ops(rec, VOLUME_RETURNS))
            out = inference.VolumeInference(case['cfg'], (fn or case['fn'])(rec), **{**case['kw'], 'consistency_weight': 0.5, **kw})(
                vol, **case['call'])
        rec.record('return', {}, out)
        return rec.trace
    return run


# ---- Imagen.sample ---------------------------------------------------------------------------------------------------------------------------------
IMAGEN_RETURNS = {'axpby3': lambda a: torch.zeros_like(a['a']), 'ddpm_step': lambda a: (torch.zeros_like(a['x_t']), torch.zeros_like(a['x_t'])),
                  **PROJECTIONS}


def imagen_case(sampler, eta, mode):
    def run():
        from diffusioniqt_amd import imagen_pytorch3D
        rec, imagen = Recorder(), _imagen()
        lr, meas = torch.zeros(2, 1, 16, 16, 16), torch.full((2, 1, 16, 16, 16), 0.125)
        rec.tag(lr, 'lowres'), rec.tag(meas, 'meas_up')
        noise = [LT.zeros(2, 1, 16, 16, 16) for _ in range(8)]
        for k, t in enumerate(noise):
            rec.tag(t, f'noise{k}')
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(imagen_pytorch3D, 'ops', Ops(rec, IMAGEN_RETURNS))
            out = imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, device='cpu', sampler=sampler,
                                sample_steps=4, eta=eta, noise=noise, consistency=(meas, (2, 2, 4)), consistency_weight=0.75, **mode)[0]
        rec.record('return', {}, out)
        return rec.trace
    return run


# ---- ElucidatedImagen.sample ---------------------------------------------------------------------------------------------------------------------------
def edm_case(eta, mode):
    def run():
        from diffusioniqt_amd import elucidated_imagen
        rec = EDMRecorder()
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(elucidated_imagen, 'ops', Ops(rec, {**E.RETURNS, **PROJECTIONS}))
            out = E.sample_case(dict(self_cond=True), sampler='dpmpp2m', eta=eta, consistency=0.75, **mode)(rec)
        rec.record('return', {}, out)
        return rec.trace
    return run


IMAGEN_SAMPLERS = {'ddpm': ('ddpm', 0.0), 'ddim-eta0.5': ('ddim', 0.5), 'ddim-eta0': ('ddim', 0.0), 'dpmpp2m': ('dpmpp2m', 0.0)}
CASES = {
    **{f'joint-{chain}-{m}': volume_case(f'joint-{chain}-selfcond', mode)
       for chain in ('step', 'multistep', 'sigma-base1') for m, mode in VOLUME_MODES.items()},
    **{f'joint-{chain}-{m}': volume_case(f'joint-{chain}-selfcond', mode)
       for chain in ('step', 'sigma-base1') for m, mode in VOLUME_NOISE_MODES.items()},
    **{f'{base}-{m}': volume_case(f'{base}', mode, keyword_sampler)
       for base in ('blend-gaussian-s2-anchored', 'crop-s16')
       for m, mode in {**VOLUME_MODES, 'noise': VOLUME_NOISE_MODES['noise-large'], 'rownoise': VOLUME_NOISE_MODES['rownoise-large']}.items()},
    **{f'imagen-{s}-{m}': imagen_case(*IMAGEN_SAMPLERS[s], mode) for s in IMAGEN_SAMPLERS for m, mode in SAMPLER_MODES.items()},
    **{f'imagen-{s}-{m}': imagen_case(*IMAGEN_SAMPLERS[s], mode) for s in ('ddpm', 'ddim-eta0.5') for m, mode in SAMPLER_NOISE_MODES.items()},
    **{f'edm-eta{eta}-{m}': edm_case(eta, mode) for eta in (0, 1) for m, mode in SAMPLER_MODES.items()},
    **{f'edm-eta1-{m}': edm_case(1, mode) for m, mode in SAMPLER_NOISE_MODES.items()},
}


def summary(trace):
    assert not any(r['op'] in HOST_ONLY for r in trace)
    counts = collections.Counter(r['op'] for r in trace)
    rest = [r for r in trace if r['op'] != 'min_value']
    return {'counts': dict(sorted(counts.items())), 'sha256': hashlib.sha256(LT.canonical(rest).encode()).hexdigest()}


@pytest.mark.parametrize('name', list(CASES))
def test_launch_trace_is_the_recorded_one(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(CASES)
    trace = CASES[name]()
    got = summary(trace)
    where = os.environ.get('DIQT_LAUNCH_TRACE_DUMP')
    if where or got != golden[name]:
        print(f"{name}: full trace written to {LT.dump(name, trace, where, 'consistency_launch_trace_')}")
    print(f"{name}: {len(trace)} records, {got['counts']}")
    assert got['counts'] == golden[name]['counts']
    assert got['sha256'] == golden[name]['sha256']


def test_the_cases_reach_every_launch():
    """What the matrix is for, read off the recorded counts: every one of the six joint launches and of the six projection launches
    occurs, the noise-aware modes reach their shaped, constant-weight and plain rungs, the slab takes its coefficient launches and one
    workspace per volume, and the blend and crop modes hand the measurement on in every sampler call."""
    with open(GOLDEN) as f:
        counts = {k: collections.Counter(v['counts']) for k, v in json.load(f).items()}
    for op in JOINT + PROJECT + PROJECT_NOISE:
        assert any(c[op] for c in counts.values()), op
    S, T = 2, 3                                              # the volume stubs: two samples of three steps
    for chain in ('step', 'multistep', 'sigma-base1'):
        for mode, op in zip(VOLUME_MODES, JOINT[:3] + JOINT[5:]):
            c = counts[f'joint-{chain}-{mode}']
            assert c[op] == S * T and sum(c[o] for o in JOINT) == S * T and c['state_space'] == 1
        slab = counts[f'joint-{chain}-slab']
        assert slab['volume_joint_slab_coeffs'] == S * T and slab['slab_workspace'] == 1
    plain = {'step': 'volume_joint_step', 'sigma-base1': 'volume_joint_multistep_sde'}
    for chain, first in (('step', 0), ('sigma-base1', 1)):                 # the sigma chain's first row has kn = 0: a plain launch
        for mode, shaped, constant in (('noise', JOINT[3], JOINT[0]), ('rownoise', JOINT[4], JOINT[2])):
            large, tiny = counts[f'joint-{chain}-{mode}-large'], counts[f'joint-{chain}-{mode}-tiny']
            assert large[shaped] == S * (T - first) and large[constant] == 0 and tiny[constant] == S * (T - first) and tiny[shaped] == 0
            assert large['state_space'] == tiny['state_space'] == 2    # the measurement and the slope
            # the initial state of the sigma chain is a launch of the same op
            assert large[plain[chain]] == tiny[plain[chain]] == S * first + (S if chain == 'sigma-base1' else 0)
    for base in ('blend-gaussian-s2-anchored', 'crop-s16'):
        for mode in (*VOLUME_MODES, 'noise', 'rownoise'):
            c = counts[f'{base}-{mode}']
            assert c['sample'] > 1 and c['patch_gather'] == 1 + 2 * c['sample'] // (2 if base.startswith('blend') else 1)
            assert c['tile_backproject'] == (mode in ('operator', 'rownoise'))
    steps = 4
    for s in IMAGEN_SAMPLERS:
        for mode, op in zip(SAMPLER_MODES, PROJECT):
            assert counts[f'imagen-{s}-{mode}'][op] == counts[f'imagen-{s}-{mode}']['ddpm_step'] == steps
    for s in ('ddpm', 'ddim-eta0.5'):                                      # the last step has kn = 0: unprojected
        for mode, shaped, constant in (('noise', 'cell_project_noise', 'cell_project'), ('rownoise', 'tile_project_noise', 'tile_project')):
            large, tiny = counts[f'imagen-{s}-{mode}-large'], counts[f'imagen-{s}-{mode}-tiny']
            assert large[shaped] == tiny[constant] == steps - 1 and large[constant] == tiny[shaped] == 0
            assert large['ddpm_step'] == tiny['ddpm_step'] == steps
    for eta in (0, 1):
        for mode, op in zip(SAMPLER_MODES, PROJECT):
            c = counts[f'edm-eta{eta}-{mode}']
            assert c[op] == c['multistep_sde_step'] == c['unet'] > 1
    for mode, shaped, constant in (('noise', 'cell_project_noise', 'cell_project'), ('rownoise', 'tile_project_noise', 'tile_project')):
        large, tiny = counts[f'edm-eta1-{mode}-large'], counts[f'edm-eta1-{mode}-tiny']
        assert large[shaped] == tiny[constant] == large['multistep_sde_step'] - 1 and large[constant] == tiny[shaped] == 0


if __name__ == '__main__':              # python -m tests.test_consistency_launch_trace_host DIR [GOLDEN]: dump every full trace, print every
    import sys                          # summary and, given a second path, write the summaries there as a golden file
    summaries = {}
    for case in CASES:
        t = CASES[case]()
        summaries[case] = summary(t)
        print(case, len(t), LT.dump(case, t, sys.argv[1]), json.dumps(summaries[case]['counts'], sort_keys=True))
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            json.dump(summaries, f, indent=1, sort_keys=True)
            f.write('\n')
