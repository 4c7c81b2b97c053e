"""The launch trace of ``VolumeInference``: which ops every mode calls, in which order, with which scalars and on which buffers -- the
control flow of the crop, blend and joint paths, which has no CPU fallback and is therefore not run by any other host test.

``inference.ops``, ``inference.convertVolume2subVolume`` and ``inference.merge_sub_volumes`` are replaced by recording stand-ins:
``patch_gather`` and ``min_value`` are computed for real in CPU torch (the 5 % filter keeps real windows); every other op records its
call and returns zeros of the right shape, in-place ops the tensors they were given.  A record is the op name plus every argument
after binding to the real op's signature (so positional / keyword spelling and explicit defaults do not matter): scalars as they
are, floats rounded to fp32, float tensors as (tag, shape, dtype, storage offset) with the tag given by storage at first sight
(``vol``, ``volume_joint_init#1``, ``volume_joint_step.y#0``: in place versus fresh is visible), index tensors and host origin
arrays by value, ``slot`` / ``taps`` as a digest.  The sampler, the denoiser's ``x0`` / ``finish`` and -- through ``ops.anchored_noise``
-- every call of an ``AnchoredNoise`` source are recorded the same way, and so is what ``__call__`` returns.

tests/golden/volume_launch_trace.json holds, per case, the count per op name and the SHA-256 of the canonical JSON of the trace with
the ``min_value`` records removed (where in the order the volume minimum is launched is free; that it is launched exactly once, on
the raw volume, is asserted separately).  The golden was recorded from commit 3a43fdc, the last one before the three window setups and
four evaluation loops of inference.py became one plan and one loop, and is the behaviour that refactor had to keep: it is not to be
regenerated from later code; the ``joint-sigma-*`` cases were added from commit 51a6a1a, the last one with a chain per sampler family in
inference.py, on the same terms.  A digest that differs means launches, arguments, order or buffers changed; set
``DIQT_LAUNCH_TRACE_DUMP=<dir>`` to write the full traces there (a mismatch writes them to a temporary directory by itself) and
diff them against a dump of the older tree -- the recorder only patches module attributes, so this file runs on either."""
import collections
import hashlib
import json
import os

import pytest
import torch

from tests import volume_blend_reference as R
from tests import launch_trace
from tests.launch_trace import Recorder, canonical, dump, zeros

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'volume_launch_trace.json')
SEED = 5


def gather_cpu(vol, idx, P, mean, std, want_patches, want_nonzero):
    w = torch.stack([vol[i:i + P, j:j + P, k:k + P] for i, j, k in idx.tolist()])
    out = ((w - mean) / std)[:, None].contiguous() if want_patches else None
    nz = (w != 0).sum(dim=(1, 2, 3)).to(torch.int32) if want_nonzero else None
    return out, nz


# what each stand-in returns, from the arguments bound to the real op's signature
RETURNS = {
    'patch_gather': lambda a: gather_cpu(a['vol'], a['idx'], a['P'], a['mean'], a['std'], a['want_patches'], a['want_nonzero']),
    'min_value': lambda a: a['x'].min().reshape(1),
    'patch_scatter': lambda a: None,
    'background_reset': lambda a: None,
    'anchored_noise': lambda a: zeros(len(a['origins']), a['C'], a['P'], a['P'], a['P']),
    'volume_blend': lambda a: (zeros(*a['vol'].shape), zeros(*a['vol'].shape) if a['want_std'] else None),
    'volume_joint_init': lambda a: zeros(*a['shape']),
    'volume_joint_step': lambda a: a['out'] if a['out'] is not None else zeros(*a['x_t'].shape),
    'volume_joint_multistep': lambda a: (a['out'] if a['out'] is not None else zeros(*a['x_t'].shape),
                                         a['x0_out'] if a['x0_out'] is not None else zeros(*a['x_t'].shape)),
    'volume_joint_multistep_sde': lambda a: (zeros(*a['shape']), None) if a['x_t'] is None else (
        a['out'] if a['out'] is not None else zeros(*a['x_t'].shape), a['x0_out'] if a['x0_out'] is not None else zeros(*a['x_t'].shape)),
    'volume_joint_heun_init': lambda a: zeros(*a['shape']),
    'volume_joint_heun': lambda a: (a['xh'], a['xn'], a['x0']),
    'volume_joint_finish': lambda a: (a['mean_io'] if a['s'] else zeros(*a['x'].shape),
                                      a['m2_io'] if a['s'] else (zeros(*a['x'].shape) if a['S'] > 1 else None),
                                      zeros(*a['x'].shape) if a['want_std'] and a['s'] == a['S'] - 1 else None),
}


class RecordingOps(launch_trace.RecordingOps):
    """Stands in for ``diffusioniqt_amd.ops`` inside ``inference``: an op that is not in ``RETURNS`` is an AttributeError."""

    def __init__(self, rec):
        super().__init__(rec, RETURNS)


def sampler_of(rec):
    """``sample_fn`` of the crop and blend paths: asks an anchored source for two draws (the initial image and one step), as a
    two-call sampler would."""
    def sample(x, noise=None):
        if noise is not None:
            noise(x.shape), noise(x.shape)
        return rec.record('sample', {'x': x, 'noise': noise}, torch.zeros_like(x))
    return sample


class StubDenoiser:
    """Three steps; the first-order and multistep chains."""
    num_steps, clamp = 3, (-1.0, 1.0, 1)

    def __init__(self, rec, self_cond, multistep):
        self.rec, self.self_cond, self.multistep = rec, self_cond, multistep
        self.coefs = torch.tensor([[0.5, 0.25, 0.125], [0.75, 0.375, 0.0625], [0.875, 0.4375, 0.03125]])

    def x0(self, img, lowres, i, self_cond=None):
        return self.rec.record('x0', {'img': img, 'lowres': lowres, 'i': i, 'self_cond': self_cond}, torch.zeros_like(img))

    def finish(self, x):
        return self.rec.record('finish', {'x': x}, torch.zeros_like(x))


class StubHeunDenoiser(StubDenoiser):
    """Three Heun steps, the last one to sigma 0 (no corrector)."""
    heun, draw_base, sigma0, clamp = True, 1, 1.5, (-float('inf'), float('inf'), 1)

    def __init__(self, rec, self_cond):
        super().__init__(rec, self_cond, False)
        self.coefs = (torch.arange(21, dtype=torch.float32).reshape(3, 7) + 1) / 32
        self.sched = torch.tensor([[1.5, 0.75, 0.25], [0.75, 0.375, 0.25], [0.375, 0.0, 0.0]], dtype=torch.float64)

    def x0(self, img, lowres, i, self_cond=None, stage=0, lowres_noise=None):
        return self.rec.record('x0', {'img': img, 'lowres': lowres, 'i': i, 'self_cond': self_cond, 'stage': stage,
                                      'lowres_noise': lowres_noise}, torch.zeros_like(img))


class StubSigmaDenoiser(StubDenoiser):
    """Three steps of the EDM family's multistep chain: ODE (kn = 0) on the first, SDE on the others."""
    sigma0 = 1.5

    def __init__(self, rec, self_cond, draw_base):
        super().__init__(rec, self_cond, True)
        self.draw_base = draw_base
        self.coefs = torch.tensor([[0.5, 0.25, 0.0, 0.0], [0.75, 0.375, -0.125, 0.0625], [0.875, 0.4375, -0.25, 0.03125]])

    def x0(self, img, lowres, i, self_cond=None, lowres_noise=None):
        return self.rec.record('x0', {'img': img, 'lowres': lowres, 'i': i, 'self_cond': self_cond, 'lowres_noise': lowres_noise},
                               torch.zeros_like(img))


def _joint(chain, block, self_cond):
    stub = {'step': lambda rec: StubDenoiser(rec, self_cond, False), 'multistep': lambda rec: StubDenoiser(rec, self_cond, True),
            'heun': lambda rec: StubHeunDenoiser(rec, self_cond), 'sigma-base0': lambda rec: StubSigmaDenoiser(rec, self_cond, 0),
            'sigma-base1': lambda rec: StubSigmaDenoiser(rec, self_cond, 1)}[chain]
    if block:
        return dict(vol=R.block_volume, cfg=R.block_cfg(), fn=stub, kw=dict(blend='gaussian', noise='anchored', joint=True, seed=SEED), call={})
    return dict(vol=R.shared_volume, cfg=R.shared_cfg(8, batch_size=3), fn=stub,
                kw=dict(blend='gaussian', noise='anchored', joint=True, seed=SEED, samples=2), call=dict(return_std=True))


CASES = {
    'crop-s16': dict(vol=R.shared_volume, cfg=R.shared_cfg(16, batch_size=3), fn=sampler_of, kw={}, call={}),     # 4 kept: batches of 3 and 1
    'crop-s5-anchored-slice': dict(vol=R.shared_volume, cfg=R.shared_cfg(5), fn=sampler_of, kw=dict(noise='anchored', seed=SEED),
                                   call=dict(patch_slice=(1, 2))),                    # the serial-scatter branch
    'crop-block-anchored': dict(vol=R.block_volume, cfg=R.block_cfg(), fn=sampler_of, kw=dict(noise='anchored', seed=SEED), call={}),
    'blend-gaussian-s2-anchored': dict(vol=R.shared_volume, cfg=R.shared_cfg(8, batch_size=3), fn=sampler_of,
                                       kw=dict(blend='gaussian', samples=2, noise='anchored', seed=SEED), call=dict(return_std=True)),
    'blend-constant-block': dict(vol=R.block_volume, cfg=R.block_cfg(), fn=sampler_of, kw=dict(blend='constant'), call={}),
    **{f"joint-{chain}-{'selfcond' if sc else 'plain'}": _joint(chain, False, sc) for chain in ('step', 'multistep', 'heun') for sc in (False, True)},
    **{f"joint-{chain}-block-selfcond": _joint(chain, True, True) for chain in ('step', 'multistep', 'heun')},
    # the sigma-space multistep chain, two samples each: recorded from commit 51a6a1a, the last one with a chain per sampler family
    **{f"joint-{chain}-{'selfcond' if sc else 'plain'}": _joint(chain, False, sc) for chain in ('sigma-base0', 'sigma-base1') for sc in (False, True)},
}


def run_case(name):
    """The trace of one case, as a list of records."""
    from diffusioniqt_amd import inference
    case = CASES[name]
    rec = Recorder()
    vol = torch.from_numpy(case['vol']())
    rec.tag(vol, 'vol')
    patched = {'ops': RecordingOps(rec),
               'convertVolume2subVolume': lambda image, target_shape: rec.record('split', {'image': image, 'target_shape': target_shape},
                                                                                 zeros(*target_shape)),
               'merge_sub_volumes': lambda sub_volumes, original_shape: rec.record(
                   'merge', {'sub_volumes': sub_volumes, 'original_shape': original_shape}, zeros(*original_shape))}
    with pytest.MonkeyPatch.context() as mp:
        for k, v in patched.items():
            mp.setattr(inference, k, v)
        out = inference.VolumeInference(case['cfg'], case['fn'](rec), **case['kw'])(vol, **case['call'])
    rec.record('return', {}, out)
    return rec.trace


def summary(trace):
    counts = collections.Counter(r['op'] for r in trace)
    rest = [r for r in trace if r['op'] != 'min_value']
    return {'counts': dict(sorted(counts.items())), 'sha256': hashlib.sha256(canonical(rest).encode()).hexdigest()}


@pytest.mark.parametrize('name', list(CASES))
def test_launch_trace_is_the_recorded_one(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(CASES)
    trace = run_case(name)
    got = summary(trace)
    where = os.environ.get('DIQT_LAUNCH_TRACE_DUMP')
    if where or got != golden[name]:
        print(f"{name}: full trace written to {dump(name, trace, where, 'volume_launch_trace_')}")
    print(f"{name}: {len(trace)} records, {got['counts']}")
    mins = [r for r in trace if r['op'] == 'min_value']
    assert len(mins) == 1 and mins[0]['x']['t'] == 'vol#0' and mins[0]['x']['off'] == 0     # once per call, on the raw volume
    assert got['counts'] == golden[name]['counts']
    assert got['sha256'] == golden[name]['sha256']


def test_the_cases_reach_every_branch():
    """What the matrix is for: both scatter branches, the split / merge of block mode, every chain's ops, the self-conditioning
    gather (one more ``patch_gather`` per evaluation after the first) and the Heun step without a corrector."""
    with open(GOLDEN) as f:
        counts = {k: v['counts'] for k, v in json.load(f).items()}
    assert counts['crop-s5-anchored-slice']['patch_scatter'] > counts['crop-s5-anchored-slice']['sample'] > 1      # one launch per window
    assert counts['crop-s16']['patch_scatter'] == counts['crop-s16']['sample'] > 1                                 # one per batch
    for name in ('crop-block-anchored', 'blend-constant-block'):
        assert counts[name]['split'] == counts[name]['merge'] == counts[name]['sample'] == 27
    for chain, op in (('step', 'volume_joint_step'), ('multistep', 'volume_joint_multistep')):
        assert counts[f'joint-{chain}-plain'][op] == 2 * 3 and counts[f'joint-{chain}-plain']['volume_joint_finish'] == 2
        assert counts[f'joint-{chain}-selfcond']['patch_gather'] > counts[f'joint-{chain}-plain']['patch_gather']
    assert counts['joint-heun-plain']['volume_joint_heun'] == 2 * (2 * 3 - 1) and counts['joint-heun-plain']['volume_joint_heun_init'] == 2
    assert counts['joint-heun-selfcond']['patch_gather'] > counts['joint-heun-plain']['patch_gather']
    assert counts['joint-heun-block-selfcond']['split'] == 3 * counts['joint-heun-block-selfcond']['merge'] - 27
    for base in (0, 1):                                       # T + 1 fused launches per sample; low-res noise only behind draw_base 1
        plain, sc = counts[f'joint-sigma-base{base}-plain'], counts[f'joint-sigma-base{base}-selfcond']
        assert plain['volume_joint_multistep_sde'] == 2 * (3 + 1) and sc['patch_gather'] > plain['patch_gather']
        assert plain.get('anchored_noise', 0) == base * plain['x0'] and plain['x0'] > 2 * 3


if __name__ == '__main__':              # python -m tests.test_volume_launch_trace_host DIR: dump every full trace, print every summary
    import sys
    for case in CASES:
        t = run_case(case)
        print(case, len(t), dump(case, t, sys.argv[1]), json.dumps(summary(t), sort_keys=True))
