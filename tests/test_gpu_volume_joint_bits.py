"""The output BITS of the joint volume sampler launches, frozen: ``ops.volume_joint_init`` / ``_step`` / ``_multistep`` / ``_multistep_sde`` /
``_heun_init`` / ``_heun``, and ``ops.volume_blend`` / ``ops.volume_joint_finish`` (the launches that share the block layout and the walk).

tests/golden/volume_joint_bits.json holds, per case, the SHA-256 of the bytes of every output tensor.  It was recorded on an MI355X from
commit 51a6a1a, the last one with one kernel per sampler form (volume_joint_step_kernel, volume_joint_multistep_kernel,
volume_joint_multistep_sde_kernel), and is what folding them into one kernel had to keep: it is not to be regenerated from later code.
With ``DIQT_JOINT_BITS_DUMP=<file>`` every case merges its digests into that JSON file instead of comparing them; the cases only call
``ops`` entries that commit has, so the recorder runs on either tree.

Inputs: ``np.random.default_rng(<fixed int>)`` cast to fp32 on the host; P = 8 in a (13, 10, 70) volume (H is no multiple of the 4 rows of a
block, W fills one 64-lane block and part of a second); strides 8 (= P), 5 (does not divide P) and 1 (eight covering windows per axis:
``window_walk``'s four-windows-per-trip loop runs two trips, and fewer with a tail near the faces); about a quarter of the lattice's windows
dropped (``slot = -1``); both tap kinds.  At strides 8 and 5 the rows h >= 8 are uncovered.

Signed zeros are planted, because they are the only inputs at which re-associating the update's last additions changes a bit: at the
voxels ``zero`` (covered ones) the state is -0.0 and every covering prediction 0.0, so with kx > 0 > k0 the sum kx x_t + k0 x0 is
(-0) + (-0) = -0 and the sign of the result is the sign rule of the additions that follow; at ``zero[3:6]`` the history is -0.0 as well and
at ``zero[6:]`` +0.0 (``test_planted_zeros_tell_the_forms_apart`` asserts what that gives)."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'volume_joint_bits.json')
P, VOL = 8, (13, 10, 70)
STRIDES, KINDS = (8, 5, 1), ('gaussian', 'constant')
SEED, DRAW, SAMPLE = 0x123456789, 5, 2
KX, K0, KP = 0.8125, -0.9375, -0.3125
CLAMPS = {'min': (-0.75, 0., 0), 'box': (-1., 1., 1), 'open': (-float('inf'), float('inf'), 1)}
NORM = dict(mean=0.25, std=2.0)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def covered_mask(slot, stride):
    cov = np.zeros(VOL, dtype=bool)
    for g in np.ndindex(*slot.shape):
        if slot[g] >= 0:
            cov[tuple(slice(a * stride, a * stride + P) for a in g)] = True
    return cov


def make_case(stride, kind):
    rng = np.random.default_rng(1000 * stride + KINDS.index(kind))
    lattice = tuple(len(range(0, s - P + 1, stride)) for s in VOL)
    kept = rng.random(lattice) >= 0.25
    slot = np.where(kept, np.cumsum(kept.reshape(-1)).reshape(lattice) - 1, -1).astype(np.int32)
    N = int(kept.sum())
    y = (rng.standard_normal((N, P, P, P)) * 2).astype(np.float32)
    x = (rng.standard_normal(VOL) * 3).astype(np.float32)
    prev = (rng.standard_normal(VOL) * 2).astype(np.float32)
    xn = (rng.standard_normal(VOL) * 3).astype(np.float32)
    patches = (rng.standard_normal((3, N, P, P, P)) * 2).astype(np.float32)
    raw = (rng.random(VOL) * 100 + 1).astype(np.float32)
    raw.reshape(-1)[rng.choice(raw.size, 40, replace=False)] = 0.5               # the background: the volume minimum, 40 times
    cov = covered_mask(slot, stride)
    idx = np.flatnonzero(cov)
    zero = [tuple(int(c) for c in np.unravel_index(idx[len(idx) * (2 * k + 1) // 17], VOL)) for k in range(8)]   # spread out
    for v in zero:
        x[v] = -0.0
        for g in np.ndindex(*lattice):
            o = tuple(c - a * stride for c, a in zip(v, g))
            if slot[g] >= 0 and all(0 <= i < P for i in o):
                y[(slot[g],) + o] = 0.0
                patches[(slice(None), slot[g]) + o] = 0.0
    for v in zero[3:6]:
        prev[v] = -0.0
    for v in zero[6:]:
        prev[v] = 0.0
    return dict(stride=stride, kind=kind, lattice=lattice, N=N, slot=slot, covered=cov, zero=zero, y=y, x=x, prev=prev, xn=xn,
                patches=patches, raw=raw, taps=R.taps_of(P, kind).astype(np.float32))


@pytest.fixture(scope="module")
def cases():
    return {(s, k): make_case(s, k) for s in STRIDES for k in KINDS}


def windows(c):
    return cu(c['y']), cu(c['slot']), cu(c['taps'])


def run_init(c, ops):
    return {'draw0': sha(ops.volume_joint_init(VOL, SEED)), 'draw5-sample2': sha(ops.volume_joint_init(VOL, SEED, sample=SAMPLE, draw=DRAW))}


def run_step(c, ops):
    out, w = {}, windows(c)
    for kn, (cn, cl), with_x0, inplace in itertools.product((0., 0.625), CLAMPS.items(), (True, False), (True, False)):
        x = cu(c['x'])
        x0 = torch.full(VOL, 7., device=DEV) if with_x0 else None
        got = ops.volume_joint_step(*w, x, KX, K0, kn, *cl, c['stride'], SEED, DRAW, SAMPLE, out=x if inplace else None, x0_out=x0)
        assert (got.data_ptr() == x.data_ptr()) == inplace and (inplace or torch.equal(x, cu(c['x'])))
        key = f"kn{kn}-{cn}-{'x0' if with_x0 else 'nox0'}-{'inplace' if inplace else 'fresh'}"
        out[key + '.x'] = sha(got)
        if with_x0:
            out[key + '.x0'] = sha(x0)
    return out


def run_multistep(c, ops):
    out, w = {}, windows(c)
    for with_prev, kp, (cn, cl) in itertools.product((False, True), (0., KP), CLAMPS.items()):
        got, got0 = ops.volume_joint_multistep(*w, cu(c['x']), cu(c['prev']) if with_prev else None, KX, K0, kp, *cl, c['stride'])
        key = f"{'prev' if with_prev else 'noprev'}-kp{kp}-{cn}"
        out[key + '.x'], out[key + '.x0'] = sha(got), sha(got0)
    for kp in (0., KP):                                     # in place on both pairs: x0_out aliases x0_prev
        x, prev = cu(c['x']), cu(c['prev'])
        got, got0 = ops.volume_joint_multistep(*w, x, prev, KX, K0, kp, *CLAMPS['box'], c['stride'], out=x, x0_out=prev)
        assert got.data_ptr() == x.data_ptr() and got0.data_ptr() == prev.data_ptr()
        out[f"alias-kp{kp}.x"], out[f"alias-kp{kp}.x0"] = sha(x), sha(prev)
    return out


def run_multistep_sde(c, ops):
    out, w = {}, windows(c)
    for with_prev, kn, (cn, cl) in itertools.product((False, True), (0., 0.625), CLAMPS.items()):
        got, got0 = ops.volume_joint_multistep_sde(*w, cu(c['x']), cu(c['prev']) if with_prev else None, KX, K0, KP, kn, *cl, c['stride'],
                                                   SEED, DRAW, SAMPLE)
        key = f"{'prev' if with_prev else 'noprev'}-kn{kn}-{cn}"
        out[key + '.x'], out[key + '.x0'] = sha(got), sha(got0)
    for kn in (0., 0.625):
        x, prev = cu(c['x']), cu(c['prev'])
        ops.volume_joint_multistep_sde(*w, x, prev, KX, K0, KP, kn, *CLAMPS['box'], c['stride'], SEED, DRAW, SAMPLE, out=x, x0_out=prev)
        out[f"alias-kn{kn}.x"], out[f"alias-kn{kn}.x0"] = sha(x), sha(prev)
    got, none = ops.volume_joint_multistep_sde(None, None, None, None, None, 0., 0., 0., 80., -1., 1., 1, c['stride'], SEED, DRAW, SAMPLE,
                                               shape=VOL)
    assert none is None
    out['initial-kn80'] = sha(got)
    return out


def run_heun(c, ops):
    out, w = {}, windows(c)
    for kc in (0., 0.625):
        out[f"init-kc{kc}"] = sha(ops.volume_joint_heun_init(VOL, 80., kc, SEED, draw=DRAW, sample=SAMPLE))
    for cn, cl in CLAMPS.items():
        vols = cu(c['x']), cu(c['xn']), cu(c['prev'])
        ops.volume_joint_heun(*w, *vols, 1, (1.25, -0.25), 0., *cl, c['stride'])
        out.update({f"phase1-{cn}.{n}": sha(v) for n, v in zip(('xh', 'xn', 'x0'), vols)})
        for kc in (0., 0.625):
            vols = cu(c['x']), cu(c['xn']), cu(c['prev'])
            ops.volume_joint_heun(*w, *vols, 2, (1.125, -0.125, 0.375, -0.375), kc, *cl, c['stride'], SEED, DRAW, SAMPLE)
            out.update({f"phase2-kc{kc}-{cn}.{n}": sha(v) for n, v in zip(('xh', 'xn', 'x0'), vols)})
    return out


def _min_val(c):
    return float((np.float32(c['raw'].min()) - np.float32(NORM['mean'])) / np.float32(NORM['std']))


def run_blend(c, ops):
    out = {}
    for S in (1, 3):
        mean, dev = ops.volume_blend(cu(c['patches'][:S]), cu(c['slot']), cu(c['taps']), cu(c['raw']), NORM['mean'], NORM['std'], _min_val(c),
                                     -0.125, c['stride'], S > 1)
        out[f"S{S}.mean"] = sha(mean)
        if S > 1:
            out[f"S{S}.std"] = sha(dev)
    return out


def run_finish(c, ops):
    out, slot, raw = {}, cu(c['slot']), cu(c['raw'])
    m = m2 = None
    for s, state in enumerate((c['x'], c['xn'], c['prev'])):
        m, m2, dev = ops.volume_joint_finish(cu(state), slot, raw, P, c['stride'], NORM['mean'], NORM['std'], _min_val(c), -0.125, s, 3, m, m2,
                                             want_std=True)
        out[f"s{s}.mean"], out[f"s{s}.m2"] = sha(m), sha(m2)
    out['std'] = sha(dev)
    return out


ENTRIES = {'init': run_init, 'step': run_step, 'multistep': run_multistep, 'multistep_sde': run_multistep_sde, 'heun': run_heun,
           'blend': run_blend, 'finish': run_finish}


@pytest.mark.parametrize('entry', list(ENTRIES))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('stride', STRIDES)
def test_output_bits_are_the_recorded_ones(cases, stride, kind, entry):
    from diffusioniqt_amd import ops
    name = f"{entry}-s{stride}-{kind}"
    got = ENTRIES[entry](cases[stride, kind], ops)
    assert len(set(got.values())) > 1, name
    where = os.environ.get('DIQT_JOINT_BITS_DUMP')
    if where:
        table = {}
        if os.path.exists(where):
            with open(where) as f:
                table = json.load(f)
        table[name] = got
        with open(where, 'w') as f:
            json.dump(table, f, indent=0, sort_keys=True)
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(f"{e}-s{s}-{k}" for e in ENTRIES for s in STRIDES for k in KINDS)
    bad = sorted(k for k in set(got) | set(golden[name]) if got.get(k) != golden[name].get(k))
    assert not bad, f"{name}: {len(bad)} of {len(got)} outputs differ from the recorded bits: {bad[:8]}"


def test_the_inputs_are_what_the_cases_need(cases):
    for (stride, kind), c in cases.items():
        cov, slot = c['covered'], c['slot']
        assert c['N'] == slot.max() + 1 and 0.1 <= (slot < 0).mean() <= 0.4, (stride, kind)         # about a quarter dropped
        if stride != 1:
            assert cov.any() and not cov.all() and not cov[:, 8:].any(), (stride, kind)
        assert len(set(c['zero'])) == 8 and all(cov[v] for v in c['zero'])
        assert all(np.signbit(c['x'][v]) and c['x'][v] == 0 for v in c['zero'])
        assert all(np.signbit(c['prev'][v]) and c['prev'][v] == 0 for v in c['zero'][3:6])
    windows_along_w = {int(min(x, 62) - max(0, x - P + 1) + 1) for x in range(VOL[2])}             # stride 1
    assert max(windows_along_w) == 8 and windows_along_w & {5, 6, 7} and windows_along_w & {1, 2, 3}


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('stride', STRIDES)
def test_planted_zeros_tell_the_forms_apart(cases, stride, kind):
    """At the planted voxels u = fma(kx, -0, k0 * +0) = -0 (kx > 0 > k0), and IEEE addition gives (-0) + (-0) = -0, (-0) + (+0) = +0:
    the multistep form adds kp * prev = -0 for (kp, prev) in {(0, -0), (< 0, +0)} and +0 for {(0, +0), (< 0, -0)}; the step form with
    kn = 0 adds 0 * 0 = +0; the SDE form with kn = 0 adds nothing after the history term."""
    from diffusioniqt_amd import ops
    c, w, cl = cases[stride, kind], windows(cases[stride, kind]), CLAMPS['box']
    z = c['zero']

    def at(t, vs):
        """The sign bits of the zeros at ``vs``."""
        a = t.cpu().numpy()
        assert all(a[v] == 0 for v in vs)
        return [bool(np.signbit(a[v])) for v in vs]
    step = ops.volume_joint_step(*w, cu(c['x']), KX, K0, 0., *cl, stride, SEED, DRAW, SAMPLE)
    assert at(step, z) == [False] * 8
    m0, x0 = ops.volume_joint_multistep(*w, cu(c['x']), cu(c['prev']), KX, K0, 0., *cl, stride)
    assert at(m0, z[3:]) == [True] * 3 + [False] * 2 and at(x0, z) == [False] * 8
    mp, _ = ops.volume_joint_multistep(*w, cu(c['x']), cu(c['prev']), KX, K0, KP, *cl, stride)
    assert at(mp, z[3:]) == [False] * 3 + [True] * 2
    none, _ = ops.volume_joint_multistep(*w, cu(c['x']), None, KX, K0, KP, *cl, stride)            # no history: prev = +0
    assert at(none, z) == [True] * 8
    sde, _ = ops.volume_joint_multistep_sde(*w, cu(c['x']), cu(c['prev']), KX, K0, KP, 0., *cl, stride, SEED, DRAW, SAMPLE)
    assert at(sde, z[3:]) == [False] * 3 + [True] * 2
