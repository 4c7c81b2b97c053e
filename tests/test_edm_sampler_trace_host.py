"""The launch trace of the ``ElucidatedImagen`` samplers: which ops ``sample`` calls for the Heun sampler, its inpainting loop and
DPM-Solver++ 2M, in which order, with which scalars and on which buffers; what the U-Net is handed; which noise draw goes where; and
the tables and launches of the two window denoisers.  The loops have no CPU fallback, so no other host test runs their control flow.

``elucidated_imagen.ops`` is replaced by recording stand-ins (tests/launch_trace.py) and nothing else is: every stand-in returns zeros
of the right shape, an in-place op the tensor it was given, and the control flow does not depend on data.  Only the public surface is
driven -- ``sample``, and ``window_denoiser`` with its ``x0``, ``finish``, ``normalize`` and tables -- so this file runs unchanged on
any tree that has that surface.  A record is the op name and every bound argument: scalars as they are, floats rounded to fp32, float
tensors as (storage tag, shape, dtype, offset) so that in place against fresh is visible, the per-sample coefficient vectors (1-D, at
most ``batch`` elements) also by value, byte masks and index tensors by value, the float mask of ``mask_blend`` by digest.  The stub
U-Nets record their calls the same way: ``c_noise`` by value (and, in the ``axpby3`` record before it, c_in: between them the sigma of
the evaluation), ``cond_scale``, and which tensor arrived as ``self_cond`` and as the low-res image.  Every entry of a noise list is
tagged ``noise<k>`` beforehand, so a record shows which pop it received; a callable source records each call; the case without a noise
argument runs under ``torch.manual_seed`` and records four normals drawn after the call, which pins how many it consumed.  What each
entry point returned is recorded last.

The model is ``tests.volume_joint_heun_reference.make_elucidated`` on its test schedule ``HP`` (four sigmas, so three steps with a
corrector and the last one to sigma 0 without), a low-res conditioned stub U-Net at 16^3, batch 2; the cascades are two stub U-Nets,
8^2 x 8 frames then 16^3, with image normalisation on.

tests/golden/edm_sampler_trace.json holds, per case, the count per op name and the SHA-256 of the canonical JSON of the trace, and
for the denoiser cases the tables as fp32 hex.  It was recorded from commit b28b2d1 -- the last one with a prologue, a Heun body and
a schedule computation per sampler loop in elucidated_imagen.py -- on a checkout of that commit outside the repository, with this file
and tests/launch_trace.py copied in (``python -m tests.test_edm_sampler_trace_host DIR GOLDEN``), and is the behaviour the refactor to
one table, one Heun loop, one prologue and one chain end had to keep: it is not to be regenerated from later code.  A digest that
differs means launches, arguments, order, buffers or draws changed; set ``DIQT_LAUNCH_TRACE_DUMP=<dir>`` to write the full traces
there (a mismatch writes them to a temporary directory by itself) and diff them against a dump of the older tree."""
import collections
import hashlib
import json
import os

import pytest
import torch

from tests import volume_joint_heun_reference as HN
from tests.launch_trace import Recorder, RecordingOps, canonical, dump, zeros

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'edm_sampler_trace.json')
B, P = 2, 16
SEED = 11


class EDMRecorder(Recorder):
    def describe(self, v, role):
        out = super().describe(v, role)
        if torch.is_tensor(v) and v.is_floating_point():
            if v.ndim == 1 and v.numel() <= B:                                   # a coefficient per sample
                out['v'] = [self.describe(float(e), role) for e in v.tolist()]
            if role.endswith('.mask'):
                out['sha'] = hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest()[:16]
        return out


def _like(key):
    return lambda a: torch.zeros_like(a[key], dtype=torch.float32)


def _into(key):
    return lambda a: a['out'] if a['out'] is not None else torch.zeros_like(a[key], dtype=torch.float32)


# what each stand-in returns, from the arguments bound to the real op's signature
RETURNS = {
    'axpby3': _like('a'), 'add': _like('a'), 'mask_blend': _like('x'), 'q_sample': _like('x0'), 'dynamic_threshold': _like('x0'),
    'abs_quantile': lambda a: zeros(a['x'].shape[0]),
    'nearest_resize': lambda a: zeros(a['x'].shape[0], *a['size'], a['x'].shape[-1]),
    'edm_inpaint_churn': _into('x'), 'multistep_sde_step': _into('x'), 'cell_project': _into('x0'),
}


def stub_unet(rec, name, self_cond, lowres_cond=True):
    """A ``Unet`` subclass ``ElucidatedImagen`` accepts (``__init__`` runs only ``nn.Module.__init__``) that records what it is handed."""
    from diffusioniqt_amd.imagen_pytorch3D import Unet

    def __init__(self):
        torch.nn.Module.__init__(self)
        self.dummy_parameter = torch.nn.Parameter(torch.tensor([0.]))

    def forward_with_cond_scale(self, x, c_noise, **kw):
        return rec.record(name, {'x': x, 'c_noise': c_noise, **dict(sorted(kw.items()))}, torch.zeros_like(x))

    return type('TraceStubUnet', (Unet,), dict(__init__=__init__, forward_with_cond_scale=forward_with_cond_scale, self_cond=bool(self_cond),
                                               lowres_cond=lowres_cond, cast_model_parameters=lambda self, **kw: self))()


def single(rec, churn='churn-on', dynamic=False, self_cond=False):
    return HN.make_elucidated(churn, dynamic, size=P, unet=stub_unet(rec, 'unet', self_cond))


def cascade(rec, churn='churn-on'):
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    return ElucidatedImagen(unets=(stub_unet(rec, 'unet1', False, lowres_cond=False), stub_unet(rec, 'unet2', True)), image_sizes=(P // 2, P),
                            channels=1, condition_on_text=False, auto_normalize_img=True, cond_drop_prob=0.0, dynamic_thresholding=(False, True),
                            dynamic_thresholding_percentile=HN.PERCENTILE, lowres_sample_noise_level=HN.LOWRES_LEVEL,
                            temporal_downsample_factor=(2, 1), **{**HN.HP, 'S_churn': HN.CHURN[churn]})


def volume(rec, role, batch=B, size=P, value=0.):
    t = torch.full((batch, 1, size, size, size), float(value))
    rec.tag(t, role)
    return t


def noise_list(rec, n, shapes=None):
    """``n`` tagged entries ``noise0`` .. (more than any case pops: what is left over is not the trace's business)."""
    out = [zeros(*(shapes[k] if shapes and k < len(shapes) else (B, 1, P, P, P))) for k in range(n)]
    for k, t in enumerate(out):
        rec.tag(t, f'noise{k}')
    return out


def noise_source(rec):
    return lambda shape: rec.record('noise', {'shape': tuple(shape)}, zeros(*shape))


def masks(batch=B):
    m = torch.zeros(batch, P, P, P, dtype=torch.bool)
    m[:, ::2, 1::3] = True
    m[-1, 3] = True
    return m


def sample_case(model=None, noise='list', seed=None, batch_size=B, inpaint=0, consistency=None, images=B, **call):
    """One ``sample`` of the second U-Net of ``single(**model)`` from a 16^3 low-res volume."""
    def run(rec):
        elu = single(rec, **(model or {}))
        kw = dict(call)
        if noise == 'list':
            kw['noise'] = noise_list(rec, 24)
        elif noise == 'callable':
            kw['noise'] = noise_source(rec)
        if inpaint:
            kw.update(inpaint_images=volume(rec, 'known', images, value=0.25), inpaint_masks=masks(images), inpaint_resample_times=inpaint)
        if 'init_images' in kw:
            kw['init_images'] = volume(rec, 'init', value=0.5)
        if consistency is not None:
            kw.update(consistency=(volume(rec, 'meas_up', value=0.125), (2, 2, 4)), consistency_weight=consistency)
        if seed is not None:
            torch.manual_seed(seed)
        out = elu.sample(batch_size=batch_size, video_frames=P, start_image_or_video=volume(rec, 'lowres', images), start_at_unet_number=2,
                         use_tqdm=False, device='cpu', **kw)
        if seed is not None:
            rec.record('rng', {'next': torch.randn(4).tolist()})
        return out
    return run


def cascade_case(stage1_draws, inpaint=0, **call):
    """Both stages of ``cascade`` from one noise list: the first ``stage1_draws`` entries at [B,1,8,8,8], the rest (the low-res noise
    of stage 2 first) at 16^3."""
    def run(rec):
        elu = cascade(rec)
        kw = dict(call)
        if inpaint:
            kw.update(inpaint_images=volume(rec, 'known', value=0.25), inpaint_masks=masks(), inpaint_resample_times=inpaint)
        return elu.sample(batch_size=B, video_frames=P, use_tqdm=False, device='cpu', return_all_unet_outputs=True,
                          noise=noise_list(rec, 40, [(B, 1, P // 2, P // 2, P // 2)] * stage1_draws), **kw)
    return run


def hexed(t):
    return torch.as_tensor(t).to(torch.float32).contiguous().numpy().tobytes().hex()


def denoiser_tables(d):
    """Every attribute table of a window denoiser: numbers as fp32 hex (``sched`` and ``sigmas`` are fp32 values, widened)."""
    out = dict(num_steps=int(d.num_steps), draw_base=int(d.draw_base), self_cond=bool(d.self_cond), heun=bool(d.heun),
               multistep=bool(getattr(d, 'multistep', False)), clamp=[str(float(v)) for v in d.clamp], sigma0=hexed(float(d.sigma0)),
               coefs=hexed(d.coefs), coefs_shape=list(d.coefs.shape), coefs_dtype=str(d.coefs.dtype))
    for name in ('sched', 'sigmas'):
        if hasattr(d, name):
            t = getattr(d, name)
            assert t.dtype == torch.float64 and torch.equal(t, t.float().double())
            out.update({name: hexed(t), name + '_shape': list(t.shape)})
    if hasattr(d, 'eta'):
        out['eta'] = hexed(float(d.eta))
    stages = (0, 1) if d.heun else (0,)
    out['sigma_of'] = [[hexed(float(d.sigma_of(i, s))) for s in stages] for i in range(d.num_steps)]
    return out


def denoiser_case(model=None, **make):
    """``window_denoiser(**make)``: its tables, ``x0`` at every step and stage, ``finish`` with and without known values, ``normalize``."""
    def run(rec):
        elu = single(rec, **(model or {}))
        d = elu.window_denoiser(unet_number=2, **make)
        rec.tables = denoiser_tables(d)
        img, lowres, ln = volume(rec, 'img'), volume(rec, 'lowres'), volume(rec, 'lowres_noise')
        prev = None
        for i in range(d.num_steps):
            for stage in ((0, 1) if d.heun and float(d.sigma_of(i, 1)) != 0 else (0,)):
                args = dict(img=img, lowres=lowres, i=i, self_cond=prev if d.self_cond else None, lowres_noise=ln)
                if d.heun:
                    args['stage'] = stage
                prev = rec.record('x0', args, d.x0(**args))
        x = volume(rec, 'state')[0, 0]                                            # finish takes any shape: one [P,P,P] volume
        rec.record('finish', {'x': x}, d.finish(x))
        known, mask = volume(rec, 'known', value=0.25)[0, 0], masks()[0].float()
        rec.record('finish', {'x': x, 'known': known, 'mask': mask}, d.finish(x, known, mask))
        rec.record('normalize', {'x': known}, d.normalize(known))
        return None
    return run


CASES = {
    # the Heun sampler
    'heun-churn-on': sample_case(),
    'heun-churn-off': sample_case(dict(churn='churn-off')),
    'heun-dynamic': sample_case(dict(dynamic=True)),
    'heun-selfcond': sample_case(dict(self_cond=True)),
    'heun-selfcond-dynamic-churn-off': sample_case(dict(churn='churn-off', dynamic=True, self_cond=True)),
    'heun-skip1': sample_case(skip_steps=1),
    'heun-init': sample_case(init_images=True),
    'heun-sigma-override': sample_case(sigma_min=0.4, sigma_max=1.2),
    'heun-callable': sample_case(noise='callable'),
    'heun-callable-selfcond-skip1': sample_case(dict(self_cond=True), noise='callable', skip_steps=1),
    'heun-seeded': sample_case(noise=None, seed=SEED),
    # its inpainting loop
    'inpaint-r1': sample_case(inpaint=1),
    'inpaint-r2': sample_case(inpaint=2),
    'inpaint-r3': sample_case(inpaint=3),
    'inpaint-r2-selfcond': sample_case(dict(self_cond=True), inpaint=2),
    'inpaint-r2-dynamic-callable-init-skip1': sample_case(dict(dynamic=True), noise='callable', inpaint=2, init_images=True, skip_steps=1),
    'inpaint-r2-broadcast': sample_case(inpaint=2, batch_size=1),                   # batch 1 broadcast to the two inpaint images
    'inpaint-r2-seeded': sample_case(noise=None, seed=SEED, inpaint=2),
    # DPM-Solver++ 2M
    'dpmpp2m-eta0': sample_case(sampler='dpmpp2m'),
    'dpmpp2m-eta0.5': sample_case(sampler='dpmpp2m', eta=0.5),
    'dpmpp2m-eta0-steps3': sample_case(sampler='dpmpp2m', sample_steps=3),
    'dpmpp2m-eta0.5-steps6-dynamic': sample_case(dict(dynamic=True), sampler='dpmpp2m', sample_steps=6, eta=0.5),
    'dpmpp2m-eta0.5-selfcond': sample_case(dict(self_cond=True), sampler='dpmpp2m', eta=0.5),
    'dpmpp2m-eta0-init-sigma-override': sample_case(sampler='dpmpp2m', init_images=True, sigma_min=0.4, sigma_max=1.2),
    'dpmpp2m-eta0.5-callable': sample_case(noise='callable', sampler='dpmpp2m', eta=0.5),
    'dpmpp2m-eta0.5-seeded': sample_case(noise=None, seed=SEED, sampler='dpmpp2m', eta=0.5),
    'dpmpp2m-consistency-w1': sample_case(sampler='dpmpp2m', consistency=1),
    'dpmpp2m-consistency-w0.5-eta0.5-selfcond': sample_case(dict(self_cond=True), sampler='dpmpp2m', eta=0.5, consistency=0.5),
    # two stages from one noise list: how many draws each stage takes (stage 1: the initial image and one per step)
    'cascade-heun': cascade_case(stage1_draws=5),
    'cascade-heun-skip': cascade_case(stage1_draws=4, skip_steps=(1, 2), init_images=None),
    'cascade-inpaint-r2': cascade_case(stage1_draws=1 + 4 * 2 + 3, inpaint=2),
    'cascade-dpmpp2m-eta0.5': cascade_case(stage1_draws=4, sampler='dpmpp2m', eta=0.5),
    'cascade-dpmpp2m-eta0-then-heun': cascade_case(stage1_draws=1, sampler=('dpmpp2m', 'heun'), sample_steps=(3, None)),
    # the window denoisers
    'denoiser-heun-churn-on-selfcond': denoiser_case(dict(self_cond=True)),
    'denoiser-heun-churn-off-dynamic-sigma-override': denoiser_case(dict(churn='churn-off', dynamic=True), sigma_min=0.4, sigma_max=1.2),
    'denoiser-heun-noclamp': denoiser_case(clamp=False, cond_scale=2.),
    'denoiser-dpmpp2m-eta0-steps3': denoiser_case(sampler='dpmpp2m', sample_steps=3),
    'denoiser-dpmpp2m-eta0.5-selfcond': denoiser_case(dict(self_cond=True), sampler='dpmpp2m', eta=0.5),
    'denoiser-dpmpp2m-eta0.5-dynamic-sigma-override': denoiser_case(dict(dynamic=True), sampler='dpmpp2m', eta=0.5, sigma_min=0.4, sigma_max=1.2),
}


def run_case(name):
    """(trace, tables) of one case: a list of records, and the denoiser's tables (None for a ``sample`` case)."""
    from diffusioniqt_amd import elucidated_imagen
    rec = EDMRecorder()
    rec.tables = None
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(elucidated_imagen, 'ops', RecordingOps(rec, RETURNS))
        out = CASES[name](rec)
    rec.record('return', {}, out)
    return rec.trace, rec.tables


def summary(trace, tables):
    counts = collections.Counter(r['op'] for r in trace)
    out = {'counts': dict(sorted(counts.items())), 'sha256': hashlib.sha256(canonical(trace).encode()).hexdigest()}
    if tables is not None:
        out['tables'] = tables
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_sampler_trace_is_the_recorded_one(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(CASES)
    trace, tables = run_case(name)
    got = summary(trace, tables)
    where = os.environ.get('DIQT_LAUNCH_TRACE_DUMP')
    if where or got != golden[name]:
        print(f"{name}: full trace written to {dump(name, trace, where, 'edm_sampler_trace_')}")
    print(f"{name}: {len(trace)} records, {got['counts']}")
    assert got['counts'] == golden[name]['counts']
    assert got.get('tables') == golden[name].get('tables')
    assert got['sha256'] == golden[name]['sha256']


def test_the_cases_reach_every_branch():
    """What the matrix is for, read off the recorded counts: the plain Heun loop never launches the inpainting churn or a paste, the
    inpainting loop runs R passes per step with one churn launch each and one paste at the end, self-conditioning and thresholding
    change what a prediction costs but not how many there are, the multistep sampler is one evaluation and one step launch per step and
    projects every prediction under ``consistency``, and a callable source is asked for exactly the draws a list gives up."""
    with open(GOLDEN) as f:
        counts = {k: collections.Counter(v['counts']) for k, v in json.load(f).items()}
    T = HN.HP['num_sample_steps']
    for name in ('heun-churn-on', 'heun-churn-off', 'heun-dynamic', 'heun-selfcond', 'heun-init', 'heun-sigma-override', 'heun-seeded'):
        assert counts[name]['unet'] == 2 * T - 1 and counts[name]['edm_inpaint_churn'] == counts[name]['mask_blend'] == 0
    assert counts['heun-skip1']['unet'] == 2 * (T - 1) - 1
    assert counts['heun-callable']['noise'] == 1 + 1 + T                                  # the low-res noise, the initial image, one eps per step
    assert counts['heun-init']['add'] == 1 and counts['heun-churn-on']['add'] == 0
    assert counts['heun-dynamic']['dynamic_threshold'] == counts['heun-dynamic']['abs_quantile'] == 2 * T - 1
    for R in (1, 2, 3):
        c = counts[f'inpaint-r{R}']
        assert c['edm_inpaint_churn'] == T * R and c['unet'] == (2 * T - 1) * R and c['mask_blend'] == 1
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    assert counts['inpaint-r2-dynamic-callable-init-skip1']['noise'] == 2 + ElucidatedImagen.inpaint_draws(T - 1, 2)
    assert counts['dpmpp2m-eta0']['unet'] == counts['dpmpp2m-eta0']['multistep_sde_step'] == T
    assert counts['dpmpp2m-eta0-steps3']['unet'] == 3 and counts['dpmpp2m-eta0.5-steps6-dynamic']['unet'] == 6
    assert counts['dpmpp2m-eta0.5-callable']['noise'] == 2 + (T - 1)                     # every step but the last draws
    assert counts['dpmpp2m-consistency-w1']['cell_project'] == T and counts['dpmpp2m-eta0']['cell_project'] == 0
    assert counts['cascade-heun']['unet1'] == counts['cascade-heun']['unet2'] == 2 * T - 1
    assert counts['cascade-heun-skip']['unet1'] == 2 * (T - 1) - 1 and counts['cascade-heun-skip']['unet2'] == 2 * (T - 2) - 1
    assert counts['cascade-dpmpp2m-eta0-then-heun']['unet1'] == 3 and counts['cascade-dpmpp2m-eta0-then-heun']['unet2'] == 2 * T - 1
    assert counts['denoiser-heun-churn-on-selfcond']['unet'] == 2 * T - 1 and counts['denoiser-dpmpp2m-eta0-steps3']['unet'] == 3


if __name__ == '__main__':              # python -m tests.test_edm_sampler_trace_host DIR [GOLDEN]: dump every full trace, print every
    import sys                          # summary and, given a second path, write the summaries there as a golden file
    summaries = {}
    for case in CASES:
        t, tab = run_case(case)
        summaries[case] = summary(t, tab)
        print(case, len(t), dump(case, t, sys.argv[1]), json.dumps(summaries[case]['counts'], sort_keys=True))
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            json.dump(summaries, f, indent=1, sort_keys=True)
            f.write('\n')
