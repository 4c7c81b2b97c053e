"""Data-consistent sampling, the part every sampler shares: which combinations of the nine ``consistency*`` keywords are admitted, and
which launch a step takes.  ``Imagen.sample`` / ``p_sample_loop``, ``ElucidatedImagen.sample`` / ``one_unet_sample`` and
``VolumeInference`` take the same keywords, hand them to ``plan`` as they received them and keep what it returns: None (no
``consistency``) or a ``Plan``.  The measurement models themselves are described in the docstring of ``inference``; the kernels are
behind ``ops``.

The keywords:
* ``consistency=(measurement, cell)`` with ``consistency_weight=w`` in (0, 1]: ``cell`` = (fz, fy, fx), 2 <= fz fy fx <= 64.  A one-call
  sampler takes the measurement replicated onto the grid it samples (``meas_up`` [B,C,P,P,P], ``ops.cell_replicate``), in state space
  (``ElucidatedImagen.sample`` takes it in the units it returns); ``VolumeInference`` takes the raw measurement [D/fz, H/fy, W/fx].
  Every x0 prediction is replaced by x0 + w A+(y - A x0) (DDNM).  The Heun sampler (two predictions per step) takes it with
  ``consistency_heun`` only; it goes with neither inpainting, ``init_images`` nor ``skip_steps``; the cell must divide the sampled cube
  -- in the crop and blend modes of ``VolumeInference`` the stride and the window.
* ``consistency_profile=(pz, py, px)``: the measurement of a cell is the weighted mean of a slice profile (``ops.cell_profile``).
* ``consistency_operator=A``: a tile-local linear measurement (``ops.tile_operator``); the measurement is then t = A+ y on the grid, for
  ``VolumeInference`` the raw [m, D/fz, H/fy, W/fx] stack.  Not with a profile (one row of an operator) or ``consistency_noise``.
* ``consistency_slab=(pz, py, px)``: slice profiles that overlap between neighbouring cells along z (``ops.slab_profile``).  With none of
  the other modes.
* ``consistency_band=(hz, hy, hx)`` or ``(hz, hy, hx, offset)``: the measurement is the central box of the k-space of the periodic
  domain, sampled on the low-res grid (``ops.band_table``): per axis None (the full band of the low-res grid) or the weights of the
  frequencies k = 0 .. len - 1; ``offset`` = three numbers in high-res voxels or 'centre'.  The measurement is then t = A+ y on the
  grid (``ops.band_backproject``), for ``VolumeInference`` the raw [D/fz, H/fy, W/fx] volume.  The operator crosses every tile border:
  the domain of a one-call sampler is its cube, and ``VolumeInference`` takes it with ``joint=True`` only.  With none of the other modes.
* ``consistency_noise=sigma`` (a cell mean or a profile): the deviation of the measurement's noise (DDNM+).  Every step gets its own
  weight, capped by ``consistency_weight``, and a reduction of its fresh normals in the range of A
  (``ops.consistency_noise_schedule``).  It needs a chain with a stochastic step.
* ``consistency_row_noise=sigma`` (an operator): the deviation of the noise of each row of A, one number or m of them; every singular
  direction of the whitened operator takes that schedule on its own (``ops.tile_noise_operator`` / ``ops.tile_noise_tables``).  Not with
  ``consistency_noise`` or a profile; a stochastic chain; a cell whose launch plans at most 64 KiB of LDS.
* ``consistency_heun='both'`` or ``'predictor'``: the stochastic Heun sampler of ``ElucidatedImagen`` (``sampler='heun'``, or a
  joint denoiser with ``heun``) under ``consistency``.  ``'both'``: the prediction of either U-Net evaluation of a step is replaced by
  its projection; ``'predictor'``: the first alone (at sigma_hat), the corrector's stays the network's.  The step that ends at
  sigma = 0 has no corrector, and its predictor row is (0, 1): either way the chain ends in its last projected prediction.  There is
  no "corrector only" (it would leave the final state unprojected).  Per window with any of the five modes (the band, in
  ``VolumeInference``, with ``joint=True`` only -- and there not with Heun); with ``joint=True`` the cell mean, a profile or an
  operator: the joint step launches of the slab and the band carry the three linear update forms only.  With no other sampler, and
  with neither ``consistency_noise`` nor ``consistency_row_noise``: Heun's noise is the churn BEFORE the evaluation, and the shaped
  normal that follows a step of DDNM+ has no counterpart there.  Without the keyword Heun stays refused.
Every keyword but the first rides on ``consistency``, ``consistency_row_noise`` also on ``consistency_operator``.  A refusal is a
``ValueError`` raised before anything touches the device; it begins with the entry point's name and names the keyword at fault, and
what ``consistency`` (or the operator) refuses also names the keyword that rides on it.

The ladder of a step, resolved per step once per chain (``Chain.steps``): ``plain`` -- the family's own step, no projection (weight 0:
the step with kn = 0 of a noise-aware chain); ``constant`` -- the projection of the mode with one weight (``ops.cell_project`` /
``cell_project_profile`` / ``tile_project`` / ``slab_project`` / ``band_project``, or the fused
``ops.volume_joint_consistent*_step``, or ``ops.volume_joint_consistent_heun`` in a phase of a joint Heun chain); ``noise`` -- the
projection with the step's own weights that also shapes the step's normals (``ops.cell_project_noise`` / ``tile_project_noise`` and
their fused launches).  A projected prediction is not clamped again: the
projection launch clamps first, the step runs with the clamp off.

A further measurement model adds a branch to ``plan`` (its admission rules and host table), one to ``Chain.__init__`` (its device
table), a rung to ``Chain.project`` and ``Chain.joint_step`` (``Chain.joint_heun``, if it has a Heun launch), and its wrappers in
``ops``."""
from contextlib import contextmanager

import torch

from . import ops

HEUN = ('both', 'predictor')                                 # ``consistency_heun``: which predictions of a Heun step are projected
NO_CLAMP = (-float('inf'), float('inf'), 1)                  # ``ddpm_step``'s box mode with an infinite box: the identity, bit for bit


@contextmanager
def _riders(slab, noise, row_noise, band=None, heun=None):
    """A ``ValueError`` raised inside keeps its wording and also names the given keyword that rides on what refused."""
    try:
        yield
    except ValueError as err:
        msg = str(err)
        for name, value, note in (('consistency_slab', slab, "consistency_slab rides on consistency"),
                                  ('consistency_band', band, "consistency_band rides on consistency"),
                                  ('consistency_heun', heun, "consistency_heun rides on consistency"),
                                  ('consistency_noise', noise, f"consistency_noise={noise!r} rides on consistency"),
                                  ('consistency_row_noise', row_noise,
                                   f"consistency_row_noise={row_noise!r} rides on consistency_operator")):
            if value is not None and name not in msg:
                msg = f"{msg} ({note})"
        raise ValueError(msg) from None


def slope(state_space):
    """The slope of an affine ``state_space`` / ``normalize_img`` map, state_space(1) - state_space(0), in float64."""
    unit = state_space(torch.tensor([0., 1.], dtype=torch.float64))
    return float(unit[1] - unit[0])


def in_units(sigma, std=1., slope=1.):
    """A noise deviation (one number or a sequence, already checked) under the change of units the measurement itself takes: divided
    by ``std``, then multiplied by |``slope``|."""
    if torch.is_tensor(sigma) or type(sigma).__module__ == 'numpy':
        sigma = sigma.tolist()
    if isinstance(sigma, (tuple, list)):
        return [float(v) / float(std) * abs(float(slope)) for v in sigma]
    return float(sigma) / float(std) * abs(float(slope))


def _sampled_pair(who, consistency, weight, shape, has_inpainting, init_images, skip_steps, sampler, heun=None):
    """``consistency`` of a one-call sampler that generates ``shape`` = [B,C,P,P,P]: the checked ``(meas_up, cell, weight)``."""
    if not isinstance(consistency, (tuple, list)) or len(consistency) != 2:
        raise ValueError(f"{who}: consistency must be (meas_up, cell), got {type(consistency).__name__}")
    if sampler == 'heun' and heun is None:
        raise ValueError(f"{who}: consistency is not offered with the Heun sampler (two predictions per step): use sampler='dpmpp2m' "
                         f"(or say which predictions to project: consistency_heun='both' or 'predictor')")
    if has_inpainting:
        raise ValueError(f"{who}: consistency and inpainting are not offered together")
    if init_images is not None or skip_steps is not None:
        raise ValueError(f"{who}: consistency takes neither init_images nor skip_steps")
    meas_up, cell = consistency
    cell, weight = ops.consistency_cell(who, cell, weight, [(shape[2 + a], a) for a in range(3)])
    if not torch.is_tensor(meas_up) or not meas_up.is_floating_point() or tuple(meas_up.shape) != tuple(shape):
        got = f"{meas_up.dtype} {tuple(meas_up.shape)}" if torch.is_tensor(meas_up) else type(meas_up).__name__
        raise ValueError(f"{who}: the consistency measurement must be a float tensor of the sampled shape {tuple(shape)} (replicated "
                         f"onto the high-res grid, ops.cell_replicate), got {got}")
    return meas_up, cell, weight


def _volume_pair(who, consistency, weight, window, rows, heun=None):
    """``consistency`` of ``VolumeInference``: the checked ``(measurement fp32, cell, weight)``, the tensor on the host or the device as
    it was given.  ``rows``: an operator is given and the measurement is [m, D/fz, H/fy, W/fx], one volume per row of it."""
    if not isinstance(consistency, (tuple, list)) or len(consistency) != 2:
        raise ValueError(f"{who}: consistency must be (measurement, cell), got {type(consistency).__name__}")
    if window['inpaint']:
        raise ValueError(f"{who}: consistency and inpaint are not offered together")
    meas, cell = consistency
    cell, weight = ops.consistency_cell(who, cell, weight)
    meas = torch.as_tensor(meas)
    if rows and (meas.ndim != 4 or not meas.is_floating_point()):
        raise ValueError(f"{who}: with consistency_operator the consistency measurement must be a float [m, D/fz, H/fy, W/fx] tensor, "
                         f"one volume per row of the operator, got {meas.dtype} {tuple(meas.shape)}")
    if not rows and (meas.ndim != 3 or not meas.is_floating_point()):
        raise ValueError(f"{who}: the consistency measurement must be a float [D/fz, H/fy, W/fx] tensor, got {meas.dtype} "
                         f"{tuple(meas.shape)}")
    if window['joint'] and getattr(window['denoiser'], 'heun', False) and heun is None:
        raise ValueError(f"{who}: consistency is not offered with the EDM Heun denoiser (two predictions per step and three joint "
                         f"volumes): use window_denoiser(sampler='dpmpp2m') (or say which predictions to project: "
                         f"consistency_heun='both' or 'predictor')")
    if window['joint'] and not hasattr(window['denoiser'], 'state_space'):
        raise ValueError(f"{who}: joint=True with consistency needs a denoiser with state_space(x), the map of the measurement into "
                         f"the space of the state")
    return meas.float(), cell, weight


def plan(who, launch, consistency, weight=1., profile=None, noise=None, operator=None, row_noise=None, slab=None, band=None, *, shape=None,
         window=None, stochastic=True, has_inpainting=False, init_images=None, skip_steps=None, sampler=None, heun=None):
    """The admission rules of the nine keywords (the module docstring), run once and in one order -- Heun, band, slab, row noise,
    operator, the pair itself, the profile, the noise deviation, the LDS plans -- for the entry point ``who``: None without
    ``consistency``, else the ``Plan``.  ``launch`` is the ``ops`` of the calling module: the rules and host tables here are
    ``ops``'s own host arithmetic, but everything that touches the device -- the replication, the back-projection, the workspace,
    every projection and step -- goes through the namespace its sampler launches through.  A one-call sampler gives the ``shape``
    [B,C,P,P,P] it generates and what else its rules depend on: whether its chain has a ``stochastic`` step, ``has_inpainting``,
    ``init_images``, ``skip_steps`` and the ``sampler`` name; every entry point hands ``consistency_heun`` on as ``heun``.
    ``VolumeInference`` gives ``window`` instead: a dict of the window ``edge``, the ``stride``, ``joint``, the ``denoiser`` (its
    second argument), whether it inpaints (``inpaint``) and the z-score's ``mean`` / ``std``."""
    has = consistency is not None
    if heun is not None:
        if not has:
            raise ValueError(f"{who}: consistency_heun needs consistency=(measurement, cell)")
        if heun not in HEUN:
            raise ValueError(f"{who}: consistency_heun must be 'both' (both predictions of a Heun step are projected) or 'predictor' "
                             f"(the first alone), got {heun!r}")
        joint_heun = window is not None and window['joint'] and getattr(window['denoiser'], 'heun', False)
        if (window is None and sampler != 'heun') or (window is not None and window['joint'] and not joint_heun):
            raise ValueError(f"{who}: consistency_heun goes with the Heun sampler of ElucidatedImagen only (sampler='heun', "
                             f"window_denoiser()): every other sampler has one prediction per step and projects it without the keyword")
        for other, name in ((noise, 'consistency_noise'), (row_noise, 'consistency_row_noise')):
            if other is not None:
                raise ValueError(f"{who}: consistency_heun and {name} are not offered together: the Heun sampler's noise is the churn "
                                 f"before the evaluation, and the shaped normal that follows a step of DDNM+ has no counterpart there")
        for other, name in ((slab, 'consistency_slab'), (band, 'consistency_band')):
            if other is not None and joint_heun:
                raise ValueError(f"{who}: consistency_heun and {name} are not offered together with joint=True: the joint step kernels "
                                 f"of the {name[12:]} carry the three linear update forms only, not the Heun phases")
    if band is not None:
        if not has:
            raise ValueError(f"{who}: consistency_band needs consistency=(measurement, cell)")
        for other, name in ((profile, 'consistency_profile'), (noise, 'consistency_noise'), (operator, 'consistency_operator'),
                            (row_noise, 'consistency_row_noise'), (slab, 'consistency_slab')):
            if other is not None:
                raise ValueError(f"{who}: consistency_band and {name} are not offered together")
        if not isinstance(band, (tuple, list)) or len(band) not in (3, 4):
            raise ValueError(f"{who}: consistency_band must be (hz, hy, hx) or (hz, hy, hx, offset), got {band!r}")
        if window is not None and not window['joint']:
            raise ValueError(f"{who}: consistency_band needs joint=True: the band's projector crosses every window border, and a window "
                             f"of t = A+ y is not the t of a window (the crop and blend modes project window by window)")
    if slab is not None:
        if not has:
            raise ValueError(f"{who}: consistency_slab needs consistency=(meas_up, cell)")
        for other, name in ((profile, 'consistency_profile'), (noise, 'consistency_noise'), (operator, 'consistency_operator'),
                            (row_noise, 'consistency_row_noise')):
            if other is not None:
                raise ValueError(f"{who}: consistency_slab and {name} are not offered together")
    if row_noise is not None:
        if operator is None:
            raise ValueError(f"{who}: consistency_row_noise needs consistency_operator=A (and consistency=(target_up, cell)): it is the "
                             f"noise of each row of A; the noise of a plain cell mean is consistency_noise")
        if noise is not None or profile is not None:
            raise ValueError(f"{who}: consistency_row_noise is not offered together with consistency_noise or consistency_profile: give "
                             f"the operator all its rows and every row its deviation")
        if not stochastic:
            raise ValueError(f"{who}: consistency_row_noise needs a sampler with fresh noise per step (ddpm, ddim or dpmpp2m with eta > "
                             f"0): a deterministic chain would never project; use a constant consistency_weight < 1 there")
    p = None
    with _riders(slab, noise, row_noise, band, heun):
        if operator is not None:
            if not has:
                raise ValueError(f"{who}: consistency_operator needs consistency=(measurement, cell)")
            if profile is not None:
                raise ValueError(f"{who}: consistency_operator and consistency_profile are not offered together: a profile is the "
                                 f"single row u of a measurement; give the operator all its rows")
            if noise is not None:
                raise ValueError(f"{who}: consistency_operator and consistency_noise are not offered together (DDNM+ for a general A "
                                 f"needs a weight per singular direction: that is consistency_row_noise)")
        if not has and profile is not None:
            raise ValueError(f"{who}: consistency_profile needs consistency=(measurement, cell)")
        if has:
            if window is None:
                pair = _sampled_pair(who, consistency, weight, shape, has_inpainting, init_images, skip_steps, sampler, heun)
            else:
                pair = _volume_pair(who, consistency, weight, window, operator is not None, heun)
            p = Plan(who, launch, *pair, profile, operator, row_noise, slab, band, **({} if window is None else
                                                                             dict(mean=window['mean'], std=window['std'])))
            p.heun = heun
            if operator is not None:
                p.mode, p.op = 'tile', ops.tile_operator(p.cell, operator)
                if window is not None and p.measurement.shape[0] != p.op.m:
                    raise ValueError(f"{who}: the consistency_operator has m = {p.op.m} rows, the consistency measurement "
                                     f"{tuple(p.measurement.shape)} has {p.measurement.shape[0]} volumes")
                if row_noise is not None:                    # the whitened operator: its effective A+ makes t, its P the table
                    p.op = ops.tile_noise_operator(p.cell, p.op, row_noise)
                if window is not None:                       # what a sampler call takes: the decomposition is not made again
                    p.operator = p.op
            elif band is not None:                           # the table for the cubes of a sampler; a joint chain makes its own per
                p.mode = 'band'                              # volume: the domain is the whole volume
                if window is None:
                    p.band_table = p.band_of(shape[2:])
            elif slab is not None:                           # the table for the cubes of a sampler; a joint chain makes its own per
                p.mode = 'slab'                              # volume, whose depth sets the number of run positions
                p.slab_table = ops.slab_profile(p.cell, slab, jmax=1 if window is not None else shape[2] // p.cell[0])
            elif profile is not None:
                p.mode, p.profile_table = 'profile', ops.cell_profile(p.cell, profile)
    if noise is not None:
        noise = ops.consistency_noise_sigma(who, noise, has, stochastic)
    if p is None:
        return None
    p.noise = noise
    with _riders(slab, noise, row_noise, band, heun):
        # the cubes a projection launch sees; None: the fused launch of a joint chain, which rides the window's taps
        edge = shape[2] if window is None else None if window['joint'] else window['edge']
        if row_noise is not None:
            ops.tile_noise_plan(who, p.op.cell, 0 if window is None else window['edge'], edge)
        if slab is not None and edge is not None:
            ops.slab_plan(who, p.cell, edge)
        if window is not None and window['joint']:
            p.state_space = window['denoiser'].state_space
        elif window is not None:
            for f in p.cell:                                 # per axis: origins are multiples of the stride, a sampler call sees the window
                if window['stride'] % f or window['edge'] % f:
                    raise ValueError(f"{who}: the consistency cell {p.cell} must divide the stride {window['stride']} and the window "
                                     f"{window['edge']}: a per-window projection is defined for cells inside a window only (joint=True "
                                     f"projects on the whole volume)")
    return p


class Plan:
    """What ``plan`` admitted.  ``measurement``, ``cell``, ``weight``: the checked pair; ``profile``, ``operator``, ``row_noise``,
    ``slab``, ``band``, ``heun``: as given (what a sampler call takes); ``noise``: the checked deviation or None; ``mode``: ``'cell'``,
    ``'profile'``, ``'tile'``, ``'slab'`` or ``'band'``, and its host table -- ``profile_table`` (``ops.cell_profile``), ``op`` (the
    ``ops.TileOperator``, whitened under ``row_noise``), ``slab_table`` (the ``ops.SlabTable`` for a sampler's cubes) or ``band_table``
    (the ``ops.BandTable`` for a sampler's cubes; ``band_of(shape)`` makes the one of a volume, once); for ``VolumeInference`` the
    z-score's ``mean``
    / ``std`` and, in joint mode, the denoiser's ``state_space``."""
    mode, op, profile_table, slab_table, band_table, noise, state_space, heun = 'cell', None, None, None, None, None, None, None

    def __init__(self, who, launch, measurement, cell, weight, profile, operator, row_noise, slab, band=None, mean=0., std=1.):
        self.who, self.launch, self.measurement, self.cell, self.weight = who, launch, measurement, cell, weight
        self.profile, self.operator, self.row_noise, self.slab, self.band = profile, operator, row_noise, slab, band
        self.mean, self.std = mean, std
        self._band_tables = {}

    def band_of(self, shape):
        """The host ``ops.BandTable`` of ``consistency_band`` for the periodic domain ``shape``, made once per shape; its refusals begin
        with the entry point's name."""
        shape = tuple(int(s) for s in shape)
        if shape not in self._band_tables:
            try:
                ops.band_plan("band_plan", shape)
                self._band_tables[shape] = ops.band_table(shape, self.cell, tuple(self.band[:3]), *self.band[3:])
            except ValueError as err:
                raise ValueError(f"{self.who}: {err}") from None
        return self._band_tables[shape]

    def admit_volume(self, shape):
        """``ValueError`` for a ``VolumeInference`` measurement that is not the volume's ``shape`` divided by the cell."""
        if tuple(s * f for s, f in zip(self.measurement.shape[-3:], self.cell)) != tuple(shape):
            with _riders(self.slab, self.noise, self.row_noise, self.band, self.heun):
                raise ValueError(f"{self.who}: the consistency measurement {tuple(self.measurement.shape)} times the cell {self.cell} "
                                 f"is not the volume's shape {tuple(shape)}")

    def volume(self, device):
        """The measurement of ``VolumeInference`` on the high-res grid, z-scored like the low-res volume, on ``device``: fp32 [D,H,W]
        (``admit_volume`` has checked its shape).  An operator's t = A+ y is made here, once per volume: P 1 = 1, so the z-score of t
        is the t of the z-scored acquisition; the band's t = A+ y likewise, with the table of this volume."""
        meas = self.measurement.to(device)
        if self.mode == 'band':
            table = self.band_of(tuple(s * f for s, f in zip(meas.shape, self.cell))).to(device)
            up = self.launch.band_backproject(meas.contiguous(), table)
        else:
            up = self.launch.cell_replicate(meas, self.cell) if self.op is None else self.launch.tile_backproject(meas.contiguous(), self.op)
        return ((up - self.mean) / self.std).contiguous()

    def keywords(self, measurement, std=1., slope=1.):
        """What a sampler call takes: ``measurement`` (the batch's windows of ``volume``, or ``meas_up`` in other units) with the
        cell and the weight, and every other keyword exactly when it was given -- the deviations under the change of units
        ``measurement`` has taken (``in_units``)."""
        kw = dict(consistency=(measurement, self.cell), consistency_weight=self.weight)
        given = dict(consistency_profile=self.profile, consistency_noise=self.noise, consistency_operator=self.operator,
                     consistency_row_noise=self.row_noise, consistency_slab=self.slab, consistency_band=self.band,
                     consistency_heun=self.heun)
        for name in ('consistency_noise', 'consistency_row_noise'):
            if given[name] is not None:
                given[name] = in_units(given[name], std, slope)
        return {**kw, **{k: v for k, v in given.items() if v is not None}}

    def prepare(self, rows, device, shape=None):
        """The state of one chain (``Chain``), made once per chain of a one-call sampler or -- with the volume's ``shape`` -- once
        per volume of a joint chain.  ``rows``: the chain's host table, (kx, k0, kn) or (kx, k0, kp, kn) per step."""
        return Chain(self, rows, device, shape)


class Chain:
    """What the steps of one chain read, on the device: ``meas`` (the measurement in state space: ``meas_up`` of a sampler, the
    z-scored volume through ``state_space`` of a joint chain), ``table`` (the profile's [2, n], the operator's P, the ``SlabTable`` of
    this depth, the ``BandTable`` of this cube or volume, or None), ``tables`` ([T, 2, n, n] of ``consistency_row_noise``, one upload),
    ``slab`` (the workspace and coefficient volume of the joint slab launches), ``band_ws`` (the five volumes of the joint band
    launches) and ``steps``: per step ``(rung, weight, shrink)`` with rung ``'plain'``, ``'constant'`` or
    ``'noise'`` (the module docstring), resolved on the fp32 values of the schedule."""

    def __init__(self, plan, rows, device, shape=None):
        p, joint, self.launch = plan, shape is not None, plan.launch
        self.mode, self.cell, self.heun = p.mode, p.cell, p.heun
        self.meas = p.state_space(p.volume(device)).contiguous() if joint else p.measurement.to(device).float().contiguous()
        self.table = self.tables = self.slab = self.band_ws = None
        if p.mode == 'band':                                 # the volume's table was made for ``p.volume``; the workspace once per volume
            self.table = (p.band_of(shape) if joint else p.band_table).to(device)
            self.band_ws = self.launch.band_workspace(shape, device) if joint else None
        elif p.mode == 'slab':
            table = ops.slab_profile(p.cell, p.slab, jmax=shape[0] // p.cell[0]) if joint else p.slab_table
            self.table = table.to(device)
            self.slab = self.launch.slab_workspace(shape, p.cell, device) if joint else None
        elif p.mode != 'cell':
            self.table = (p.op.table if p.mode == 'tile' else p.profile_table).to(device)
        rows = [[float(v) for v in r] for r in (rows.tolist() if torch.is_tensor(rows) else rows)]
        rows = [(r[0], r[1], 0., r[2]) if len(r) == 3 else tuple(r) for r in rows]           # a first-order row has no history term
        self.steps = [('constant', p.weight, 0.)] * len(rows)
        if p.noise is None and p.row_noise is None:
            return
        # the deviation in the units the chain projects in: the z-score and the slope of ``state_space``, as the measurement
        units = (p.std, slope(p.state_space)) if joint else (1., 1.)
        if p.noise is not None:                              # (w_i, shrink_i) once per chain, from the host table
            schedule = ops.consistency_noise_dispatch(ops.consistency_noise_schedule(
                rows, ops.cell_norm(p.cell, p.profile_table), in_units(p.noise, *units), p.weight))
            self.steps = [('plain', 0., 0.) if not w > 0 else ('noise', w, s) if s > 0 else ('constant', w, 0.) for w, s in schedule]
        else:                                                # the tables of every step and their kinds: one upload
            tables, kinds = ops.tile_noise_tables(p.op, ops.tile_noise_schedule(p.op, rows, in_units(float(p.op.row_noise.min()), *units),
                                                                                p.weight))
            self.tables = tables.to(device)
            self.steps = [('noise', 0., 0.) if kind == 'noise' else ('constant', w, 0.) if w > 0 else ('plain', 0., 0.) for kind, w in kinds]

    def project(self, i, pred, normals, clamp=None):
        """Step ``i`` of a one-call loop: at most one projection launch on the prediction ``pred`` [B,C,P,P,P], which clamps with
        ``clamp`` = (lo, hi, mode) first (None: ``pred`` arrives clamped).  ``normals()`` gives the step's normals (or None); it is
        called before the launch that shapes them and after any other.  Returns ``(pred, normals, clamp)``: the prediction and the
        normals the step is to use (new tensors where a launch made them) and the clamp it must still apply."""
        ops, (rung, weight, shrink) = self.launch, self.steps[i]        # ``ops``: the calling module's from here on
        if rung == 'plain':
            return pred, normals(), clamp
        if rung == 'noise' and self.mode == 'tile':
            pred, eps = ops.tile_project_noise(pred, self.meas, normals(), self.cell, self.tables[i], clamp=clamp)
        elif rung == 'noise':
            pred, eps = ops.cell_project_noise(pred, self.meas, normals(), self.cell, weight, shrink, self.table, clamp=clamp)
        else:
            if self.mode == 'tile':
                pred = ops.tile_project(pred, self.meas, self.cell, self.table, weight, clamp=clamp)
            elif self.mode == 'slab':
                pred = ops.slab_project(pred, self.meas, self.cell, self.table, weight, clamp=clamp)
            elif self.mode == 'band':
                pred = ops.band_project(pred, self.meas, self.cell, self.table, weight, clamp=clamp)
            elif self.mode == 'profile':
                pred = ops.cell_project_profile(pred, self.meas, self.cell, self.table, weight, clamp=clamp)
            else:
                pred = ops.cell_project(pred, self.meas, self.cell, weight, clamp=clamp)
            eps = normals()
        return pred, eps, NO_CLAMP

    def joint_step(self, i, head, x0_prev, form, row, tail, seed, draw, sample, io):
        """Step ``i`` of a joint chain: the fused launch of its rung in the place of the family's plain one -- ``head`` = (y, slot,
        taps, x_t), ``tail`` = (lo, hi, clamp_mode, stride) and ``io`` = dict(out=, x0_out=) as every joint step takes them, ``form``
        0 / 1 / 2 the update of ``ops.volume_joint_step`` / ``_multistep`` / ``_multistep_sde`` and ``row`` its coefficients (kx, k0,
        kn), (kx, k0, kp) or (kx, k0, kp, kn).  The slab takes two calls, the band three.  False on a plain rung: nothing was launched."""
        ops, (rung, weight, shrink) = self.launch, self.steps[i]        # ``ops``: the calling module's from here on
        if rung == 'plain':
            return False
        kx, k0, k2, k3 = (*row, 0.)[:4]
        update = (form, kx, k0, 0. if form == 0 else k2, k2 if form == 0 else k3, *tail, seed)
        key = dict(draw=draw, sample=sample, **io)
        if rung == 'noise' and self.mode == 'tile':
            ops.volume_joint_consistent_tile_noise_step(*head, x0_prev, self.meas, self.cell, self.tables[i], *update, **key)
        elif rung == 'noise':
            ops.volume_joint_consistent_noise_step(*head, x0_prev, self.meas, self.cell, self.table, weight, shrink, *update, **key)
        elif self.mode == 'slab':                            # the solve runs along the whole depth: the coefficients, then the step
            ops.volume_joint_slab_coeffs(*head[:3], self.meas, self.cell, self.table, *self.slab, *tail)
            ops.volume_joint_consistent_slab_step(*head, x0_prev, self.cell, self.table, *self.slab, weight, *update, **key)
        elif self.mode == 'band':                            # the projector runs over the whole volume: residual, P, then the step
            ws = self.band_ws
            ops.volume_joint_band_residual(*head[:3], self.meas, self.table, ws, *tail)
            ops.band_apply(ws[2], self.table, ws[3], ws[4])
            ops.volume_joint_consistent_band_step(*head, x0_prev, self.cell, self.table, ws, weight, *update, **key)
        elif self.mode == 'cell':
            ops.volume_joint_consistent_step(*head, x0_prev, self.meas, self.cell, weight, *update, **key)
        else:                                                # the profile's table or the operator's projector
            step = ops.volume_joint_consistent_tile_step if self.mode == 'tile' else ops.volume_joint_consistent_profile_step
            step(*head, x0_prev, self.meas, self.cell, self.table, weight, *update, **key)
        return True

    def joint_heun(self, i, phase, head, coefs, kc, tail, seed, draw, sample):
        """Phase ``phase`` (1: predictor, 2: corrector and the next churn) of step ``i`` of a joint Heun chain: the fused launch
        ``ops.volume_joint_consistent_heun`` in the place of ``ops.volume_joint_heun`` -- ``head`` = (y, slot, taps, xh, xn, x0),
        ``coefs``, ``kc`` and ``tail`` = (lo, hi, clamp_mode, stride) as that launch takes them.  False where this phase is not
        projected (phase 2 under ``consistency_heun='predictor'``): nothing was launched."""
        ops, (rung, weight, _) = self.launch, self.steps[i]             # ``ops``: the calling module's from here on
        if rung == 'plain' or (phase == 2 and self.heun == 'predictor'):
            return False
        ops.volume_joint_consistent_heun(*head, self.meas, self.cell, self.table, weight, phase, coefs, kc, *tail, seed, draw=draw,
                                         sample=sample, mode=self.mode)
        return True
