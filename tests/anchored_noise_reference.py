"""Specification of the volume-anchored noise of ``diffusioniqt_amd.ops.anchored_noise`` and of the few-step sampler of
``Imagen.p_sample_loop(sampler='ddim')`` in plain numpy: Philox4x32-10 on uint64 arrays, the raw field of a whole volume, the
Box-Muller normals in float64 from those bits, the DDIM coefficients in float64 and the sampling loop in float64.  Not a test module:
the host and GPU tests of both features import it.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Random123 philox.h: PHILOX_M4x32_0 / _1
W0, W1 = 0x9E3779B9, 0xBB67AE85            # PHILOX_W32_0 / _1
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or scalars) of 32-bit words, key: 2.  Returns the 4 output words as uint64 arrays holding 32-bit values.
    One round: (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped by the Weyl
    constants between rounds."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]              # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def field_at(lin, seed, draw, sample):
    """The two words (r0, r1) used at the linear voxel indices ``lin`` (uint64 array): [..., 2] uint32."""
    lin = np.asarray(lin, dtype=np.uint64)
    r = philox4x32_10((lin & MASK, lin >> np.uint64(32), draw, sample), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack((r[0], r[1]), axis=-1).astype(np.uint32)


def field(volume_shape, C, seed, draw, sample):
    """Raw bits of the whole field: uint32 [C, D, H, W, 2] with lin = ((c D + z) H + y) W + x."""
    D, H, W = volume_shape
    lin = np.arange(C * D * H * W, dtype=np.uint64).reshape(C, D, H, W)
    return field_at(lin, seed, draw, sample)


def window_lin(volume_shape, origin, P, C=1):
    """Linear indices [C, P, P, P] of the window at ``origin`` -- also for volumes too large to enumerate."""
    D, H, W = (np.uint64(v) for v in volume_shape)
    c = np.arange(C, dtype=np.uint64)[:, None, None, None]
    z = (np.uint64(origin[0]) + np.arange(P, dtype=np.uint64))[None, :, None, None]
    y = (np.uint64(origin[1]) + np.arange(P, dtype=np.uint64))[None, None, :, None]
    x = (np.uint64(origin[2]) + np.arange(P, dtype=np.uint64))[None, None, None, :]
    return ((c * D + z) * H + y) * W + x


def window(bits_or_normals, origin, P):
    """[C, P, P, P, ...] cut of a [C, D, H, W, ...] field."""
    z, y, x = origin
    return bits_or_normals[:, z:z + P, y:y + P, x:x + P]


def normals(bits):
    """Box-Muller in float64 on the bits [..., 2]: u1 = ((r0 >> 9) + 0.5) 2^-23, u2 = (r1 >> 8) 2^-24, n = sqrt(-2 ln u1) cos(2 pi u2)."""
    r0, r1 = bits[..., 0].astype(np.uint64), bits[..., 1].astype(np.uint64)
    u1 = ((r0 >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (r1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# ---- the sampler -------------------------------------------------------------------------------------------------------------------
def alpha_sigma64(log_snr):
    ls = np.asarray(log_snr, dtype=np.float64)
    return np.sqrt(1.0 / (1.0 + np.exp(-ls))), np.sqrt(1.0 / (1.0 + np.exp(ls)))


def ddim_coefficients64(log_snr, log_snr_next, last, eta):
    """The closed form in float64 on the (fp32) log-SNR values of a step: x_next = kx x_t + k0 x0 + kn noise."""
    ls, lsn = np.asarray(log_snr, dtype=np.float64), np.asarray(log_snr_next, dtype=np.float64)
    alpha, sigma = alpha_sigma64(ls)
    alpha_next, sigma_next = alpha_sigma64(lsn)
    c = -np.expm1(ls - lsn)
    s = eta * np.sqrt(sigma_next ** 2 * c)
    kx = np.sqrt(np.maximum(sigma_next ** 2 - s ** 2, 0.0)) / sigma
    k0 = alpha_next - kx * alpha
    kn = s * (1.0 - np.asarray(last, dtype=np.float64))
    return kx, k0, kn


def ddim_reference_loop(net, init, step_noise, coefs, x0_coefs, log_snr, objective, lo, hi=None, dyn_q=None, dyn_floor=None):
    """The sampling loop in float64.  ``net(x, log_snr_row)`` is the network in float64; ``init`` [B, ...] the initial image;
    ``step_noise`` a list of per-step draws (ignored where kn == 0; may be shorter than the chain then); ``coefs`` [T, 3, B] and
    ``x0_coefs`` [T, 2, B] the per-step (kx, k0, kn) and the (a, b) of x0 = a x + b pred, as the device holds them (fp32, widened);
    ``log_snr`` [T, B] the fp32 conditioning.  Static clamp: x0 = max(x0, lo), or clip(x0, lo, hi) when ``hi`` is given.  Dynamic thresholding (``dyn_q`` set):
    s = max(quantile(|x0|, dyn_q) per batch row, dyn_floor), x0 = clip(x0, -s, s) / s, no static clamp in the step.
    Returns (final image, [x after each step] + [last again], [x0 of each step] + [last again]) like ``Imagen.sample``."""
    x = np.asarray(init, dtype=np.float64)
    B = x.shape[0]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape((B,) + (1,) * (x.ndim - 1))
    clamp = (lambda v: np.maximum(v, lo)) if hi is None else (lambda v: np.clip(v, lo, hi))
    noisy, x0s = [], []
    x0 = None
    for i in range(coefs.shape[0]):
        pred = net(x, np.asarray(log_snr[i], dtype=np.float64))
        if objective != 'x_start':
            pred = col(x0_coefs[i, 0]) * x + col(x0_coefs[i, 1]) * pred
        if dyn_q is not None:
            # torch.quantile's rank arithmetic is fp32 (aten quantile_compute), as ops.abs_quantile reproduces it
            flat = np.sort(np.abs(pred).reshape(B, -1), axis=1)
            rank = np.float32(dyn_q) * np.float32(flat.shape[1] - 1)
            k = int(np.floor(rank))
            w = np.float64(np.float32(rank - np.float32(k)))
            s = flat[:, k] + w * (flat[:, min(k + 1, flat.shape[1] - 1)] - flat[:, k])
            s = col(np.maximum(s, dyn_floor))
            x0 = np.clip(pred, -s, s) / s
        else:
            x0 = clamp(pred)
        kx, k0, kn = (col(coefs[i, j]) for j in range(3))
        x = kx * x + k0 * x0
        if np.any(np.asarray(coefs[i, 2]) != 0):
            x = x + kn * np.asarray(step_noise[i], dtype=np.float64)
        noisy.append(x)
        x0s.append(x0)
    noisy.append(x)
    x0s.append(x0)
    return clamp(x), noisy, x0s


# ---- the stand-in network of the sampler tests -----------------------------------------------------------------------------------------
def stub_net64(x, lowres, log_snr):
    """f(x, lowres, log-SNR) = x / (2 (1 + |x|)) + lowres / 4 + log-SNR / 64 per batch row: elementwise, Lipschitz constant 1/2 in x, and
    built from operations that fp32 rounds correctly (one division, three additions; the scalings are powers of two), so what the sampler
    test measures is the sampler's own round-off."""
    x = np.asarray(x, dtype=np.float64)
    ls = np.asarray(log_snr, dtype=np.float64).reshape((x.shape[0],) + (1,) * (x.ndim - 1))
    return 0.5 * (x / (1.0 + np.abs(x))) + 0.25 * np.asarray(lowres, dtype=np.float64) + 0.015625 * ls


def make_stub_unet():
    """``stub_net64`` as the module ``Imagen`` samples from: the attributes the sampling loop reads and ``forward_with_cond_scale``."""
    import torch

    class StubUnet(torch.nn.Module):
        lowres_cond = True
        self_cond = False

        def cast_model_parameters(self, **kwargs):
            return self

        def forward_with_cond_scale(self, x, time_steps, log_snr, *, lowres_cond_img=None, **kwargs):
            return 0.5 * (x / (1.0 + x.abs())) + 0.25 * lowres_cond_img + 0.015625 * log_snr.view(-1, 1, 1, 1, 1)

    return StubUnet()
