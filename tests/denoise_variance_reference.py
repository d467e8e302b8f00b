"""The variance-guided mode of the preview denoiser (PT_DENOISE_VARIANCE) restated in numpy float32:
(colour, guides, params, sigma_variance) -> (image, V0).

The conventions are those of denoise_reference.py, which this file builds on and does not edit: every operation is one IEEE binary32
operation on float32 arrays, in the order the definition gives, nothing fused, selects are np.where (NaN > 0 is False), one vectorised
shift per tap, accumulated in tap order (dy outer, dx inner).  u, the guides, the taps, the kernel h, the id rule, w_n and w_z are
denoise_reference's; only the luminance stop differs, and the variance it is scaled by is estimated (stage V) and filtered here.
csrc/pt_denoise.hip (pt_variance_kernel, pt_atrous_kernel<S, true>) must reproduce this bit for bit (tests/test_gpu_denoise_variance.py);
tests/test_denoise_variance_cpu.py checks the properties of the restatement itself.
"""
from __future__ import annotations

import numpy as np

import denoise_reference as dr

F = dr.F
EPS = F(1e-8)
DEFAULT_SIGMA_VARIANCE = 6.0


def k2_of(sigma_variance: float) -> np.float32:
    """sigma_variance * sigma_variance in binary32, as the host computes the kernel argument."""
    with np.errstate(all="ignore"):  # (the square may overflow to inf or underflow to 0, by IEEE and without a warning)
        return F(sigma_variance) * F(sigma_variance)


def _shift(H, W, oy, ox):
    """Slices (P, Q) of the centres p whose q = p + (ox, oy) lies inside the image, or None."""
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def estimate(rgb: np.ndarray, guides: np.ndarray) -> np.ndarray:
    """Stage V: V0 (H, W) float32 from the image's RGB (rgb[..., :3] is read) and the guides' ids."""
    H, W = guides.shape
    ids = guides["id"]
    u = dr.u_of(np.ascontiguousarray(rgb[..., :3], dtype=F))
    with np.errstate(all="ignore"):
        # Dx(q) = (u(q + (1, 0)) - u(q))^2, valid when q + (1, 0) lies inside the image and has q's id; Dy the same with (0, 1)
        Dx, Dy = np.zeros((H, W), F), np.zeros((H, W), F)
        vx, vy = np.zeros((H, W), bool), np.zeros((H, W), bool)
        ex = u[:, 1:] - u[:, :-1]
        Dx[:, :-1] = ex * ex
        vx[:, :-1] = ids[:, 1:] == ids[:, :-1]
        ey = u[1:, :] - u[:-1, :]
        Dy[:-1, :] = ey * ey
        vy[:-1, :] = ids[1:, :] == ids[:-1, :]
        n = np.zeros((H, W), F)
        s = np.zeros((H, W), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                sh = _shift(H, W, dy, dx)
                if sh is None:
                    continue
                P, Q = sh
                visit = ids[Q] == ids[P]
                ok = visit & vx[Q]
                n[P] = np.where(ok, n[P] + F(1.0), n[P])
                s[P] = np.where(ok, s[P] + Dx[Q], s[P])
                ok = visit & vy[Q]
                n[P] = np.where(ok, n[P] + F(1.0), n[P])
                s[P] = np.where(ok, s[P] + Dy[Q], s[P])
        v0 = np.where((n > 0) & (ids != -1), F(0.5) * (s / n), F(0.0))
    return v0.astype(F)


def variance_pass(colour: np.ndarray, var: np.ndarray, guides: np.ndarray, i: int, p: dr.Params, sigma_variance: float):
    """Pass i (step 2^i) over colour (H, W, 4) float32 (RGB is read) and its variance var (H, W) float32 ->
    (colour (H, W, 4) with alpha = 1, variance (H, W)).  p.sigma_color is not read."""
    H, W = guides.shape
    st = 1 << i
    rgb = np.ascontiguousarray(colour[..., :3], dtype=F)
    var = np.ascontiguousarray(var, dtype=F)
    ids, pos, nrm, t = guides["id"], guides["pos"], guides["normal"], guides["t"]
    u = dr.u_of(rgb)
    k2 = k2_of(sigma_variance)
    with np.errstate(all="ignore"):  # (sigma_plane near FLT_MAX: the product is inf, by IEEE and without a warning)
        den = F(p.sigma_plane) * t
    Wsum = np.zeros((H, W), F)
    S = np.zeros((H, W, 3), F)
    Qsum = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        inv = F(1.0) / (k2 * var + EPS)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sh = _shift(H, W, st * dy, st * dx)
                if sh is None:
                    continue
                P, Q = sh
                h = dr.KERNEL[abs(dx)] * dr.KERNEL[abs(dy)]
                d = dr._dot(nrm[P], nrm[Q])
                wn = np.where(d > 0, d, F(0.0))
                for _ in range(p.normal_log2_power):
                    wn = wn * wn
                e = dr._dot(nrm[P], pos[Q] - pos[P])
                r = e / den[P]
                z = F(1.0) - r * r
                wz = np.where(z > 0, z, F(0.0))
                du = u[Q] - u[P]
                a2 = (du * du) * inv[P]
                c = F(1.0) - a2
                c = np.where(c > 0, c, F(0.0))
                wc = c * c
                w = ((h * wn) * wz) * wc
                match = ids[Q] == ids[P]
                Wsum[P] = np.where(match, Wsum[P] + w, Wsum[P])
                S[P] = np.where(match[..., None], S[P] + w[..., None] * rgb[Q], S[P])
                Qsum[P] = np.where(match, Qsum[P] + (w * w) * var[Q], Qsum[P])
        out = np.empty((H, W, 4), F)
        ok = (Wsum > 0) & (ids != -1)
        out[..., :3] = np.where(ok[..., None], S / Wsum[..., None], rgb)
        var_out = np.where(ok, Qsum / (Wsum * Wsum), var).astype(F)
    out[..., 3] = F(1.0)
    return out, var_out


def denoise(colour: np.ndarray, guides: np.ndarray, params: dr.Params = dr.Params(), sigma_variance: float = DEFAULT_SIGMA_VARIANCE):
    """colour (H, W, 4) float32 (the accumulation image; RGB is read), guides (H, W) GUIDE_DTYPE -> (image (H, W, 4) float32, V0 (H, W)
    float32).  iterations = 0: the input itself, and V0 = None (no estimate is made for a copy)."""
    assert colour.dtype == np.float32 and colour.shape == guides.shape + (4,)
    if params.iterations == 0:
        return colour.copy(), None
    v0 = estimate(colour, guides)
    out, var = colour, v0
    for i in range(params.iterations):
        out, var = variance_pass(out, var, guides, i, params, sigma_variance)
    return out, v0
