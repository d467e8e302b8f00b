"""The lens mode of the preview denoiser (pt_denoise_set_lens) restated in numpy float32: the blur radius of a
pixel, the relaxed-tap rule, and the passes of both filter modes under it.

The conventions are those of denoise_reference.py and denoise_variance_reference.py, which this file builds on and edits neither: every
operation is one IEEE binary32 operation on float32 arrays, in the order the definition gives, nothing fused, selects are np.where (every
comparison is False for NaN), `/` is the correctly rounded quotient, one vectorised shift per tap, accumulated in tap order (dy outer,
dx inner).  u, the taps, the kernel h, w_n, w_z and the luminance stop of each mode are theirs; what is added: c(p), the rule that takes
a tap on the luminance stop alone, and the host's cocK.  With cocK = 0 the passes are theirs bit for bit.  csrc/pt_denoise.hip
(pt_atrous_kernel<S, VARIANCE, true>, pt_guides_ray_kernel<true>) must reproduce this bit for bit (tests/test_gpu_denoise_lens.py);
tests/test_denoise_lens_cpu.py checks the properties of the restatement itself.
"""
from __future__ import annotations

import math

import numpy as np

import denoise_reference as dr
import denoise_variance_reference as dv

F = dr.F
DEFAULT_COC_SCALE = 1.0


def cock_of(coc_scale: float, aperture: float, focal: float, height: int, inv_proj5: float) -> np.float32:
    """cocK = coc_scale (A / 2) / F H / (2 |invProj[5]|), evaluated left to right in double from the binary32 inputs and rounded once, as
    the host computes the kernel argument; 0 when A <= 0, F <= 0, coc_scale = 0 or the result is not finite."""
    s, A, Fl, m5 = float(F(coc_scale)), float(F(aperture)), float(F(focal)), float(F(inv_proj5))
    if not A > 0.0 or not Fl > 0.0 or s == 0.0:
        return F(0.0)
    den = 2.0 * abs(m5)
    if den == 0.0:
        return F(0.0)  # (the quotient is inf or NaN)
    with np.errstate(all="ignore"):
        k = F(s * (A / 2.0) / Fl * float(height) / den)
    return k if np.isfinite(k) else F(0.0)


def coc_radius(guides: np.ndarray, cocK, focal) -> np.ndarray:
    """c (H, W) float32: (cocK * |t - F|) / t on a hit — one subtract, one abs, one multiply, one divide — and cocK on a miss (id -1)."""
    t = guides["t"]
    with np.errstate(all="ignore"):
        c = (F(cocK) * np.abs(t - F(focal))) / t
    return np.where(guides["id"] == -1, F(cocK), c).astype(F)


def relaxed_rule(r, cP, cQ, match, cocK, s, dx, dy):
    """-> (relaxed, use) of one tap shift: relaxed iff cocK > 0, r <= c(p) and r <= c(q), with r = s max(|dx|, |dy|) (handed in as a
    float32 scalar; s, dx, dy are for the test's edited rules); a tap is used when it is relaxed or its id matches."""
    with np.errstate(all="ignore"):
        relaxed = bool(F(cocK) > 0) & (r <= cP) & (r <= cQ)
    return relaxed, relaxed | match


def new_stats():
    """Counters a pass adds to, over the in-image taps of centres with id != -1: taps, relaxed ones, relaxed ones that cross an id."""
    return {"taps": 0, "relaxed": 0, "crossing": 0}


def lens_pass(colour, var, guides, i, p: dr.Params, sigma_variance, cocK, focal, rule=relaxed_rule, stats=None):
    """Pass i (step 2^i) under the lens rule.  var None: the fixed mode (dr.atrous_pass) -> (colour (H, W, 4) alpha 1, None); else the
    variance mode (dv.variance_pass) -> (colour, variance)."""
    variance = var is not None
    H, W = guides.shape
    st = 1 << i
    rgb = np.ascontiguousarray(colour[..., :3], dtype=F)
    ids, pos, nrm, t = guides["id"], guides["pos"], guides["normal"], guides["t"]
    u = dr.u_of(rgb)
    c = coc_radius(guides, cocK, focal)
    centre = ids != -1
    Wsum, S, Qsum = np.zeros((H, W), F), np.zeros((H, W, 3), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        den = F(p.sigma_plane) * t
        if variance:
            var = np.ascontiguousarray(var, dtype=F)
            inv = F(1.0) / (dv.k2_of(sigma_variance) * var + dv.EPS)
        else:
            isig = dr.inv_sigma(p.sigma_color, i)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sh = dv._shift(H, W, st * dy, st * dx)
                if sh is None:
                    continue
                P, Q = sh
                h = dr.KERNEL[abs(dx)] * dr.KERNEL[abs(dy)]
                d = dr._dot(nrm[P], nrm[Q])
                wn = np.where(d > 0, d, F(0.0))
                for _ in range(p.normal_log2_power):
                    wn = wn * wn
                e = dr._dot(nrm[P], pos[Q] - pos[P])
                q = e / den[P]
                z = F(1.0) - q * q
                wz = np.where(z > 0, z, F(0.0))
                if variance:
                    du = u[Q] - u[P]
                    cc = F(1.0) - (du * du) * inv[P]
                else:
                    a = (u[Q] - u[P]) * isig
                    cc = F(1.0) - a * a
                cc = np.where(cc > 0, cc, F(0.0))
                wc = cc * cc
                match = ids[Q] == ids[P]
                r = F(st * max(abs(dx), abs(dy)))
                relaxed, use = rule(r, c[P], c[Q], match, cocK, st, dx, dy)
                w = np.where(relaxed, h * wc, ((h * wn) * wz) * wc)
                Wsum[P] = np.where(use, Wsum[P] + w, Wsum[P])
                S[P] = np.where(use[..., None], S[P] + w[..., None] * rgb[Q], S[P])
                if variance:
                    Qsum[P] = np.where(use, Qsum[P] + (w * w) * var[Q], Qsum[P])
                if stats is not None:
                    stats["taps"] += int(centre[P].sum())
                    stats["relaxed"] += int((relaxed & centre[P]).sum())
                    stats["crossing"] += int((relaxed & ~match & centre[P]).sum())
        out = np.empty((H, W, 4), F)
        ok = (Wsum > 0) & centre
        out[..., :3] = np.where(ok[..., None], S / Wsum[..., None], rgb)
        var_out = np.where(ok, Qsum / (Wsum * Wsum), var).astype(F) if variance else None
    out[..., 3] = F(1.0)
    return out, var_out


def denoise(colour, guides, params: dr.Params = dr.Params(), sigma_variance=None, cocK=0.0, focal=0.0, rule=relaxed_rule, stats=None):
    """colour (H, W, 4) float32 (RGB is read), guides (H, W) GUIDE_DTYPE, sigma_variance None: PT_DENOISE_FIXED -> (image, V0 or None),
    as dr.denoise / dv.denoise return them.  Stage V is dv.estimate, unchanged."""
    assert colour.dtype == np.float32 and colour.shape == guides.shape + (4,)
    if params.iterations == 0:
        return colour.copy(), None
    v0 = dv.estimate(colour, guides) if sigma_variance is not None else None
    out, var = colour, v0
    for i in range(params.iterations):
        out, var = lens_pass(out, var, guides, i, params, sigma_variance, cocK, focal, rule, stats)
    return out, v0


def guides_from_records(records: np.ndarray, normals: np.ndarray) -> np.ndarray:
    """The guide records of first-hit records (FIRST_HIT_DTYPE) of the same ray: P = dir * t + origin in two roundings per component,
    id and t as they are, the normal handed in (the query has none); a miss: id -1, t +inf, P = N = 0."""
    g = np.zeros(records.shape, dr.GUIDE_DTYPE)
    hit = records["id"] >= 0
    with np.errstate(all="ignore"):
        pos = records["dir"] * records["t"][..., None] + records["origin"]
    g["pos"] = np.where(hit[..., None], pos, F(0.0))
    g["normal"] = np.where(hit[..., None], normals, F(0.0))
    g["id"], g["t"] = records["id"], records["t"]
    return g
