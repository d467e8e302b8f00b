"""The adaptive sampler's noise as the preview denoiser's noise source (pt_denoise_set_adaptive_noise) restated in
numpy float32: stage A, which forms pass 0's variance var_0 from the per-pixel estimate e and the tile records of a live adaptive state,
blended with stage V's spatial estimate V0, and the filter that reads it.

The conventions are those of denoise_moments_reference.py, which this file builds on and edits nothing of: every operation is one IEEE
binary32 operation on float32 arrays, in the order the definition gives, nothing fused, selects are np.where on ids and counts only
(never on a value), `/` is the correctly rounded quotient, one vectorised shift per window cell, accumulated in window order (dy outer,
dx inner).  Stage V and the passes are those of denoise_variance_reference.py / denoise_lens_reference.py.
csrc/pt_denoise_adaptive.hip (pt_adaptive_blend_kernel) must reproduce `blend` bit for bit (tests/test_gpu_denoise_adaptive.py);
tests/test_denoise_adaptive_cpu.py checks the properties of the restatement itself.
"""
from __future__ import annotations

import numpy as np

import denoise_reference as dr
import denoise_variance_reference as dv
import denoise_lens_reference as dl

F = dr.F
DEFAULT_PRIOR_SAMPLES = 8


def pixel_counts(tiles: np.ndarray, shape) -> tuple:
    """(k, k - k0) of every pixel's own 8x8 tile (x >> 3, y >> 3) as (H, W) int32 arrays; tiles: (ceil(H / 8), ceil(W / 8)) records
    with the fields k and k0 (adaptive_reference.TILE_DTYPE, PathTracer.AdaptiveTiles)."""
    H, W = shape
    assert tiles.shape == ((H + 7) // 8, (W + 7) // 8), (tiles.shape, shape)
    def up(a):
        return np.repeat(np.repeat(np.asarray(a, np.int32), 8, 0), 8, 1)[:H, :W]
    k = up(tiles["k"])
    return k, k - up(tiles["k0"])


def per_sample(e: np.ndarray, tiles: np.ndarray) -> np.ndarray:
    """e(q) kf_q: one multiply with the count of q's own tile — q's per-sample variance of u."""
    k, _ = pixel_counts(tiles, e.shape)
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(e, dtype=F) * k.astype(F)).astype(F)


def window_mean(x: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """S: the sum of x over the cells of the 3x3 window that lie inside the image and have the centre's id, divided by their number."""
    H, W = ids.shape
    s, cnt = np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            sh = dv._shift(H, W, dy, dx)
            if sh is None:
                continue
            P, Q = sh
            visit = ids[Q] == ids[P]
            with np.errstate(all="ignore"):
                s[P] = np.where(visit, s[P] + x[Q], s[P])
            cnt[P] = np.where(visit, cnt[P] + F(1.0), cnt[P])
    with np.errstate(all="ignore"):
        return (s / cnt).astype(F)


def blend(e: np.ndarray, tiles: np.ndarray, v0: np.ndarray, ids: np.ndarray, prior_samples: int = DEFAULT_PRIOR_SAMPLES) -> np.ndarray:
    """Stage A: var_0 = ((jf Et) + (K0 V0)) / (jf + K0), Et = S / kf_p, S = window_mean(e kf); V0 where id = -1 or k - k0 <= 0."""
    k, j = pixel_counts(tiles, ids.shape)
    kf, jf, k0 = k.astype(F), j.astype(F), F(prior_samples)
    v0 = np.ascontiguousarray(v0, dtype=F)
    S = window_mean(per_sample(e, tiles), ids)
    with np.errstate(all="ignore"):
        et = S / kf
        var0 = ((jf * et) + (k0 * v0)) / (jf + k0)
    return np.where((ids != -1) & (j > 0), var0, v0).astype(F)


def denoise(colour, guides, e, tiles, params: dr.Params = dr.Params(), sigma_variance=dv.DEFAULT_SIGMA_VARIANCE,
            prior_samples: int = DEFAULT_PRIOR_SAMPLES, cocK=0.0, focal=0.0, var0=None):
    """PT_DENOISE_VARIANCE with the switch on, on a live adaptive state whose per-pixel estimate is e and whose records are tiles ->
    (image (H, W, 4), V0, var_0); iterations = 0: (a copy, None, None).  cocK > 0: the passes of the lens mode.  var0 given: the passes
    on that var_0 (what a read-out of the handle returned) instead of on blend's."""
    assert colour.dtype == np.float32 and colour.shape == guides.shape + (4,)
    if params.iterations == 0:
        return colour.copy(), None, None
    v0 = dv.estimate(colour, guides)
    if var0 is None:
        var0 = blend(e, tiles, v0, guides["id"], prior_samples)
    out, var = colour, var0
    for i in range(params.iterations):
        out, var = dl.lens_pass(out, var, guides, i, params, sigma_variance, cocK, focal)
    return out, v0, var0
