"""The temporal moments of the preview denoiser (pt_denoise_set_moments) restated in numpy float32: the moment
set and its observations (stage M), the noise map Vm, the blend with the spatial estimate (stage B), the filter that reads it, and the
noise level.

The conventions are those of denoise_reference.py, denoise_variance_reference.py and denoise_lens_reference.py, which this file builds on
and edits none of: every operation is one IEEE binary32 operation on float32 arrays, in the order the definition gives, nothing fused,
selects are np.where (every comparison is False for NaN, so NaN goes to 0), `/` is the correctly rounded quotient, one vectorised shift
per window cell, accumulated in window order (dy outer, dx inner).  u, stage V and the passes are theirs; what is added: the luminance
l of u's definition on its own, the weighted Welford update of (lprev, M2), Vm, Vt and var_0.  csrc/pt_denoise_moments.hip
(pt_moments_kernel, pt_moments_blend_kernel, pt_moments_level_kernel) must reproduce stages M and B bit for bit
(tests/test_gpu_denoise_moments.py); tests/test_denoise_moments_cpu.py checks the properties of the restatement itself.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import denoise_reference as dr
import denoise_variance_reference as dv
import denoise_lens_reference as dl

F = dr.F
DEFAULT_PRIOR_SAMPLES = 32


def luminance(rgb: np.ndarray) -> np.ndarray:
    """l = 0.2126 r + 0.7152 g + 0.0722 b evaluated left to right: the luminance of u's definition (dr.u_of)."""
    with np.errstate(all="ignore"):
        return ((F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]).astype(F)


@dataclass(frozen=True)
class MomentSet:
    """What the handle keeps: per pixel lprev and M2 (None while K = 0), per handle the observation count K, the sample count nPrev of
    the last observation, and the spp and reset epoch it was made under."""
    lprev: np.ndarray | None = None
    M2: np.ndarray | None = None
    K: int = 0
    nPrev: int = 0
    spp: int = 1
    epoch: int = 0


def observe(ms: MomentSet, colour: np.ndarray, n: int, spp: int = 1, epoch: int = 0) -> MomentSet:
    """Stage M's state update for a look at colour (H, W, >= 3) float32 (RGB is read) holding n = frame index * spp samples.  The set is
    forgotten first when the epoch or spp differs or n < nPrev; n = 0, or n = nPrev with K > 0, is no observation."""
    if ms.K > 0 and (ms.epoch != epoch or ms.spp != spp or n < ms.nPrev):
        ms = MomentSet()
    if n == 0 or (ms.K > 0 and n == ms.nPrev):
        return ms
    l = luminance(np.ascontiguousarray(colour[..., :3], dtype=F))
    if ms.K == 0:
        M2 = np.zeros(l.shape, F)
    else:
        nf, npf, w = F(n), F(ms.nPrev), F(n - ms.nPrev)  # (converted by the host)
        with np.errstate(all="ignore"):
            b = (nf * l - npf * ms.lprev) / w
            M2 = ms.M2 + (w * (b - ms.lprev)) * (b - l)
    return MomentSet(l, M2.astype(F), ms.K + 1, n, spp, epoch)


def noise(ms: MomentSet, colour: np.ndarray, ids: np.ndarray, n: int) -> np.ndarray:
    """Vm (H, W) float32 of the image as it stands (colour holds n samples; ms counts this look): 0 where id = -1 or K < 2."""
    if ms.K < 2:
        return np.zeros(ids.shape, F)
    l = luminance(np.ascontiguousarray(colour[..., :3], dtype=F))
    with np.errstate(all="ignore"):
        s2 = ms.M2 / F(ms.K - 1)
        vl = s2 / F(n)
        g = F(1.0) / (F(1.0) + l)
        g2 = g * g
        v = (vl * g2) * g2
        v = np.where(v > 0, v, F(0.0))
    return np.where(ids != -1, v, F(0.0)).astype(F)


def window_mean(vm: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """Vt: the sum of Vm over the cells of the 3x3 window that lie inside the image and have the centre's id, divided by their number."""
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
                s[P] = np.where(visit, s[P] + vm[Q], s[P])
            cnt[P] = np.where(visit, cnt[P] + F(1.0), cnt[P])
    with np.errstate(all="ignore"):
        return (s / cnt).astype(F)


def blend(vm: np.ndarray, v0: np.ndarray, ids: np.ndarray, K: int, prior_samples: int = DEFAULT_PRIOR_SAMPLES) -> np.ndarray:
    """Stage B: var_0 = ((Km1 Vt) + (K0 V0)) / (Km1 + K0); V0 where id = -1.  With K < 2 the stage does not run: V0 itself."""
    if K < 2:
        return v0
    km1, k0 = F(K - 1), F(prior_samples)
    vt = window_mean(np.ascontiguousarray(vm, dtype=F), ids)
    with np.errstate(all="ignore"):
        var0 = ((km1 * vt) + (k0 * v0)) / (km1 + k0)
    return np.where(ids != -1, var0, v0).astype(F)


def denoise(colour, guides, ms: MomentSet, n: int, params: dr.Params = dr.Params(), sigma_variance=dv.DEFAULT_SIGMA_VARIANCE,
            prior_samples: int = DEFAULT_PRIOR_SAMPLES, cocK=0.0, focal=0.0):
    """PT_DENOISE_VARIANCE with the switch on and the temporal stage off, ms counting this look at colour (n samples) ->
    (image (H, W, 4), V0, Vm, var_0); iterations = 0: (a copy, None, Vm, None).  cocK > 0: the passes of the lens mode."""
    assert colour.dtype == np.float32 and colour.shape == guides.shape + (4,)
    ids = guides["id"]
    vm = noise(ms, colour, ids, n)
    if params.iterations == 0:
        return colour.copy(), None, vm, None
    v0 = dv.estimate(colour, guides)
    var0 = blend(vm, v0, ids, ms.K, prior_samples)
    out, var = colour, var0
    for i in range(params.iterations):
        out, var = dl.lens_pass(out, var, guides, i, params, sigma_variance, cocK, focal)
    return out, v0, vm, var0


def noise_level(vm: np.ndarray, ids: np.ndarray):
    """pt_denoise_noise_level: one binary32 partial sum of Vm over the pixels with id >= 0 and one count per 256 consecutive pixels (rows
    like the image), summed in index order in double -> (mean as float32, pixel count).  The order of the additions inside a partial
    sum is the device's; any order is within a relative 255 * 2^-24 of the exact sum, the terms being non-negative."""
    hit = (ids >= 0).ravel()
    v = np.where(hit, vm.ravel(), F(0.0)).astype(F)
    pad = (-v.size) % 256
    v = np.concatenate([v, np.zeros(pad, F)]).reshape(-1, 256)
    total = 0.0
    for part in v.sum(axis=1, dtype=F):
        total += float(part)
    count = int(hit.sum())
    return (F(total / count) if count else F(0.0)), count
