"""The rebuild of an adaptive state (pt_adaptive_write_state; pt_adaptive_rebuild_kernel in csrc/pt_adaptive_state.hip; DESIGN.md section
3.5) restated in numpy float32 on top of tests/adaptive_reference.py: from the image, the per-pixel M2 and the tiles' (k, k0, n) the
per-pixel estimate e (step 4 of the sampler's definition with k' = k) and the tiles' err (step 5) — and the levelling of pt_adaptive_end
as parameters of the sampler's own passes.
Used by tests/test_adaptive_state_cpu.py (against the tabulated states) and tests/test_gpu_adaptive_state.py (the kernel against it)."""
from __future__ import annotations

import numpy as np

import adaptive_reference as ar

F32 = np.float32
END_PARAMS = (F32(0.0), 65535)  # pt_adaptive_end: threshold 0, min_samples 65535, max_samples = the largest count


def pixel_counts(k: np.ndarray, rows: int, width: int) -> np.ndarray:
    return np.repeat(np.repeat(np.asarray(k), 8, 0), 8, 1)[:rows, :width]


def rebuild(image, m2, k, k0):
    """-> (e (rows, width), err (tilesY, tilesX)).  image (rows, width, 4), m2 (rows, width), k (tilesY, tilesX) int, k0 int.
    Per tile: j = k - k0; j >= 1 ? e = clamp((M2 / ((float)j (float)k)) / ((s s) (s s))), s = 1 + l(image) : e = 0; then the butterfly and
    err = s_0 / (float)n."""
    image, m2, k = np.asarray(image, F32), np.asarray(m2, F32), np.asarray(k)
    rows, width = m2.shape
    ty, tx = ar.tile_grid(rows, width)
    assert k.shape == (ty, tx) and image.shape == (rows, width, 4)
    l = ar.lum(image)
    e = np.zeros((rows, width), F32)
    for y in range(ty):
        for x in range(tx):
            sl = (slice(8 * y, 8 * y + 8), slice(8 * x, 8 * x + 8))
            e[sl] = ar.pixel_estimate(m2[sl], int(k[y, x]), int(k0), l[sl])
    return e, ar.tile_error(e, ar.tile_pixels(rows, width))


def colour_with_luminance_minus_one() -> np.ndarray:
    """an RGBA colour whose l is -1 bit for bit (s = 0, q = 0 in step 4): (0, g, 0, 1) with g the float32 next to -1 / 0.7152 that does it"""
    g = F32(-1.0) / F32(0.7152)
    for cand in (g, np.nextafter(g, F32(0.0)), np.nextafter(g, F32(-2.0))):
        c = np.array([0.0, cand, 0.0, 1.0], F32)
        if ar.lum(c) == F32(-1.0):
            return c
    raise AssertionError("no float32 g with l((0, g, 0)) == -1")


def level(sim: ar.Sim) -> tuple:
    """pt_adaptive_end on a Sim: kmax - kmin passes under (0, 65535, kmax).  -> (kmax, the passes run)"""
    kmax, kmin = int(sim.k.max()), int(sim.k.min())
    sim.run(kmax - kmin, END_PARAMS[0], END_PARAMS[1], kmax)
    return kmax, kmax - kmin
