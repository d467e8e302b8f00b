"""The preview denoiser's definition restated in numpy float32: (colour, guides, params) -> image.

Every operation is one IEEE binary32 operation on float32 arrays, in the order the definition gives; nothing is fused (numpy has no fused
multiply-add), selects are np.where (NaN > 0 is False: NaN becomes 0).  One vectorised shift per tap, accumulated in tap order (dy outer,
dx inner).  csrc/pt_denoise.hip must reproduce this bit for bit (tests/test_gpu_denoise.py); tests/test_denoise_cpu.py checks the
properties of the restatement itself.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32
GUIDE_DTYPE = np.dtype([("pos", np.float32, 3), ("id", np.int32), ("normal", np.float32, 3), ("t", np.float32)])
KERNEL = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))  # k[|d|], exact in binary32 (and so are the 9 products)


@dataclass(frozen=True)
class Params:
    iterations: int = 5
    sigma_color: float = 0.5
    sigma_plane: float = 0.02
    normal_log2_power: int = 5


def inv_sigma(sigma_color: float, i: int) -> np.float32:
    """1.0f / (sigma_color * 2^-i) in binary32, as the host computes the kernel argument of pass i."""
    with np.errstate(all="ignore"):  # (a subnormal sigma_color gives inf, by IEEE and without a warning)
        return F(1.0) / (F(sigma_color) * F(2.0 ** -i))


def u_of(c: np.ndarray) -> np.ndarray:
    """u = l / (1 + l), l = 0.2126 r + 0.7152 g + 0.0722 b evaluated left to right."""
    with np.errstate(all="ignore"):  # (l may overflow, 1 + l may be 0: the quotient is what IEEE says, and no warning is wanted)
        l = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
        return l / (F(1.0) + l)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def atrous_pass(colour: np.ndarray, guides: np.ndarray, i: int, p: Params) -> np.ndarray:
    """Pass i (step 2^i) over colour (H, W, 4) float32 -> (H, W, 4) float32 with alpha = 1.  Only colour's RGB is read."""
    H, W = guides.shape
    s = 1 << i
    rgb = np.ascontiguousarray(colour[..., :3], dtype=F)
    ids, pos, nrm, t = guides["id"], guides["pos"], guides["normal"], guides["t"]
    u = u_of(rgb)
    isig = inv_sigma(p.sigma_color, i)
    with np.errstate(all="ignore"):  # (sigma_plane near FLT_MAX: the product is inf, by IEEE and without a warning)
        den = F(p.sigma_plane) * t
    Wsum = np.zeros((H, W), F)
    S = np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                # centres p = (y, x) whose tap q = p + (oy, ox) lies inside the image
                y0, y1 = max(0, -oy), min(H, H - oy)
                x0, x1 = max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                h = KERNEL[abs(dx)] * KERNEL[abs(dy)]
                d = _dot(nrm[P], nrm[Q])
                wn = np.where(d > 0, d, F(0.0))
                for _ in range(p.normal_log2_power):
                    wn = wn * wn
                e = _dot(nrm[P], pos[Q] - pos[P])
                r = e / den[P]
                z = F(1.0) - r * r
                wz = np.where(z > 0, z, F(0.0))
                a = (u[Q] - u[P]) * isig
                c = F(1.0) - a * a
                c = np.where(c > 0, c, F(0.0))
                wc = c * c
                w = ((h * wn) * wz) * wc
                match = ids[Q] == ids[P]
                Wsum[P] = np.where(match, Wsum[P] + w, Wsum[P])
                S[P] = np.where(match[..., None], S[P] + w[..., None] * rgb[Q], S[P])
        out = np.empty((H, W, 4), F)
        ok = (Wsum > 0) & (ids != -1)
        out[..., :3] = np.where(ok[..., None], S / Wsum[..., None], rgb)
    out[..., 3] = F(1.0)
    return out


def denoise(colour: np.ndarray, guides: np.ndarray, params: Params = Params()) -> np.ndarray:
    """colour (H, W, 4) float32 (the accumulation image; RGB is read), guides (H, W) GUIDE_DTYPE -> (H, W, 4) float32.
    iterations = 0: the input itself."""
    assert colour.dtype == np.float32 and colour.shape == guides.shape + (4,)
    out = colour.copy()
    for i in range(params.iterations):
        out = atrous_pass(out, guides, i, params)
    return out
