"""The temporal stage of the preview denoiser (pt_denoise_set_temporal) restated in numpy float32:
(image, n, guides, history image, history guides, history camera, params, max_history) -> I, the integrated image (rgb, count).

The conventions are those of denoise_reference.py and denoise_variance_reference.py, which this file builds on and edits neither: every
operation is one IEEE binary32 operation on float32 arrays, in the order the definition gives, nothing fused, selects are np.where (every
comparison is False for NaN), `/` is the correctly rounded quotient.  The four taps are gathers (one fancy index per tap), accumulated
in tap order (j outer, i inner); w_n and w_z are the a-trous filter's own expressions.  csrc/pt_denoise.hip (pt_temporal_kernel) must
reproduce this bit for bit (tests/test_gpu_denoise_temporal.py); tests/test_denoise_temporal_cpu.py checks the properties of the
restatement itself.  camera() restates the host's side: the ray matrix A of a BasicDataUBO blob, its inverse B and the ray origin O.
"""
from __future__ import annotations

import numpy as np

import denoise_reference as dr
import denoise_variance_reference as dv  # noqa: F401  (the mode the integrated image is filtered in: see filter())

F = dr.F
DEFAULT_MAX_HISTORY = 32


def camera(basic: bytes):
    """-> (A (3, 3) float64, B (3, 3) float32, O (3,) float32) of a BasicDataUBO blob.  The ray generator (compute.glsl:352-357) is
    linear in the NDC point: wd = A (ndcx, ndcy, 1), A = [a b c] from m = InvProjection and v = InvView read column-major; B = A^-1 in
    double rounded to binary32 once; O = InvView's translation."""
    f = np.frombuffer(basic, np.float32, 32)
    m, v = f[:16].astype(np.float64), f[16:32].astype(np.float64)
    A = np.empty((3, 3), np.float64)
    for r in range(3):
        A[r, 0] = v[r] * m[0] + v[4 + r] * m[1]
        A[r, 1] = v[r] * m[4] + v[4 + r] * m[5]
        A[r, 2] = -(v[r] * m[8] + v[4 + r] * m[9]) - v[8 + r]
    return A, np.linalg.inv(A).astype(F), f[28:31].copy()


def integrate(image, n, guides, history_image, history_guides, B, O, params: dr.Params = dr.Params(), max_history: int = DEFAULT_MAX_HISTORY):
    """image (H, W, 4) float32 (the accumulation image; RGB is read), n = frame index * spp, guides (H, W) GUIDE_DTYPE of the current view;
    history_image (H, W, 4) float32 (rgb, count), history_guides, B (3, 3), O (3,) of the history set — history_image None: no valid
    history.  -> I (H, W, 4) float32, alpha = the per-pixel sample count.  params.sigma_plane and params.normal_log2_power are read."""
    H, W = guides.shape
    assert image.dtype == np.float32 and image.shape == (H, W, 4)
    n = F(n)
    rgb = np.ascontiguousarray(image[..., :3], dtype=F)
    out = np.empty((H, W, 4), F)
    out[..., :3] = rgb
    out[..., 3] = n
    if history_image is None:
        return out
    assert history_image.dtype == np.float32 and history_image.shape == (H, W, 4) and history_guides.shape == (H, W)
    B = np.asarray(B, F).reshape(3, 3)
    O = np.asarray(O, F).reshape(3)
    ids, pos, nrm, t = guides["id"], guides["pos"], guides["normal"], guides["t"]
    hids, hpos, hnrm = history_guides["id"], history_guides["pos"], history_guides["normal"]
    himg = np.ascontiguousarray(history_image, dtype=F)
    fw, fh, half, one = F(W), F(H), F(0.5), F(1.0)
    with np.errstate(all="ignore"):
        # projection
        d = pos - O
        x = (B[0, 0] * d[..., 0] + B[0, 1] * d[..., 1]) + B[0, 2] * d[..., 2]
        y = (B[1, 0] * d[..., 0] + B[1, 1] * d[..., 1]) + B[1, 2] * d[..., 2]
        z = (B[2, 0] * d[..., 0] + B[2, 1] * d[..., 1]) + B[2, 2] * d[..., 2]
        fx = ((x / z) * half + half) * fw - half
        fy = ((y / z) * half + half) * fh - half
        ok = (ids != -1) & (z > 0) & (fx >= -1) & (fx < fw) & (fy >= -1) & (fy < fh)
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
        x0 = np.where(ok, flx, F(0.0)).astype(np.int64)
        y0 = np.where(ok, fly, F(0.0)).astype(np.int64)
        den_plane = F(params.sigma_plane) * t
        Wh = np.zeros((H, W), F)
        Sh = np.zeros((H, W, 3), F)
        Mh = np.zeros((H, W), F)
        # taps
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                take = inside & (hids[cy, cx] == ids)
                bw = (ax if i else one - ax) * (ay if j else one - ay)
                dn = dr._dot(nrm, hnrm[cy, cx])
                wn = np.where(dn > 0, dn, F(0.0))
                for _ in range(params.normal_log2_power):
                    wn = wn * wn
                e = dr._dot(nrm, hpos[cy, cx] - pos)
                r = e / den_plane
                zz = one - r * r
                wz = np.where(zz > 0, zz, F(0.0))
                w = (bw * wn) * wz
                hq = himg[cy, cx]
                Wh = np.where(take, Wh + w, Wh)
                Sh = np.where(take[..., None], Sh + w[..., None] * hq[..., :3], Sh)
                Mh = np.where(take, Mh + w * hq[..., 3], Mh)
        # blend
        Hc = Sh / Wh[..., None]
        m = Mh / Wh
        mh = F(max_history)
        mc = np.where(m < mh, m, mh)
        den = n + mc
        blend = (Wh > 0) & (den > 0)
        mixed = (n * rgb + mc[..., None] * Hc) / den[..., None]
        out[..., :3] = np.where(blend[..., None], mixed, rgb)
        out[..., 3] = np.where(blend, den, n)
    return out


def filter(integrated, guides, params: dr.Params = dr.Params(), variance_sigma=None):
    """The passes over C_0 = I in the mode in force (variance_sigma None: PT_DENOISE_FIXED) -> the image pt_denoise_read returns.  The
    existing restatements read only the RGB of their first input; the alpha every observer of the result sees is 1 (iterations = 0: the
    copy kernel writes it), so the count in I's alpha is replaced by 1 on the way in."""
    c0 = integrated.copy()
    c0[..., 3] = F(1.0)
    if variance_sigma is None:
        return dr.denoise(c0, guides, params)
    return dv.denoise(c0, guides, params, variance_sigma)[0]
