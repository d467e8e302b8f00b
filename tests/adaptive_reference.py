"""The definition of adaptive sampling (pt_adaptive_render; DESIGN.md section 3.5, csrc/pt_adaptive.hip) restated in numpy float32: every
operation below is one IEEE binary32 operation on float32 operands, in the order the definition writes them.

Input: the uniform images U_0 .. U_K (U_k = the image after k uniform frames, U_0 = what it held before), the frame index F the state
starts from, and the parameters.  A tile's record after it has received k samples depends on the tile, k and F only — not on the
decisions of any pass — so `tabulate` computes (M2, e, err) for every k once, and `Sim` replays the passes on that table.
Used by tests/test_adaptive_cpu.py (its own properties) and tests/test_gpu_adaptive.py (the kernel against it, bit for bit).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32 = np.float32
FLT_MAX = F32(3.4028235e38)
DEFAULT_THRESHOLD, DEFAULT_MIN, DEFAULT_MAX = F32(1e-4), 8, 1024
TILE_DTYPE = np.dtype([("k", np.int32), ("k0", np.int32), ("err", np.float32), ("n", np.int32)])
_LANES = np.arange(64)


def lum(c):
    """l(c) = (0.2126 r + 0.7152 g) + 0.0722 b"""
    c = np.asarray(c, F32)
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def tile_grid(rows: int, width: int):
    return (rows + 7) // 8, (width + 7) // 8


def tile_pixels(rows: int, width: int) -> np.ndarray:
    """n per tile: the tile's in-image pixels, (tilesY, tilesX) int32"""
    ty, tx = tile_grid(rows, width)
    h = np.minimum(8, rows - 8 * np.arange(ty))
    w = np.minimum(8, width - 8 * np.arange(tx))
    return (h[:, None] * w[None, :]).astype(np.int32)


def active(k, k0, err, thr, min_samples: int, max_samples: int):
    """step 1: k < max && (k - k0 < min - 1 || err > thr); a NaN err compares false"""
    k, k0 = np.asarray(k), np.asarray(k0)
    with np.errstate(invalid="ignore"):
        return (k < max_samples) & ((k - k0 < min_samples - 1) | (np.asarray(err, F32) > F32(thr)))


def fold_m2(m2, k_next: int, k0: int, d):
    """step 3: M2' = k' > k0 ? M2 + (kf (kf - 1)) (d d) : M2"""
    m2, d = np.asarray(m2, F32), np.asarray(d, F32)
    if k_next <= k0:
        return m2.copy()
    kf = F32(k_next)
    with np.errstate(all="ignore"):
        return m2 + (kf * (kf - F32(1.0))) * (d * d)


def pixel_estimate(m2, k_next: int, k0: int, l_next):
    """step 4: e = max-free clamp of (M2' / ((float)j kf)) / ((s s) (s s)), s = 1 + l(next); 0 while j < 1; NaN -> 0"""
    m2, l_next = np.asarray(m2, F32), np.asarray(l_next, F32)
    j = k_next - k0
    if j < 1:
        return np.zeros(np.broadcast(m2, l_next).shape, F32)
    with np.errstate(all="ignore"):
        v = m2 / (F32(j) * F32(k_next))
        s = F32(1.0) + l_next
        q = (s * s) * (s * s)
        e = v / q
        return np.where(e > F32(0.0), e, F32(0.0)).astype(F32)


def butterfly(lanes):
    """step 5: for step = 1, 2, 4, 8, 16, 32: s_i = s_i + s_(i ^ step) over the last axis (64 lanes); returns all 64 lanes"""
    s = np.asarray(lanes, F32).copy()
    assert s.shape[-1] == 64
    with np.errstate(all="ignore"):
        for step in (1, 2, 4, 8, 16, 32):
            s = s + s[..., _LANES ^ step]
    return s


def tile_lanes(e: np.ndarray) -> np.ndarray:
    """(rows, width) -> (tilesY, tilesX, 64): lane (y & 7) 8 + (x & 7); lanes outside the image hold +0"""
    rows, width = e.shape
    ty, tx = tile_grid(rows, width)
    pad = np.zeros((ty * 8, tx * 8), F32)
    pad[:rows, :width] = e
    return pad.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)


def tile_error(e: np.ndarray, n: np.ndarray) -> np.ndarray:
    """err' = s_0 / (float)n"""
    with np.errstate(all="ignore"):
        return (butterfly(tile_lanes(e))[..., 0] / n.astype(F32)).astype(F32)


@dataclass
class Table:
    """What a pixel / tile holds after it has received k samples, k = F .. K (index k - F)."""
    F: int
    k0: int
    n: np.ndarray        # (tilesY, tilesX)
    m2: np.ndarray       # (K - F + 1, rows, width)
    e: np.ndarray        # (K - F + 1, rows, width)
    err: np.ndarray      # (K - F + 1, tilesY, tilesX)

    @property
    def K(self) -> int:
        return self.F + len(self.err) - 1


def tabulate(U, F: int) -> Table:
    """U[k] = the image after k uniform frames, k = 0 .. K (only k >= F is read)."""
    U = np.asarray(U, F32)
    K = len(U) - 1
    assert 0 <= F <= K
    rows, width = U.shape[1:3]
    k0 = max(F, 1)
    n = tile_pixels(rows, width)
    m2 = [np.zeros((rows, width), F32)]
    e = [np.zeros((rows, width), F32)]
    err = [np.zeros(n.shape, F32)]
    for k in range(F, K):
        l_next = lum(U[k + 1])
        with np.errstate(all="ignore"):
            d = l_next - lum(U[k])
        m2.append(fold_m2(m2[-1], k + 1, k0, d))
        e.append(pixel_estimate(m2[-1], k + 1, k0, l_next))
        err.append(tile_error(e[-1], n))
    return Table(F, k0, n, np.stack(m2), np.stack(e), np.stack(err))


class Sim:
    """The passes replayed on a table: per tile the count k; a pass advances every active tile by one."""

    def __init__(self, table: Table):
        self.t = table
        self.k = np.full(table.n.shape, table.F, np.int32)

    def err(self) -> np.ndarray:
        return np.take_along_axis(self.t.err, (self.k - self.t.F)[None], 0)[0]

    def active(self, thr, min_samples: int, max_samples: int) -> np.ndarray:
        return active(self.k, self.t.k0, self.err(), thr, min_samples, max_samples)

    def run(self, passes: int, thr, min_samples: int, max_samples: int) -> "Sim":
        assert max_samples <= self.t.K, "the table ends before max_samples"
        for _ in range(passes):
            self.k = self.k + self.active(thr, min_samples, max_samples).astype(np.int32)
        return self

    def records(self) -> np.ndarray:
        r = np.empty(self.k.shape, TILE_DTYPE)
        r["k"], r["k0"], r["err"], r["n"] = self.k, self.t.k0, self.err(), self.t.n
        return r

    def pixel_counts(self) -> np.ndarray:
        rows, width = self.t.m2.shape[1:]
        return np.repeat(np.repeat(self.k, 8, 0), 8, 1)[:rows, :width]

    def stats(self):
        """-> (M2, e) per pixel"""
        idx = (self.pixel_counts() - self.t.F)[None]
        return np.take_along_axis(self.t.m2, idx, 0)[0], np.take_along_axis(self.t.e, idx, 0)[0]

    def image(self, U) -> np.ndarray:
        """which U_k every tile must show"""
        U = np.asarray(U)
        return np.take_along_axis(U, self.pixel_counts()[None, :, :, None], 0)[0]

    def status(self, thr, min_samples: int, max_samples: int, spp: int) -> dict:
        return {"active_tiles": int(self.active(thr, min_samples, max_samples).sum()), "tiles": int(self.k.size),
                "pixel_samples": int((self.k.astype(np.int64) * self.t.n).sum()) * spp, "min_count": int(self.k.min()),
                "max_count": int(self.k.max())}


def median_threshold(table: Table, k: int = 8) -> np.float32:
    """the tests' threshold: the median over the tiles of the tabulated err at k samples (a float32 that is one of the values, or the
    float32 mean of the middle two)"""
    return F32(np.median(table.err[k - table.F].astype(F32)))


def non_vacuous(counts: np.ndarray, min_samples: int, max_samples: int) -> bool:
    """at least three distinct counts, at least one strictly between min and max"""
    c = np.unique(counts)
    return len(c) >= 3 and bool(((c > min_samples) & (c < max_samples)).any())
