"""An independent statement of the environment lookup: LINEAR, LOD 0, seamless cube map, in numpy float64.

It shares nothing with the construction of `sample_env` (csrc/pt_device.hpp, oracle/pt_oracle.c) beyond the specification:

* **Face and (s, t)**: OpenGL 4.5 table 8.19 in float64 on the binary32 direction, ties Z, then X, then Y (the order the project
  documents).  |x|, |y|, |z| and their comparisons are exact in any format, so the face never depends on the arithmetic.
* **Neighbours across an edge: integer geometry only** (`neighbour_table`).  Texel (x, y) of a face gets the lattice point of its centre
  on the cube of half-width S: in-face coordinates 2x+1-S and 2y+1-S, the face's axis at +-S.  The neighbour of a border texel across an
  edge is the one texel of another face whose lattice point is at squared distance 2: one step outwards along the in-face axis that
  crosses the edge, one step inwards along the face's own axis.  The 6 x 4 x S table is a look-up of those points among the lattice
  points of all border texels - no float, no reciprocal, no floor.
* **Corner**: the tap that has no texel takes the mean of the other three (GL 4.5 section 8.14.2).
* **sRGB8** texels are linearised with the exact GL formula (section 8.24) before filtering.

**The error bound** (second result of `sample`).  Bilinear filtering is continuous in (u, v), across texel boundaries and across seams,
so a binary32 evaluation whose (u, v) is off by at most DU texels differs from the exact value by at most

    bound = DU * (Du + Dv) + ROUND * M

with Du / Dv the largest difference between horizontally / vertically adjacent taps of the footprint, M the largest tap magnitude.
A binary32 evaluation can land in the NEXT texel cell when (u, v) is within DU of a cell boundary; the slope there belongs to taps
outside this footprint, so for those samples Du and Dv are replaced by the whole cube's value range of the channel (an upper bound
of every tap difference).  No sample is excluded.

DU, from the operations of `sample_env` on one coordinate, in units of eps = 2^-24 (half an ulp, the relative error of one rounding):
    ima = 0.5 * f_rcp(ma)        f_rcp <= 0.51 ulp = 1.02 eps relative (pt_math.hpp); |sc * ima| <= 0.5  ->  0.51 eps absolute
    t   = fma(sc, ima, 0.5)      one rounding of a value in [0, 1]                                        ->  1 eps
    t * fs                       scales both by S, one rounding of a value <= S                          ->  (1.51 + 1) S eps
    ... - 0.5                    one rounding of a value <= S                                             ->  1 S eps
  DU = 3.51 * S * 2^-24 texels (times 1 + 2^-20 for the products of these terms).  fs = (float)S is exact for S <= 2^24.

ROUND, in eps, relative to M (the weights are in [0, 1] and sum to 1, every partial sum is <= M up to these same terms):
    wu = u - floor(u)            exact, except u in (-1, 0) where u + 1 rounds: 0.5 eps on a weight, * (Du <= 2 M)   ->  1
    1 - wu, 1 - wv, product      three roundings per weight, the four weights sum to 1                               ->  3
    corner: a = w * 0.333333343f, w + a   constant 2^-25 off, two roundings, a <= 1/12, three taps                   ->  1
    t00 * w00 and three fma      four roundings of partial sums                                                      ->  4
    sRGB8 decode table           float64 formula rounded once to binary32 against the float64 formula here          ->  1
  ROUND = 10 * 2^-24.

Largest error / bound that the CPU oracle's `pto_sample_env` reaches over every case of tests/test_env_sampler_cpu.py
(13 cubes, edge sweeps, corner grids, the 26 tie directions, random interior directions; every sample and channel): 0.33
(sRGB8 3352, edge sweeps; the worst of each cube lies between 0.18 and 0.33).  A ratio above 1 would mean
that the derivation above is wrong; the bound carries no fitted factor.
"""
import numpy as np

EPS = 2.0 ** -24
DU_PER_SIZE = 3.51 * EPS * (1.0 + 2.0 ** -20)  # texels per unit of S
ROUND = 10.0 * EPS

# inverse of table 8.19: the point (s, t) of face f is  N[f] + s * U[f] + t * V[f]
N = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)
U = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.int64)
V = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.int64)
# the four edges of a face, as the off-face tap sees them: 0: x = -1, 1: x = S, 2: y = -1, 3: y = S (the other coordinate = position p)
EDGES = 4


def _border_xy(S, edge):
    """(x, y) of the S border texels of `edge`, by position along the edge"""
    p = np.arange(S, dtype=np.int64)
    return [(np.zeros_like(p), p), (np.full_like(p, S - 1), p), (p, np.zeros_like(p)), (p, np.full_like(p, S - 1))][edge]


def _outward(face, edge):
    return [-U[face], U[face], -V[face], V[face]][edge]


def lattice_point(S, face, x, y):
    """integer lattice point (..., 3) of the centre of texel (x, y) of `face` on the cube of half-width S"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return S * N[face] + (2 * x + 1 - S)[..., None] * U[face] + (2 * y + 1 - S)[..., None] * V[face]


def _key(P, S):
    w = 2 * S + 1
    return ((P[..., 0] + S) * w + (P[..., 1] + S)) * w + (P[..., 2] + S)


def neighbour_table(S):
    """int64 (6, 4, S, 3): (face, x, y) of the texel across `edge` from the border texel at position p - integer geometry only"""
    pts, ids = [], []
    for f in range(6):
        for e in range(EDGES):
            x, y = _border_xy(S, e)
            pts.append(lattice_point(S, f, x, y))
            ids.append(np.stack([np.full(S, f, np.int64), x, y], -1))
    pts, ids = np.concatenate(pts), np.concatenate(ids)
    keys = _key(pts, S)
    order = np.argsort(keys, kind="stable")
    keys, ids = keys[order], ids[order]
    out = np.empty((6, EDGES, S, 3), np.int64)
    for f in range(6):
        for e in range(EDGES):
            x, y = _border_xy(S, e)
            q = lattice_point(S, f, x, y) + _outward(f, e) - N[f]  # squared distance 2: one step out across the edge, one step in
            k = _key(q, S)
            at = np.searchsorted(keys, k)
            assert (at < len(keys)).all() and (keys[np.minimum(at, len(keys) - 1)] == k).all(), "no texel at squared distance 2"
            hit = ids[at]
            assert (hit[:, 0] != f).all()
            out[f, e] = hit
    return out


def count_neighbours_at_distance2(S):
    """(6, S, S) number of texels of OTHER faces whose lattice point is at squared distance 2: 1 on a border, 2 at a face corner, else 0"""
    allp = np.concatenate([lattice_point(S, f, *np.meshgrid(np.arange(S), np.arange(S))).reshape(-1, 3) for f in range(6)])
    facev = np.repeat(np.arange(6), S * S)
    d2 = ((allp[:, None, :] - allp[None, :, :]) ** 2).sum(-1)
    n = ((d2 == 2) & (facev[:, None] != facev[None, :])).sum(1)
    return n.reshape(6, S, S)  # [face, y, x]


def srgb8_to_linear(b):
    """GL 4.5 section 8.24 in float64"""
    cs = np.asarray(b, np.float64) / 255.0
    return np.where(cs <= 0.04045, cs / 12.92, ((cs + 0.055) / 1.055) ** 2.4)


def face_st(d):
    """table 8.19 on float64 copies of the binary32 direction: face, sc, tc, ma"""
    d = np.asarray(d, np.float32).astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    isz = az >= np.maximum(ax, ay)
    isx = ~isz & (ax >= ay)
    face = np.where(isz, np.where(z < 0, 5, 4), np.where(isx, np.where(x < 0, 1, 0), np.where(y < 0, 3, 2)))
    sc = np.where(isz, np.where(z < 0, -x, x), np.where(isx, np.where(x < 0, z, -z), x))
    tc = np.where(isz | isx, -y, np.where(y < 0, -z, z))
    ma = np.where(isz, az, np.where(isx, ax, ay))
    return face, sc, tc, ma


class Sample:
    """value (n, 3), bound (n, 3), face (n,), taps (n, 4, 3) = (face, x, y) of t00 t10 t01 t11 (-1 where the tap has no texel),
    weights (n, 4) on those texels after the corner rule, near_boundary (n,)"""


def sample(cube, dirs, table=None, value_range=None, extra_du=0.0):
    """cube: (6, S, S, 4) float32 or uint8 (sRGB8); dirs: (n, 3) binary32, finite, not all zero; extra_du: further uncertainty of (u, v) in units
    of S * 2^-24 texels, for a caller whose kernel does not get exactly `dirs` (it says why)"""
    S = cube.shape[1]
    table = neighbour_table(S) if table is None else table
    face, sc, tc, ma = face_st(dirs)
    n = len(face)
    u = (sc / ma * 0.5 + 0.5) * S - 0.5
    v = (tc / ma * 0.5 + 0.5) * S - 0.5
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    wu, wv = u - x0, v - y0
    taps = np.empty((n, 4, 3), np.int64)
    w = np.stack([(1 - wu) * (1 - wv), wu * (1 - wv), (1 - wu) * wv, wu * wv], 1)
    for k, (dx, dy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        x, y = x0 + dx, y0 + dy
        offx, offy = (x < 0) | (x >= S), (y < 0) | (y >= S)
        edge = np.where(offx, np.where(x < 0, 0, 1), np.where(y < 0, 2, 3))
        pos = np.clip(np.where(offx, y, x), 0, S - 1)
        nb = table[face, edge, pos]
        inside = ~offx & ~offy
        taps[:, k, 0] = np.where(inside, face, nb[:, 0])
        taps[:, k, 1] = np.where(inside, x, nb[:, 1])
        taps[:, k, 2] = np.where(inside, y, nb[:, 2])
        taps[offx & offy, k, :] = -1
    missing = taps[:, :, 0] < 0
    assert (missing.sum(1) <= 1).all()
    t = cube[np.maximum(taps[:, :, 0], 0), np.maximum(taps[:, :, 2], 0), np.maximum(taps[:, :, 1], 0), :3]
    t = srgb8_to_linear(t) if cube.dtype == np.uint8 else t.astype(np.float64)
    has = missing.any(1)
    mean3 = np.where(missing[:, :, None], 0.0, t).sum(1) / 3.0
    t = np.where(missing[:, :, None], mean3[:, None, :], t)  # the corner rule: the tap without a texel = mean of the other three
    value = (w[:, :, None] * t).sum(1)
    wm = np.where(missing, w, 0.0).sum(1)
    weights = np.where(missing, 0.0, w + np.where(has, wm / 3.0, 0.0)[:, None])

    du = (DU_PER_SIZE + extra_du * EPS) * S
    Du = np.maximum(np.abs(t[:, 1] - t[:, 0]), np.abs(t[:, 3] - t[:, 2]))
    Dv = np.maximum(np.abs(t[:, 2] - t[:, 0]), np.abs(t[:, 3] - t[:, 1]))
    near = (np.minimum(wu, 1 - wu) <= du) | (np.minimum(wv, 1 - wv) <= du)
    if value_range is None:
        lin = srgb8_to_linear(np.arange(256)) if cube.dtype == np.uint8 else None
        value_range = np.array([(lin[cube[..., c].max()] - lin[cube[..., c].min()]) if lin is not None
                                else float(cube[..., c].max()) - float(cube[..., c].min()) for c in range(3)])
    Du = np.where(near[:, None], value_range[None, :], Du)
    Dv = np.where(near[:, None], value_range[None, :], Dv)
    M = np.abs(t).max(1)
    r = Sample()
    r.value, r.bound, r.face, r.taps, r.weights, r.near_boundary = value, du * (Du + Dv) + ROUND * M, face, taps, weights, near
    return r
