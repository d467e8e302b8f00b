"""Test cubes and direction sets of the environment sampler tests (tests/test_env_sampler_cpu.py, tests/test_gpu_env_sampler.py)."""
import numpy as np

import env_sampler_reference as ref

F32_SIZES = [1, 2, 3, 5, 7, 24, 100, 255, 2048]
SRGB_SIZES = [3, 32, 2048, 3352]
SRGB_STEP, SRGB_BASE = 20, 17  # bytes at least 20 levels apart, all above level 16

# 12 classes: 4 in-face residues x 3 axis pairs.  Opposite faces never touch, every other pair of faces gets disjoint classes, so a
# texel differs from every across-seam neighbour whatever the size; the in-face residue differs between all eight neighbours.  The
# residue has another period per channel (R: 2 x 2, G: 4 x 2, B: 2 x 4) and is rotated on the odd faces, so a texel two steps off, or
# the same texel of the opposite face, differs in some channel.
_AXIS_ORDER = [(0, 1, 2), (2, 0, 1), (1, 2, 0)]
_F32_LEVELS = [0.5 + 0.75 * np.arange(12), 9.0 - 0.75 * np.arange(12), 0.25 + 1.5 * ((np.arange(12) * 5) % 12)]


def _classes(face, size):
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    odd = face & 1
    res = [((x & 1) + 2 * (y & 1) + odd) % 4, (x + 2 * y + odd) % 4, (2 * x + y + 3 * odd) % 4]
    return [(4 * _AXIS_ORDER[c][face // 2] + res[c]).astype(np.int8) for c in range(3)]


def pattern_cube(size, srgb, table=None):
    """(6, size, size, 4) float32 or uint8 whose every texel differs, in every channel, from its eight in-face neighbours and from its
    across-seam neighbours by at least one level step (asserted)"""
    table = ref.neighbour_table(size) if table is None else table
    cube = np.empty((6, size, size, 4), np.uint8 if srgb else np.float32)
    cls = np.empty((3, 6, size, size), np.int8)
    for f in range(6):
        for c, k in enumerate(_classes(f, size)):
            cls[c, f] = k
            cube[f, :, :, c] = (SRGB_BASE + SRGB_STEP * k) if srgb else _F32_LEVELS[c][k].astype(np.float32)
    cube[..., 3] = 255 if srgb else 1.0
    for c in range(3):
        k = cls[c]
        for dy in (-1, 0, 1):  # the eight in-face neighbours
            for dx in (-1, 0, 1):
                if (dx or dy) and size > 1:
                    a = k[:, max(dy, 0):size + min(dy, 0), max(dx, 0):size + min(dx, 0)]
                    b = k[:, max(-dy, 0):size + min(-dy, 0), max(-dx, 0):size + min(-dx, 0)]
                    assert (a != b).all()
        for f in range(6):  # the across-seam neighbours, from the integer table
            for e in range(ref.EDGES):
                x, y = ref._border_xy(size, e)
                nb = table[f, e]
                assert (k[f, y, x] != k[nb[:, 0], nb[:, 2], nb[:, 1]]).all()
    if srgb:
        assert SRGB_BASE > 16 and SRGB_BASE + 11 * SRGB_STEP <= 255
    else:
        assert all(np.diff(np.sort(lv)).min() >= 0.75 for lv in _F32_LEVELS)
    return cube


def min_level_step(cube):
    """smallest difference between two different levels of the cube, after the sRGB decode"""
    if cube.dtype == np.uint8:
        lin = ref.srgb8_to_linear(SRGB_BASE + SRGB_STEP * np.arange(12))
        return float(np.diff(lin).min())
    return 0.75


def point_dirs(face, s, t):
    """float64 directions of the points (s, t) of `face`'s plane; |s| or |t| > 1 lies on a neighbouring face"""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    return ref.N[face] + s[..., None] * ref.U[face] + t[..., None] * ref.V[face]


def to_f32_unit(d):
    d = np.asarray(d, np.float64).reshape(-1, 3)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


# the 12 cube edges, each named once: (face, edge as in the reference: 0: x = -1 side, 1: x = S side, 2: y = -1, 3: y = S)
EDGE_LIST = [(f, e) for f in (0, 1) for e in range(4)] + [(f, e) for f in (2, 3) for e in (2, 3)]
CORNER_LIST = [(f, sx, sy) for f in (0, 1) for sx in (-1, 1) for sy in (-1, 1)]  # the 8 cube corners
ACROSS = np.linspace(-2.25, 2.25, 61)  # texels from the edge: steps of 0.075 texel
GRID = np.linspace(-2.25, 2.25, 25)


def edge_positions(size):
    """positions along an edge in texels: centres of the first, second, middle and last texel and points off the centres"""
    return sorted({p + fr for p in {0, 1, size // 2, size - 1} if p < size for fr in (0.5, 0.23)})


def edge_sweep(size, face, edge, along):
    """61 points across `edge` of `face` at position `along` (texels) along it"""
    c = (1.0 + 2.0 * ACROSS / size) * (-1.0 if edge in (0, 2) else 1.0)
    a = np.full_like(c, 2.0 * along / size - 1.0)
    return point_dirs(face, c, a) if edge < 2 else point_dirs(face, a, c)


def corner_grid(size, face, sx, sy, grid=GRID):
    s, t = np.meshgrid(sx * (1.0 + 2.0 * grid / size), sy * (1.0 + 2.0 * grid / size))
    return point_dirs(face, s.ravel(), t.ravel())


def tie_dirs(normalize):
    """the 26 exact tie and axis directions, normalised by `normalize` (the kernel's: one factor for all components)"""
    d = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
    out = np.array([normalize(np.array(v, np.float32)) for v in d], np.float32)
    a = np.abs(out)
    for v, o in zip(d, a):  # equal components stay equal
        nz = o[np.array(v) != 0]
        assert (nz == nz[0]).all()
    return out


def interior_dirs(size, count=2000, seed=20):
    rng = np.random.default_rng(seed + size)
    lim = 1.0 - 3.0 / size if size > 3 else 1.0  # a texel and a half from every edge (the smallest sizes have no such point: anywhere)
    f = rng.integers(0, 6, count)
    s, t = rng.uniform(-lim, lim, count), rng.uniform(-lim, lim, count)
    return ref.N[f] + s[:, None] * ref.U[f] + t[:, None] * ref.V[f]


def direction_sets(size, normalize):
    """{'edges', 'corners', 'ties', 'interior'} -> (n, 3) float32"""
    edges = np.concatenate([edge_sweep(size, f, e, a) for f, e in EDGE_LIST for a in edge_positions(size)])
    corners = np.concatenate([corner_grid(size, *c) for c in CORNER_LIST])
    return {"edges": to_f32_unit(edges), "corners": to_f32_unit(corners), "ties": tie_dirs(normalize), "interior": to_f32_unit(interior_dirs(size))}


# directions outside the reference: what DESIGN.md and the clamp in sample_env promise is a defined tap set inside the cube
_SUB = np.float32(1e-40)
ODD_DIRS = np.array([[np.nan, 0, 0], [0, np.nan, 1], [1, 1, np.nan], [np.nan] * 3, [np.inf, 0, 0], [-np.inf, 1, 0], [np.inf, np.inf, 0],
                     [np.inf, -np.inf, np.inf], [1, np.inf, -np.inf], [0, 0, 0], [-0.0, 0, -0.0], [_SUB, 0, 0], [_SUB, -_SUB, 0],
                     [_SUB, _SUB, _SUB], [-_SUB, _SUB, -3 * _SUB], [3 * _SUB, -_SUB, _SUB], [_SUB, 3 * _SUB, -_SUB], [-_SUB, -_SUB, 3 * _SUB],
                     [_SUB, 1e-39, -1e-39], [1e-39, -1e-39, 1e-39], [np.nan, np.inf, _SUB], [3e38, 3e38, 3e38], [-3e38, 1e-38, 3e38]], np.float32)


# ---- camera blocks (BasicDataUBO: InvProjection, InvView, ViewPos; element (row r, column c) at [4 c + r]) that steer the primary rays of
# an image: eye = InvProjection (ndc.x, ndc.y, -1, 0), world = InvView (eye.x, eye.y, -1, 0) (compute.glsl:352-357)
def _basic(inv_proj, inv_view):
    b = np.zeros(36, np.float32)
    b[0:16], b[16:32] = inv_proj, inv_view
    return b.tobytes()


def sweep_basic(face, cs, hs, ct, ht):
    """every pixel looks at the point (s, t) = (cs + hs ndc.x, ct + ht ndc.y) of `face`'s plane: a very narrow field of view"""
    p, v = np.zeros(16, np.float32), np.zeros(16, np.float32)
    p[0], p[5], p[8], p[9] = hs, ht, -cs, -ct
    v[0:3], v[4:7], v[8:11] = ref.U[face], ref.V[face], -ref.N[face]
    return _basic(p, v)


def exact_basic(direction):
    """x and y columns zero: every pixel gets the one direction (before the kernel normalises it)"""
    v = np.zeros(16, np.float32)
    v[8:11] = -np.asarray(direction, np.float32)
    return _basic(np.zeros(16, np.float32), v)


SWEEP_W, SWEEP_H = 64, 36
_HALF = 2.25  # texels on the long side of the image


def edge_basics(size, edges=None):
    out = []
    for f, e in (EDGE_LIST if edges is None else edges):
        sign = -1.0 if e in (0, 2) else 1.0
        for a in edge_positions(size):
            along = 2.0 * a / size - 1.0
            if e < 2:
                out.append(sweep_basic(f, sign, 2 * _HALF / size, along, 2 * _HALF * SWEEP_H / SWEEP_W / size))
            else:
                out.append(sweep_basic(f, along, 2 * _HALF / size, sign, 2 * _HALF * SWEEP_H / SWEEP_W / size))
    return out


def corner_basics(size):
    return [sweep_basic(f, sx, 2 * _HALF / size, sy, 2 * _HALF * SWEEP_H / SWEEP_W / size) for f, sx, sy in CORNER_LIST]


TIE_VECTORS = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
