"""Adversarial colour images for the preview denoiser ("Non-finite and out-of-range colour"), in pure numpy and
deterministic: plan(ids, recipe, seed) -> Plan; build(ids, recipe, seed) -> its (H, W, 4) float32 image.

Every image starts from seeded uniform noise in [0.2, 0.8] (alpha 1) — inside the default luminance stop, so that the weights among
base pixels are non-zero — and a recipe overwrites chosen pixels with the values on which the contract's arithmetic rules decide the
result: x > 0 ? x : 0 and not fmax, the correctly rounded divide, nothing fused, no flush to zero, a tap of weight 0 still multiplies
its colour.  `ids` is the id map of the guides the image will be filtered under (-1 = miss); placement depends on nothing else.

The shapes and case tables that walk these recipes, and the conditions that keep a case from hiding a failure, are in
tests/denoise_input_cases.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F = np.float32
FLT_MAX = F(3.4028235e38)
# finite_specials: the scalar values (one channel, or all three) ...
FINITE_VALUES = tuple(F(v) for v in (FLT_MAX, -FLT_MAX, 1e30, 65504.0, 1e-30, 1e-38, 3e-39, 1e-40, 1.4e-45, 0.0, -0.0, -0.5, -2.0))
# ... and two colours: the grey whose l falls within an ulp of -1 (1 + l is 0 or tiny, u = -+inf or huge), and the largest l finite
# channels can give.  That l is FLT_MAX itself and not +inf: every operation of l is a rounding of a function that does not decrease
# in r, g, b (the coefficients are positive and rounding is monotonic), so no finite colour exceeds l(FLT_MAX, FLT_MAX, FLT_MAX), and
# that is FLT_MAX exactly (the three binary32 coefficients sum to 1).  l overflows only from a channel that is already infinite —
# nonfinite_seed's +-inf, whose u = inf / inf is NaN.
GREY_MINUS_ONE = (F(-1.0), F(-1.0), F(-1.0))
L_LARGEST = (FLT_MAX, FLT_MAX, FLT_MAX)
FLAT_COLOUR = (F(0.5), F(0.25), F(0.125))
NONFINITE = {"nan": F(np.nan), "+inf": F(np.inf), "-inf": F(-np.inf)}
BLOCK = 12  # subnormal_block: the side of the window


def boundary_xy(H, W):
    """The columns and rows of boundary_placement: both sides of the first 16-wide / 16-high LDS tile edge, of the 64-wide and 4-high
    direct tile edge, and the image's own border.  Interior tile edges first (the order a single seed is placed in)."""
    xs = [x for x in (16, 15, 64, 63, 0, W - 1) if 0 <= x < W]
    ys = [y for y in (4, 3, 16, 15, 0, H - 1) if 0 <= y < H]
    return list(dict.fromkeys(xs)), list(dict.fromkeys(ys))


@dataclass(frozen=True)
class Recipe:
    kind: str                # noise | finite_specials | subnormal_block | nonfinite_seed | flat | zero
    boundary: bool = False   # boundary_placement (finite_specials, subnormal_block, nonfinite_seed)
    value: str = "nan"       # nonfinite_seed: nan | +inf | -inf
    channel: int = 1         # nonfinite_seed: the channel that holds it
    count: int = 300         # finite_specials: how many pixels, at most (a quarter of a small image)
    where: str = "deep"      # nonfinite_seed: deep = the hit pixel farthest from its id's edge; small = the same within the id
    #                          that covers the fewest pixels, but at least 9 (the object bounds the spread)

    @property
    def name(self):
        n = self.kind + (f"[{self.count}]" if self.count != 300 else "")
        if self.kind == "nonfinite_seed":
            n += f"[{self.value},c{self.channel},{self.where}]" if not self.boundary else f"[{self.value},c{self.channel}]"
        return n + ("@boundary" if self.boundary else "")


NOISE = Recipe("noise")


@dataclass
class Plan:
    image: np.ndarray                 # (H, W, 4) float32, alpha 1
    special: np.ndarray               # (H, W) bool: the pixels the recipe overwrote
    seeds: list = field(default_factory=list)   # nonfinite_seed: [(y, x)], hit seeds first
    distance: int = -1                # nonfinite_seed: Chebyshev distance of seeds[0] to the nearest pixel of another id or off the image
    block: tuple = ()                 # subnormal_block: (y0, y1, x0, x1, id) of the window


def edge_distance(ids):
    """(H, W) int: for a hit pixel the Chebyshev distance to the nearest pixel that has another id or lies off the image, minus one —
    0 on an id's rim, k when the (2k + 1)^2 block around the pixel is all of its id and inside the image; -1 on a miss."""
    H, W = ids.shape
    inside = ids >= 0
    dist = np.where(inside, 0, -1)
    level = inside.copy()
    k = 0
    while level.any():
        padded_ok = np.zeros((H + 2, W + 2), bool)
        padded_ok[1:-1, 1:-1] = level
        padded_id = np.full((H + 2, W + 2), -2, ids.dtype)
        padded_id[1:-1, 1:-1] = ids
        nxt = level.copy()
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                nxt &= padded_ok[dy:dy + H, dx:dx + W] & (padded_id[dy:dy + H, dx:dx + W] == ids)
        k += 1
        dist[nxt] = k
        level = nxt
    return dist


def deepest(ids, only=None):
    """(y, x, distance) of the hit pixel (of id `only`, if given) farthest from its id's edge.  Among equals (every pixel of a one-pixel-wide
    image is on a rim): those of the id that covers the most pixels, and of these the middle one in raster order."""
    d = edge_distance(ids)
    if only is not None:
        d = np.where(ids == only, d, -1)
    deep = d == d.max()
    vals = np.unique(ids[deep])
    sizes = [int((ids == v).sum()) for v in vals]
    best = np.argwhere(deep & (ids == vals[int(np.argmax(sizes))]))
    y, x = (int(v) for v in best[len(best) // 2])
    return y, x, int(d[y, x])


def smallest_id(ids, at_least=9):
    """The id that covers the fewest pixels among those that cover at least `at_least` (the lowest id among equals), or None."""
    vals, counts = np.unique(ids[ids >= 0], return_counts=True)
    keep = counts >= at_least
    if not keep.any():
        return None
    return int(vals[keep][np.argmin(counts[keep])])


def _miss_sites(ids):
    """Up to three miss pixels: the first, the middle and the last in raster order."""
    miss = np.argwhere(ids == -1)
    if len(miss) == 0:
        return []
    pick = sorted({0, len(miss) // 2, len(miss) - 1})
    return [tuple(int(v) for v in miss[k]) for k in pick]


def _boundary_sites(ids):
    """The hit pixels at boundary_xy's rows x columns, rows outer."""
    H, W = ids.shape
    xs, ys = boundary_xy(H, W)
    return [(y, x) for y in ys for x in xs if ids[y, x] >= 0]


def _noise(shape, rng):
    H, W = shape
    c = np.ones((H, W, 4), F)
    c[..., :3] = rng.uniform(0.2, 0.8, (H, W, 3)).astype(F)
    return c


def _finite_colour(k, rng, base):
    """The k-th special colour: every third one sets all three channels, the others one channel of the base colour; the two whole
    colours take their turn in the cycle."""
    n = len(FINITE_VALUES) + 2
    j = k % n
    if j == len(FINITE_VALUES):
        return np.array(GREY_MINUS_ONE, F)
    if j == len(FINITE_VALUES) + 1:
        return np.array(L_LARGEST, F)
    c = np.array(base, F)
    if (k // n) % 3 == 0:
        c[:] = FINITE_VALUES[j]
    else:
        c[int(rng.integers(3))] = FINITE_VALUES[j]
    return c


def _subnormal_colour(rng):
    """RGB uniform in [1, 8] x 1e-39 (the smallest normal binary32 is 1.18e-38)."""
    return (rng.uniform(1.0, 8.0, 3) * 1e-39).astype(F)


def plan(ids, recipe: Recipe, seed: int) -> Plan:
    ids = np.asarray(ids)
    H, W = ids.shape
    rng = np.random.default_rng(seed)
    img = _noise((H, W), rng)
    special = np.zeros((H, W), bool)
    p = Plan(img, special)
    kind = recipe.kind

    def put(y, x, rgb):
        img[y, x, :3] = rgb
        special[y, x] = True

    if kind == "noise":
        pass
    elif kind in ("flat", "zero"):
        img[..., :3] = FLAT_COLOUR if kind == "flat" else F(0.0)
        special[:] = True
    elif kind == "finite_specials":
        # several hundred pixels where the image has them (a quarter of a small one), anywhere: hits and misses alike
        count = min(recipe.count, max(6, (H * W) // 4))
        for k, at in enumerate(rng.choice(H * W, count, replace=False)):
            y, x = divmod(int(at), W)
            put(y, x, _finite_colour(k, rng, img[y, x, :3]))
        if recipe.boundary:
            for k, (y, x) in enumerate(_boundary_sites(ids) + _miss_sites(ids)):
                put(y, x, _finite_colour(k, rng, img[y, x, :3]))
    elif kind == "subnormal_block":
        if recipe.boundary:  # across the LDS tile edges x = 15 | 16, y = 15 | 16 and the direct tiles' y = 11 | 12, 15 | 16, 19 | 20
            cy, cx = min(16, H - 1), min(16, W - 1)
        else:
            cy, cx, _ = deepest(ids)
        y0, x0 = max(0, min(cy - BLOCK // 2, H - BLOCK)), max(0, min(cx - BLOCK // 2, W - BLOCK))
        y1, x1 = min(H, y0 + BLOCK), min(W, x0 + BLOCK)
        window = ids[y0:y1, x0:x1]
        hits = window[window >= 0]
        if hits.size:  # the id that covers most of the window: the block lies inside one id
            vals, counts = np.unique(hits, return_counts=True)
            target = int(vals[np.argmax(counts)])
            for y in range(y0, y1):
                for x in range(x0, x1):
                    c = _subnormal_colour(rng)
                    if ids[y, x] == target:
                        put(y, x, c)
            p.block = (y0, y1, x0, x1, target)
        if recipe.boundary:
            for y, x in _boundary_sites(ids) + _miss_sites(ids):
                put(y, x, _subnormal_colour(rng))
    elif kind == "nonfinite_seed":
        v = NONFINITE[recipe.value]
        if recipe.boundary:  # one seed on the first hit pixel of the boundary set, one on a miss pixel
            sites = _boundary_sites(ids)[:1]
            if sites:
                p.distance = int(edge_distance(ids)[sites[0]])
            sites += _miss_sites(ids)[:1]
        else:
            only = smallest_id(ids) if recipe.where == "small" else None
            y, x, p.distance = deepest(ids, only)
            sites = [(y, x)] if ids[y, x] >= 0 else []
        for y, x in sites:
            c = img[y, x, :3].copy()
            c[recipe.channel] = v
            put(y, x, c)
        p.seeds = sites
    else:
        raise ValueError(f"unknown recipe {kind!r}")
    return p


def build(ids, recipe: Recipe, seed: int) -> np.ndarray:
    return plan(ids, recipe, seed).image
