"""Inputs, references and the comparison rule of the math-probe tests (tests/test_math_probe_cpu.py on the host build of
tools/pt_device_probe.hip, tests/test_gpu_math_probe.py on the device build): every grid is a seeded, deterministic array of uint32
words, one row per call, shared by both sides.

  grid W  ("word grid")    every exponent x MANTISSAS x both signs + 2^20 random words: every denormal binade edge, +-0, +-inf, quiet
                           and signalling NaNs.  Compared under the project's rule (degenerate_cases.same_colour): words equal, or both
                           NaN; rows that match only as NaNs are counted and printed.
  grid D  ("domain grid")  per function, the inputs the integrator can produce.  The oracle returns no NaN there (asserted), the rule is
                           plain word equality and no row may differ.
  edge rows                degenerate inputs of the vector functions whose result IS a NaN (normalize of a zero vector, a hit on no face
                           of a cuboid, non-finite points): compared like grid W.

References: the CPU oracle's array entry points (oracle/pt_oracle.py); numpy float32 `/`, sqrt, fmin, fmax (correctly rounded IEEE) for the
four functions the oracle has no counterpart of.  No Python loop runs over rows, no scalar ctypes call is made per row."""
import ctypes as C
import functools

import numpy as np

PI = np.float32(3.14159265)  # csrc/pt_math.hpp
EPSILON = np.float32(0.001)
U32, F32 = np.uint32, np.float32

# which -> (id, words in, words out): the table of tools/pt_device_probe.hip
FUNCS = {name: (i, ic, oc) for i, (name, ic, oc) in enumerate([
    ("f_rcp", 1, 1), ("f_rsqrt", 1, 1), ("pt_sqrt", 1, 1), ("f_sqrt", 1, 1), ("f_div_ieee", 2, 1), ("f_min", 2, 1), ("f_max", 2, 1),
    ("f_mix", 3, 1), ("pt_sincos", 1, 2), ("pt_exp", 1, 1), ("pt_exp_selected", 1, 1), ("pt_log", 1, 1), ("pt_pow5", 1, 1),
    ("aces_film", 1, 1), ("linear_to_inverse_gamma", 1, 1), ("to_unorm8", 1, 1), ("pcg_hash", 1, 2), ("rand01", 1, 2),
    ("pixel_seed", 3, 1), ("v_normalize", 3, 3), ("f_reflect", 6, 3), ("f_refract", 7, 3), ("fresnel_schlick", 3, 1),
    ("hemisphere_direction", 5, 3), ("cosine_sample_hemisphere", 4, 4), ("cuboid_normal", 9, 3),
    ("ref_rcp", 1, 2), ("ref_rsqrt", 1, 2), ("ref_sqrt", 1, 2)])}
SWEEPS = {"exp_selected": 0, "rand01": 1, "f_rcp": 2, "f_rsqrt": 3, "pt_sqrt": 4, "cuboid_scale": 5}
# the project's own accuracy bounds (tests/test_oracle_properties.py, test_contract_reciprocal_root_accuracy), in float ulps
ULP_BOUNDS = {"f_rcp": 0.52, "f_rsqrt": 1.75, "pt_sqrt": 0.502}


def words(a):
    return np.ascontiguousarray(a).view(U32)


def floats(w):
    return np.ascontiguousarray(w, U32).view(F32)


def bits(x):
    return int(F32(x).view(U32))


def around(x, n=64):
    """the n floats below x, x, and the n floats above it (as words; x > 0 or x < 0, away from the binade of zero)"""
    w = bits(x)
    return (w + np.arange(-n, n + 1, dtype=np.int64)).astype(U32)


# ---------------------------------------------------------------------------------------------- the probe library
class Probe:
    """ctypes binding of a build of tools/pt_device_probe.hip.  A non-zero status is remembered, for every build loaded: nothing is
    launched after it."""
    failed = None

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.pt_probe_eval.restype = C.c_int
        self.lib.pt_probe_eval.argtypes = [C.c_int, C.c_void_p, C.c_ulonglong, C.c_int, C.c_void_p, C.c_int]
        self.lib.pt_probe_sweep.restype = C.c_int
        self.lib.pt_probe_sweep.argtypes = [C.c_int, C.c_uint32, C.c_ulonglong, C.c_void_p]

    def _status(self, rc, what):
        if rc != 0:
            Probe.failed = f"{what} returned status {rc}"
            raise AssertionError(Probe.failed)

    def eval(self, name, rows):
        """rows: (n, words in) uint32 -> (n, words out) uint32"""
        assert Probe.failed is None, f"an earlier probe call failed ({Probe.failed}): nothing further is launched"
        which, ic, oc = FUNCS[name]
        rows = np.ascontiguousarray(rows, U32).reshape(-1, ic)
        out = np.zeros((len(rows), oc), U32)
        self._status(self.lib.pt_probe_eval(which, rows.ctypes.data, len(rows), ic, out.ctypes.data, oc), f"pt_probe_eval({name})")
        return out

    def sweep(self, name, first, count):
        assert Probe.failed is None, f"an earlier probe call failed ({Probe.failed}): nothing further is launched"
        out = np.zeros(24, U32)
        self._status(self.lib.pt_probe_sweep(SWEEPS[name], int(first), int(count), out.ctypes.data), f"pt_probe_sweep({name})")
        return {"mismatches": int(out[0]) | (int(out[1]) << 32), "max_error": float(out[2:4].view(np.float64)[0]), "max_error_word": int(out[4]),
                "offenders": [int(w) for w in out[6:6 + int(out[5])]]}


# ---------------------------------------------------------------------------------------------- comparison
def compare(got, want):
    """rows (n, k) of words -> (rows that differ, rows that match only as NaN == NaN, index of the first differing row or -1)"""
    got, want = np.ascontiguousarray(got, U32), np.ascontiguousarray(want, U32)
    assert got.shape == want.shape, (got.shape, want.shape)
    eq = got == want
    both_nan = np.isnan(floats(got)) & np.isnan(floats(want))
    ok = (eq | both_nan).all(-1)
    nan_only = ok & ~eq.all(-1)
    bad = np.flatnonzero(~ok)
    return len(bad), int(nan_only.sum()), (int(bad[0]) if len(bad) else -1)


def describe(name, rows, got, want, first):
    if first < 0:
        return f"{name}: equal"
    hexes = lambda a: " ".join(f"{int(w):08x}" for w in np.atleast_1d(a))
    return f"{name}: first differing row {first}: in {hexes(rows[first])} -> got {hexes(got[first])}, want {hexes(want[first])}"


# ---------------------------------------------------------------------------------------------- references
def reference(oracle, name, rows):
    """what row `rows` (n, words in) must give: (n, words out) uint32"""
    ic, oc = FUNCS[name][1:]
    rows = np.ascontiguousarray(rows, U32).reshape(-1, ic)
    col = lambda k: floats(rows[:, k].copy())
    vec = lambda k: floats(rows[:, k:k + 3].copy())
    one = {"f_rcp": oracle.rcp, "f_rsqrt": oracle.rsqrt, "pt_sqrt": oracle.sqrt, "pt_exp": oracle.exp_array, "pt_exp_selected": oracle.exp_array,
           "pt_log": oracle.log_array, "pt_pow5": oracle.pow5_array, "aces_film": oracle.aces_film_array,
           "linear_to_inverse_gamma": oracle.linear_to_inverse_gamma_array}
    with np.errstate(all="ignore"):
        if name in one:
            out = one[name](col(0))
        elif name == "f_sqrt":
            out = np.sqrt(col(0))
        elif name == "f_div_ieee":
            out = col(0) / col(1)
        elif name == "f_min":
            out = np.fmin(col(0), col(1))
        elif name == "f_max":
            out = np.fmax(col(0), col(1))
        elif name == "f_mix":
            out = oracle.mix_array(col(0), col(1), col(2))
        elif name == "pt_sincos":
            out = np.stack(oracle.sincos_array(col(0)), 1)
        elif name == "to_unorm8":
            out = oracle.to_unorm8_array(col(0)).astype(U32)
        elif name == "pcg_hash":
            out = np.stack(oracle.pcg_hash_array(rows[:, 0]), 1)
        elif name == "rand01":
            v, s = oracle.rand01_array(rows[:, 0])
            out = np.stack([words(v), s], 1)
        elif name == "pixel_seed":
            out = oracle.pixel_seed_array(rows.view(np.int32))
        elif name == "v_normalize":
            out = oracle.normalize_array(vec(0))
        elif name == "f_reflect":
            out = oracle.reflect_array(vec(0), vec(3))
        elif name == "f_refract":
            out = oracle.refract_array(vec(0), vec(3), col(6))
        elif name == "fresnel_schlick":
            out = oracle.fresnel_schlick_array(col(0), col(1), col(2))
        elif name == "hemisphere_direction":
            out = hemisphere_direction_reference(oracle, vec(0), col(3), col(4))
        elif name == "cosine_sample_hemisphere":
            d, s = oracle.cosine_sample_hemisphere_array(vec(0), rows[:, 3])
            out = np.concatenate([words(d), s[:, None]], 1)
        elif name == "cuboid_normal":
            out = oracle.cuboid_normal_array(vec(0), vec(3), vec(6))
        elif name in ("ref_rcp", "ref_rsqrt", "ref_sqrt"):
            x = col(0).astype(np.float64)
            d = 1.0 / x if name == "ref_rcp" else (1.0 / np.sqrt(x) if name == "ref_rsqrt" else np.sqrt(x))
            out = np.ascontiguousarray(d).view(U32)  # (little endian: low word, high word)
        else:
            raise KeyError(name)
    return words(np.ascontiguousarray(out)).reshape(len(rows), oc)


def hemisphere_direction_reference(oracle, n, z, a):
    """hemisphere_direction(n, z, a) (csrc/pt_device.hpp) put together from the oracle's pt_sqrt, sincos and normalize and IEEE float32
    products and sums (numpy): the oracle has the function only inside cosine_sample_hemisphere, behind its two draws.
    fma(-z, z, 1) is taken in float64, where it is exact (z * z has at most 48 significant bits and 1 - z * z fits 53 for |z| <= 1 on the
    2^-24 lattice of the draws; elsewhere the double rounding is harmless only by luck, so the grids stay on it) and rounded once.
    tests/test_math_probe_cpu.py holds this composition to the oracle's cosine_sample_hemisphere."""
    n = np.ascontiguousarray(n, F32).reshape(-1, 3)
    z, a = np.ascontiguousarray(z, F32), np.ascontiguousarray(a, F32)
    r = oracle.sqrt((1.0 - z.astype(np.float64) * z.astype(np.float64)).astype(F32))
    sn, cs = oracle.sincos_array(a)
    return oracle.normalize_array(n + np.stack([r * cs, r * sn, z], 1))


def hemisphere_draws_reference(oracle, seeds):
    """hemisphere_draws: z = fma(rand01, 2, -1) (exact in float64, rounded once), a = rand01 * 2.0f * PI -> (z, a, seeds after both)"""
    r1, s1 = oracle.rand01_array(seeds)
    r2, s2 = oracle.rand01_array(s1)
    return (r1.astype(np.float64) * 2.0 - 1.0).astype(F32), r2 * F32(2.0) * PI, s2


# ---------------------------------------------------------------------------------------------- grid W
MANTISSAS = (0, 1, 2, 3, 0x7FFFFF, 0x7FFFFE, 0x7FFFFD, 0x400000, 0x400001, 0x3FFFFF, 0x2AAAAA, 0x555555, 0x000100, 0x7FFF00, 0x200000, 0x600000)


def structured_words():
    """every exponent x MANTISSAS x both signs (8192 words)"""
    e, m, s = np.meshgrid(np.arange(256, dtype=np.uint64), np.array(MANTISSAS, np.uint64), np.arange(2, dtype=np.uint64), indexing="ij")
    return ((s << 31) | (e << 23) | m).astype(U32).reshape(-1)


@functools.lru_cache(None)
def grid_w():
    rng = np.random.default_rng(20240601)
    w = np.concatenate([structured_words(), rng.integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(U32)])
    w.setflags(write=False)
    return w


@functools.lru_cache(None)
def grid_w_rows(cols):
    """grid W for a function of `cols` scalar arguments: column 0 is grid W, the others seeded permutations of it; in front, the cross
    product of a short list of special words (zeros, smallest and largest denormals and normals, one, infinities, NaNs of both kinds)"""
    w = grid_w()
    if cols == 1:
        return w.reshape(-1, 1)
    rng = np.random.default_rng(7 + cols)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x80800000, 0x00FFFFFF, 0x01000000, 0x3F800000,
                        0xBF800000, 0x3F7FFFFF, 0x40000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
                        0xFFA00000, 0x34000000, 0x4B000000, 0x00400000], U32)
    cross = np.stack(np.meshgrid(*([special] * cols), indexing="ij"), -1).reshape(-1, cols)
    rows = np.concatenate([cross, np.stack([w] + [rng.permutation(w) for _ in range(cols - 1)], 1)])
    rows.setflags(write=False)
    return rows


def is_snan(w):
    w = np.asarray(w, U32)
    return ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0) & ((w & 0x00400000) == 0)


def minmax_comparable(rows):
    """f_min / f_max (and to_unorm8, whose argument goes straight into f_max): C leaves two things open.  The sign of the result for two
    zeros of opposite sign (either operand may come back), and, before C23, a signalling NaN operand (glibc returns a quiet NaN, clang's
    inline expansion and numpy the other operand).  The integrator holds no signalling NaN: every NaN it has came out of an operation."""
    rows = np.asarray(rows, U32)
    zeros = ((rows & 0x7FFFFFFF) == 0).all(1) & (rows[:, 0] != rows[:, -1])
    return ~(is_snan(rows).any(1) | zeros)


def sincos_comparable(w):
    """pt_sincos takes its quadrant from (int)k, k = rint(a * 2 / pi): for |k| >= 2^31 and for a non-finite a, C leaves the conversion
    undefined (x86 gives INT_MIN, gfx950 saturates), so the two sides are only held to each other where |a| < 2^30"""
    a = floats(w)
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & (np.abs(a) < F32(2.0 ** 30))


# ---------------------------------------------------------------------------------------------- grid D, scalar functions
def _uniform(rng, lo, hi, n):
    return (rng.random(n) * (hi - lo) + lo).astype(F32)


@functools.lru_cache(None)
def grid_d(name):
    """the domain grid of `name`: (n, words in) uint32, read-only"""
    rng = np.random.default_rng(abs(hash_name(name)))
    if name == "pt_sincos":
        # hemisphere_draws: a = rand01 * 2.0f * PI, with rand01 = k * 2^-24 for every k (k = 2^24: rand01 == 1.0)
        k = np.arange(2 ** 24 + 1, dtype=np.float64).astype(F32) * F32(2.0 ** -24)
        rows = words(k * F32(2.0) * PI)
    elif name in ("pt_exp", "pt_exp_selected"):
        rows = np.concatenate([words(_uniform(rng, -104.0, 88.73, 2 ** 20)), around(-104.0), around(88.72283935546875), around(-87.33),
                               np.arange(0, 65, dtype=np.int64).astype(U32), (0x80000000 + np.arange(0, 65, dtype=np.int64)).astype(U32)])
    elif name in ("pt_log", "linear_to_inverse_gamma"):
        rows = np.concatenate([words(_uniform(rng, 0.0031308, 1.0, 2 ** 20)), around(0.0031308), around(1.0)])
    elif name == "aces_film":
        rows = words(np.exp(rng.random(2 ** 20) * (np.log(1e4) - np.log(1e-6)) + np.log(1e-6)).astype(F32))
    elif name == "to_unorm8":
        centre = words(((np.arange(256, dtype=np.float64) + 0.5) / 255.0).astype(F32)).astype(np.int64)
        rows = (centre[:, None] + np.arange(-4, 4, dtype=np.int64)[None, :]).astype(U32).reshape(-1)
    elif name in ("rand01", "pcg_hash"):
        rows = np.concatenate([unhash(rand01_tie_words()), rng.integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(U32)])
    elif name == "pixel_seed":
        c = np.array([0, 32767], np.int64)
        f = np.array([0, 1, 1023, 1024, 2 ** 31 - 1], np.int64)
        corners = np.stack(np.meshgrid(c, c, f, indexing="ij"), -1).reshape(-1, 3)
        rand = np.stack([rng.integers(0, 32768, 2 ** 16), rng.integers(0, 32768, 2 ** 16), rng.integers(0, 2 ** 31, 2 ** 16)], 1)
        rows = np.concatenate([corners, rand]).astype(np.int32).view(U32)
    elif name in ("f_rcp", "f_rsqrt", "pt_sqrt", "f_sqrt"):
        # positive normal values over the range test_contract_reciprocal_root_accuracy samples
        rows = words(np.exp(rng.random(2 ** 20) * (np.log(1e30) - np.log(1e-30)) + np.log(1e-30)).astype(F32))
    elif name == "pt_pow5":
        rows = words(_uniform(rng, 0.0, 1.0, 2 ** 20))  # (1 - cosTheta of fresnel_schlick)
    else:
        rows = VECTOR_GRIDS[name]()[0]
    rows = np.ascontiguousarray(rows, U32).reshape(-1, FUNCS[name][1])
    assert len(rows) <= 2 ** 22 or name == "pt_sincos"
    rows.setflags(write=False)
    return rows


@functools.lru_cache(None)
def grid_edge(name):
    """the degenerate rows of a vector function (results may be NaN): (n, words in) uint32"""
    rows = np.ascontiguousarray(VECTOR_GRIDS[name]()[1], U32).reshape(-1, FUNCS[name][1])
    rows.setflags(write=False)
    return rows


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


# ---- rand01: the words around every round-to-even tie of the uint32 -> binary32 conversion, and the seeds that hash to them
def rand01_tie_words():
    """For every leading-bit position above 23 (below, the conversion is exact): mantissas (even, odd, the smallest, the largest: the
    tie that carries into the next binade) x {tie - 1, tie, tie + 1}; and 0, 1, 2^24 - 1, 2^24, 2^24 + 1, 0xFFFFFFFF (rand01 == 1.0)."""
    rng = np.random.default_rng(99)
    out = [np.array([0, 1, 2, 3, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 32 - 1, 2 ** 32 - 2, 2 ** 31, 2 ** 31 - 1], np.uint64)]
    for top in range(24, 32):
        drop = top - 23
        mant = np.concatenate([np.array([2 ** 23, 2 ** 23 + 1, 2 ** 23 + 2, 2 ** 24 - 1, 2 ** 24 - 2], np.uint64),
                               rng.integers(2 ** 23, 2 ** 24, 64, dtype=np.uint64)])
        tie = (mant << np.uint64(drop)) + np.uint64(1 << (drop - 1))
        out.append(np.concatenate([tie - np.uint64(1), tie, tie + np.uint64(1)]))
    w = np.concatenate(out)
    return w[w < 2 ** 32].astype(U32)


_MULT_SEED, _INC_SEED, _MULT_WORD = 747796405, 2891336453, 277803737


def unhash(word):
    """the seeds s with pcg_hash(s) == word (compute.glsl:334-344 is a bijection of uint32: every step is undone in turn)"""
    M = np.uint64(0xFFFFFFFF)
    w = np.asarray(word, np.uint64)
    w = w ^ (w >> np.uint64(22))                                   # (x >> 22) ^ x, 22 * 2 > 32
    w = (w * np.uint64(pow(_MULT_WORD, -1, 2 ** 32))) & M          # * 277803737
    shift = (w >> np.uint64(28)) + np.uint64(4)                    # the top four bits pass through (x >> s) ^ x, s >= 4
    x = w
    for _ in range(8):                                             # x = w ^ (x >> s) converges from the top, >= 4 bits per round
        x = w ^ (x >> shift)
    state = x
    return (((state - np.uint64(_INC_SEED)) & M) * np.uint64(pow(_MULT_SEED, -1, 2 ** 32)) & M).astype(U32)


def seed_before(seed):
    """the seed whose first pcg_hash call leaves `seed` behind (so that the SECOND draw of a stream hashes `seed`)"""
    M = np.uint64(0xFFFFFFFF)
    return ((((np.asarray(seed, np.uint64) - np.uint64(_INC_SEED)) & M) * np.uint64(pow(_MULT_SEED, -1, 2 ** 32))) & M).astype(U32)


# ---------------------------------------------------------------------------------------------- grid D, vector functions
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _special_units():
    """axis-aligned unit vectors of both signs, and unit vectors with denormal, zero and negative-zero components"""
    ax = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, -0.0, 0), (-0.0, 1, -0.0)]
    dn = [(1, 1e-40, 0), (1e-45, -1, 0), (0, 1e-39, 1), (-1e-40, 1e-40, -1), (0.6, 0.8, 1e-41), (0.70710678, 0, 0.70710678),
          (0.57735027, 0.57735027, 0.57735027), (-0.57735027, 0.57735027, -0.57735027)]
    return np.array(ax + dn, F32)


def _rows(*cols):
    cols = [np.ascontiguousarray(c) for c in cols]
    n = len(cols[0])
    return np.concatenate([words(c).reshape(n, -1) for c in cols], 1)


def _grid_normalize():
    rng = np.random.default_rng(301)
    u = _unit(rng, 2 ** 16)
    scaled = u * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (2 ** 16, 1))).astype(F32)
    tiny = np.array([(1e-40, 1e-40, -1e-40), (1e-20, 1e-20, 1e-20), (3e18, -3e18, 3e18)], F32)  # (dot = 0: denormal * inf = inf, no NaN)
    edge = np.array([(0, 0, 0), (-0.0, 0, -0.0), (1e-40, 0, 0), (3e19, 3e19, 3e19), (np.inf, 0, 0), (np.nan, 1, 0), (1e30, 1e30, 1e30), (-1, np.inf, np.nan)], F32)
    return _rows(np.concatenate([u, scaled, _special_units(), tiny])), _rows(edge)


def _incidence(rng, n):
    """(i, n) pairs: random, every special unit vector against every other, normal incidence (i = -n), grazing incidence (n . i = 0
    exactly, and within a few ulp of it)"""
    nr, i = _unit(rng, n), _unit(rng, n)
    sp = _special_units()
    a, b = np.repeat(sp, len(sp), 0), np.tile(sp, (len(sp), 1))
    normal_n = _unit(rng, 256)
    graze_n = np.tile(np.array([(0, 0, 1)], F32), (64, 1))
    t = np.linspace(0, 2 * np.pi, 64)
    graze_i = np.stack([np.cos(t), np.sin(t), np.zeros(64)], 1).astype(F32)
    near_i = graze_i.copy()
    near_i[:, 2] = (np.arange(64) - 32) * F32(2.0 ** -26)
    return (np.concatenate([i, a, -normal_n, graze_i, near_i]), np.concatenate([nr, b, normal_n, graze_n, graze_n]))


def _grid_reflect():
    i, n = _incidence(np.random.default_rng(302), 2 ** 16)
    edge = _rows(np.array([(np.nan, 0, 0), (np.inf, 0, 0), (0, 0, 0)], F32), np.array([(0, 0, 1), (1, 0, 0), (0, 0, 0)], F32))
    return _rows(i, n), edge


ETAS = (1.0 / 1.5, 1.5, 1.0, 0.0, 1000.0)


def _grid_refract():
    rng = np.random.default_rng(303)
    i, n = _incidence(rng, 2 ** 14)
    rows = [_rows(i, n, np.full(len(i), eta, F32)) for eta in ETAS]
    # both sides of total internal reflection: k = 1 - eta^2 (1 - (n.i)^2) changes sign at n.i = -sqrt(1 - 1 / eta^2); n = +z, i in the
    # xz plane with its z within 64 floats of the critical cosine (k moves in steps of ~6e-8: the rows straddle k == 0 closely)
    for eta in (1.5, 1.33, 2.4, 1000.0):
        cc = F32(np.sqrt(1.0 - 1.0 / (float(F32(eta)) ** 2)))
        cz = floats(around(cc))
        sx = np.sqrt(np.maximum(1.0 - cz.astype(np.float64) ** 2, 0.0)).astype(F32)
        for sign in (1.0, -1.0):
            ii = np.stack([sx, np.zeros_like(sx), -cz * F32(sign)], 1)
            nn = np.tile(np.array([(0, 0, sign)], F32), (len(cz), 1))
            rows.append(_rows(ii, nn, np.full(len(cz), eta, F32)))
    edge = _rows(np.array([(np.nan, 0, 0), (0, 0, -1), (0, 0, -1)], F32), np.array([(0, 0, 1), (0, 0, 1), (0, 0, 1)], F32),
                 np.array([1.5, np.nan, np.inf], F32))
    return np.concatenate(rows), edge


def _grid_fresnel():
    rng = np.random.default_rng(304)
    cos = np.concatenate([rng.random(2 ** 14).astype(F32), np.array([0.0, 1.0, -0.0, 1e-40, 0.99999994, 5.9604645e-08, 0.5], F32)])
    iors = [(1.0, 1.5), (1.5, 1.0), (1.0, 1.33), (2.4, 1.0), (1.0, 1.0), (1.0, 1.0000001)]
    rows = [_rows(cos, np.full(len(cos), a, F32), np.full(len(cos), b, F32)) for a, b in iors]
    edge = _rows(np.array([0.5, np.nan, 0.5], F32), np.array([0.0, 1.0, 1.0], F32), np.array([0.0, 1.5, -1.0], F32))  # (0 / 0, NaN, 1 / 0)
    return np.concatenate(rows), edge


def _draws(rng, n):
    """(z, a) as hemisphere_draws forms them from two rand01 values, the extremes included"""
    r1 = np.concatenate([(rng.integers(0, 2 ** 24 + 1, n).astype(np.float64) * 2.0 ** -24).astype(F32), np.array([0.0, 1.0, 0.5, 1.0, 0.0], F32)])
    r2 = np.concatenate([(rng.integers(0, 2 ** 24 + 1, n).astype(np.float64) * 2.0 ** -24).astype(F32), np.array([0.0, 1.0, 1.0, 0.0, 0.25], F32)])
    z = (r1.astype(np.float64) * 2.0 - 1.0).astype(F32)  # fma(r, 2, -1): one rounding
    return z, r2 * F32(2.0) * PI


def _grid_hemisphere_direction():
    rng = np.random.default_rng(305)
    z, a = _draws(rng, 2 ** 16)
    n = np.concatenate([_unit(rng, len(z) - 16), _special_units()])
    # z = +-1 (r = 0) on every special normal except those whose z cancels the sample's
    sp = _special_units()
    zs = np.concatenate([np.full(len(sp), 1.0, F32), np.full(len(sp), -1.0, F32)])
    ns = np.concatenate([sp, sp])
    keep = ns[:, 2] != -zs
    rows = np.concatenate([_rows(n, z, a), _rows(ns[keep], zs[keep], np.full(int(keep.sum()), 1.0, F32))])
    # n = -sample: z = +-1 makes the sample (0, 0, +-1) exactly; the sum is the zero vector and v_normalize(0) = 0 * inf
    edge = _rows(np.array([(0, 0, -1), (0, 0, 1), (-0.0, 0, -1)], F32), np.array([1.0, -1.0, 1.0], F32), np.array([0.0, 3.0, 6.2831855], F32))
    return rows, edge


def _grid_cosine_sample_hemisphere():
    rng = np.random.default_rng(306)
    seeds = rng.integers(0, 2 ** 32, 2 ** 16, dtype=np.uint64).astype(U32)
    one = unhash(np.array([0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFF7F, 0], np.uint64))  # rand01 == 1.0 (twice), the float below it, 0.0
    seeds = np.concatenate([seeds, one, seed_before(one)])                         # ... as the first draw (z) and as the second (a)
    n = np.concatenate([_unit(rng, len(seeds) - 16), _special_units()])
    edge = _rows(np.array([(0, 0, -1), (np.nan, 0, 0)], F32), np.array([one[0], 12345], U32))  # z = 1 against n = -z; a NaN normal
    return _rows(n, seeds), edge


def _grid_cuboid_normal():
    """Per axis four places — on the lower face, on the upper face, inside towards either — in all 64 combinations, and per axis three
    signs of the offset from the centre (-, 0, +) in all 27, for three boxes; then points whose distance from a face is within 2 floats
    of the EPSILON step on either side of the face; NaN and infinite points as edge rows."""
    boxes = [((-1, -1, -1), (1, 1, 1)), ((-3.25, 0.5, 10.0), (1.75, 2.0, 12.5)), ((-0.1, -7.0, 100.0), (0.3, -6.9, 100.7))]
    rows, edges = [], []
    for mn, mx in boxes:
        mn, mx = np.array(mn, F32), np.array(mx, F32)
        ce, half = (mx + mn) * F32(0.5), (mx - mn) * F32(0.5)
        places = np.stack([mn, mx, ce - half * F32(0.5), ce + half * F32(0.5)], 0)  # (4, 3)
        idx = np.stack(np.meshgrid(*([np.arange(4)] * 3), indexing="ij"), -1).reshape(-1, 3)
        p = places[idx, np.arange(3)[None, :]]
        inner = p[(idx >= 2).all(1)]  # on no face: n = 0, and normalize(0) is a NaN (edge rows)
        p = p[(idx < 2).any(1)]
        signs = np.stack([mn, ce, mx], 0)
        idx3 = np.stack(np.meshgrid(*([np.arange(3)] * 3), indexing="ij"), -1).reshape(-1, 3)
        p = np.concatenate([p, signs[idx3, np.arange(3)[None, :]][(idx3 != 1).any(1)]])
        # the EPSILON step: |cs| - half = +-EPSILON, each of the six faces, 2 floats either way; the next axis on its upper face (so
        # that some face is hit on either side of the step), the third inside
        step = []
        for axis in range(3):
            for face in (mn, mx):
                for off in (-EPSILON, EPSILON):
                    base = F32(face[axis] + off)
                    for k in range(-2, 3):
                        q = (ce + half * F32(0.25)).copy()
                        q[(axis + 1) % 3] = mx[(axis + 1) % 3]
                        q[axis] = floats(np.array([bits(base) + k], np.int64).astype(U32))[0]
                        step.append(q)
        p = np.concatenate([p, np.array(step, F32)])
        rows.append(_rows(np.tile(mn, (len(p), 1)), np.tile(mx, (len(p), 1)), p))
        edges.append(_rows(np.tile(mn, (len(inner), 1)), np.tile(mx, (len(inner), 1)), inner))
    mn, mx = np.array(boxes[0][0], F32), np.array(boxes[0][1], F32)
    bad = np.array([(np.nan, 0, 0), (np.inf, 0, 0), (1, -np.inf, np.nan), (np.nan, np.nan, np.nan), (0.5, 0.5, 0.5), (0, 0, 0)], F32)
    edge = _rows(np.tile(mn, (len(bad), 1)), np.tile(mx, (len(bad), 1)), bad)
    return np.concatenate(rows), np.concatenate(edges + [edge])


VECTOR_GRIDS = {"v_normalize": _grid_normalize, "f_reflect": _grid_reflect, "f_refract": _grid_refract, "fresnel_schlick": _grid_fresnel,
                "hemisphere_direction": _grid_hemisphere_direction, "cosine_sample_hemisphere": _grid_cosine_sample_hemisphere,
                "cuboid_normal": _grid_cuboid_normal}
VECTOR_GRIDS = {k: functools.lru_cache(None)(v) for k, v in VECTOR_GRIDS.items()}

# functions compared on grid W (scalar arguments: any word is an input), and those with a domain grid
ON_GRID_W = ("f_rcp", "f_rsqrt", "pt_sqrt", "f_sqrt", "f_div_ieee", "f_min", "f_max", "f_mix", "pt_sincos", "pt_exp", "pt_exp_selected", "pt_log",
             "pt_pow5", "aces_film", "linear_to_inverse_gamma", "to_unorm8", "pcg_hash", "rand01")
ON_GRID_D = ("f_rcp", "f_rsqrt", "pt_sqrt", "f_sqrt", "pt_sincos", "pt_exp", "pt_exp_selected", "pt_log", "pt_pow5", "aces_film",
             "linear_to_inverse_gamma", "to_unorm8", "pcg_hash", "rand01", "pixel_seed") + tuple(VECTOR_GRIDS)


def grid_w_for(name):
    """grid W as rows of `name`, with the rows the C language leaves open taken out by an explicit predicate"""
    rows = grid_w_rows(FUNCS[name][1])
    if name == "pt_sincos":
        rows = rows[sincos_comparable(rows[:, 0])]
    if name in ("f_min", "f_max", "to_unorm8"):
        rows = rows[minmax_comparable(rows)]
    return rows
