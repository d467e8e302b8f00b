"""The environment sampler against an independent reference (tests/env_sampler_reference.py): the oracle's `pto_sample_env` on every cube
size and direction set of tests/env_sampler_cases.py, the seam index rule against integer geometry at every size that matters, the earlier
binary32 rule restated (equal below 3352, wrong from there), sensitivity, the directions outside the reference, a sanitizer run.

Before the integer rule (the parent's oracle, same tests): `test_seam_index_rule_equals_integer_geometry` failed with wrong taps at
{3352: 12, 3353: 8, 6144: 28, 7168: 80, 8192: 24, 10240: 60, 11264: 152, 12288: 212, 13312: 16, 14336: 116, 15360: 416, 16383: 8,
16384: 96}, each one texel off along the edge next to a face corner, and none at the other listed sizes (4096, 5120, 9216 among them);
`test_oracle_against_reference[srgb8-3352]` failed in the edge sweeps (216 of 5,856 samples beyond the bound, largest error 1.73e-1
against a bound of 3.3e-4); everything else passed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import env_sampler_cases as cases
import env_sampler_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_SIZES = sorted(set(range(1, 513)) | {2047, 2048, 2049, 3351, 3352, 3353, 15360, 16383} | set(range(1024, 16385, 1024)))


@pytest.fixture(scope="module")
def normalize(oracle):
    """the kernel's normalize: v * f_rsqrt(dot(v, v)), one factor for all components"""
    return lambda v: _normalize(oracle, v)


def _normalize(oracle, v):
    v, out = np.ascontiguousarray(v, np.float32), np.zeros(3, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    oracle.lib.pto_normalize(v.ctypes.data_as(fp), out.ctypes.data_as(fp))
    return out


def expected_tie_face(d):
    """ties go Z, then X, then Y: all non-zero components of a tie direction have one magnitude"""
    x, y, z = d
    return (5 if z < 0 else 4) if z != 0 else (1 if x < 0 else 0) if x != 0 else (3 if y < 0 else 2)


@pytest.mark.parametrize("fmt,size", [("rgba32f", s) for s in cases.F32_SIZES] + [("srgb8", s) for s in cases.SRGB_SIZES])
def test_oracle_against_reference(oracle, normalize, fmt, size):
    """error <= bound on every sample and channel of the edge sweeps, corner grids, tie directions and interior points; nothing excluded"""
    table = ref.neighbour_table(size)
    cube = cases.pattern_cube(size, fmt == "srgb8", table)
    worst = 0.0
    for name, dirs in cases.direction_sets(size, normalize).items():
        got = oracle.sample_env_n(cube, dirs).astype(np.float64)
        want = ref.sample(cube, dirs, table)
        ratio = np.abs(got - want.value) / want.bound
        bad = ratio > 1.0
        print(f"{fmt} {size} {name}: {len(dirs)} directions, largest error / bound {ratio.max():.3f}, beyond the bound {int(bad.any(1).sum())}, "
              f"largest error {np.abs(got - want.value).max():.3e}, bound there {want.bound.ravel()[np.argmax(ratio)]:.3e}")
        worst = max(worst, float(ratio.max()))
        assert not bad.any(), f"{name}: {int(bad.any(1).sum())} of {len(dirs)} samples beyond the bound, first at direction {dirs[bad.any(1)][0]}"
        if name == "ties":
            assert [expected_tie_face(d) for d in dirs] == list(want.face)
    assert worst <= 1.0


def test_pattern_cube_levels_are_far_apart():
    """a texel that is wrong by one level step at weight 0.25 shows at every size: the kernel may be a bound away from the reference of the
    right cube, so the reference of the wrong cube is beyond the bound when a quarter step exceeds two bounds"""
    for srgb, sizes in ((False, cases.F32_SIZES), (True, cases.SRGB_SIZES)):
        cube = cases.pattern_cube(3, srgb)
        top = float(ref.srgb8_to_linear(cube[..., :3].max()) if srgb else cube[..., :3].max())
        for size in sizes:
            bound = ref.DU_PER_SIZE * size * 2 * top + ref.ROUND * top  # (the near-boundary form: the cube's whole range)
            assert 0.25 * cases.min_level_step(cube) > 2 * bound, (srgb, size)


def test_lattice_neighbours_are_unique():
    """the definition behind the table: a border texel has exactly one texel of another face at squared distance 2 per edge it lies on"""
    for size in (1, 2, 3, 4, 7):
        n = ref.count_neighbours_at_distance2(size)
        y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
        edges = (x == 0).astype(int) + (x == size - 1) + (y == 0) + (y == size - 1)
        assert (n == edges[None]).all()


def test_seam_index_rule_equals_integer_geometry(oracle):
    """pto_env_wrapped_index = the code env_texel_wrapped runs, against the integer table: every size 1 ... 512, the sizes around 2048 and
    around the first one where the binary32 rule failed, every multiple of 1024 up to the API's 16384, 15360 and 16383"""
    wrong = {}
    for size in INDEX_SIZES:
        n = int((oracle.env_wrapped_index(size) != ref.neighbour_table(size)).any(-1).sum())
        if n:
            wrong[size] = n
    print("sizes with wrong taps:", wrong)
    assert not wrong


# ---- the earlier rule, restated: re-project the tap's centre through 3D in binary32, floor
_libm = ctypes.CDLL("libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _f_rcp(x):
    """pt-f32 reciprocal (csrc/pt_math.hpp) of one positive normal binary32"""
    f = np.float32
    y = np.array([0x7EF311C7 - int(np.array([x], f).view(np.uint32)[0])], np.uint32).view(f)[0]
    for _ in range(3):
        e = f(_libm.fmaf(-x, y, f(1.0)))
        y = f(_libm.fmaf(y, e, y))
    return y


def old_wrapped_index(size):
    """(6, 4, size, 3) through the earlier binary32 rule"""
    f = np.float32
    S = size
    fs = f(S)
    rfs = f(1.0) / fs
    p = np.arange(S, dtype=np.int64)
    out = np.empty((6, 4, S, 3), np.int64)
    centre = lambda i: (i.astype(f) + f(0.5)) * rfs * f(2.0) - f(1.0)
    for edge in range(4):
        ix = [np.full(S, -1), np.full(S, S), p, p][edge]
        iy = [p, p, np.full(S, -1), np.full(S, S)][edge]
        sc, tc = centre(ix), centre(iy)
        one = np.ones(S, f)
        for face in range(6):
            x, y, z = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)][face]
            ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
            isz = az >= np.maximum(ax, ay)
            isx = ~isz & (ax >= ay)
            nface = np.where(isz, np.where(z < 0, 5, 4), np.where(isx, np.where(x < 0, 1, 0), np.where(y < 0, 3, 2)))
            nsc = np.where(isz, np.where(z < 0, -x, x), np.where(isx, np.where(x < 0, z, -z), x)).astype(f)
            ntc = np.where(isz | isx, -y, np.where(y < 0, -z, z)).astype(f)
            ma = np.where(isz, az, np.where(isx, ax, ay)).astype(f)
            rma = np.empty(S, f)
            for m in np.unique(ma):  # (one or two values per edge: the overflowing coordinate)
                rma[ma == m] = _f_rcp(f(m))
            u = (nsc * rma * f(0.5) + f(0.5)) * fs
            v = (ntc * rma * f(0.5) + f(0.5)) * fs
            out[face, edge, :, 0] = nface
            out[face, edge, :, 1] = np.clip(np.floor(u).astype(np.int64), 0, S - 1)
            out[face, edge, :, 2] = np.clip(np.floor(v).astype(np.int64), 0, S - 1)
    return out


def test_integer_rule_returns_the_earlier_rules_texel_below_3352(oracle):
    """every border tap of every size 1 ... 3351: so every fixture, digest and image made with those sizes is unchanged"""
    moved = [size for size in range(1, 3352) if not np.array_equal(oracle.env_wrapped_index(size), old_wrapped_index(size))]
    assert not moved, moved[:10]


def test_earlier_rule_fails_from_3352():
    """the restatement is the rule that failed: 12 taps of size 3352 one texel off along the edge, next to a face corner"""
    old, new = old_wrapped_index(3352), ref.neighbour_table(3352)
    bad = (old != new).any(-1)
    assert int(bad.sum()) == 12
    assert (old[bad][:, 0] == new[bad][:, 0]).all() and (np.abs(old[bad] - new[bad]).sum(-1) == 1).all()
    pos = np.argwhere(bad)[:, 2]
    assert set(pos) <= {0, 3351}
    assert old[0, 1, 0].tolist() == [5, 0, 1] and new[0, 1, 0].tolist() == [5, 0, 0]  # face 0, tap (3352, 0)


# ---- sensitivity
def sensitivity_sets(size, normalize):
    """directions around the changed texels: the edge sweeps and corner grids of face 0's x = S edge and its (S, 0) corner"""
    d = [cases.edge_sweep(size, 0, 1, a) for a in cases.edge_positions(size)] + [cases.corner_grid(size, 0, 1, -1)]
    return cases.to_f32_unit(np.concatenate(d))


def changed_cubes(cube):
    """(name, changed cube, [(face, x, y), ...] of the texels involved): two adjacent border texels swapped, one corner texel changed"""
    S = cube.shape[1]
    a, b = (0, S - 1, 0), (0, S - 1, 1 % S)
    swapped = cube.copy()
    swapped[a[0], a[2], a[1]], swapped[b[0], b[2], b[1]] = cube[b[0], b[2], b[1]].copy(), cube[a[0], a[2], a[1]].copy()
    corner = cube.copy()
    other = cube[1, 0, 0] if not np.array_equal(cube[1, 0, 0], cube[a[0], a[2], a[1]]) else cube[2, 0, 0]
    corner[a[0], a[2], a[1]] = other
    return [("swap", swapped, [a, b]), ("corner", corner, [a])]


def weight_on(sample, texel):
    hit = (sample.taps == np.array(texel)).all(-1)
    return np.where(hit, sample.weights, 0.0).sum(1)


def predicted(sample, texels):
    """(must differ, must agree): a swap moves the value by (wa - wb)(b - a), a changed texel by w * change; the levels are so far apart
    that a quarter of the weight is far beyond the bound (test_pattern_cube_levels_are_far_apart), and no weight means no change"""
    w = [weight_on(sample, t) for t in texels]
    moved = np.abs(w[0] - w[1]) if len(w) == 2 else w[0]
    return moved >= 0.25, np.max(w, 0) == 0.0


@pytest.mark.parametrize("fmt,size", [("rgba32f", 5), ("srgb8", 32)])
def test_sensitivity(oracle, normalize, fmt, size):
    """the oracle on a cube against the reference on a cube with two border texels swapped / one corner texel changed: beyond the bound
    wherever those texels carry a quarter of the weight, within it wherever the footprint does not hold them"""
    cube = cases.pattern_cube(size, fmt == "srgb8")
    dirs = sensitivity_sets(size, normalize)
    got = oracle.sample_env_n(cube, dirs).astype(np.float64)
    for name, changed, texels in changed_cubes(cube):
        want = ref.sample(changed, dirs)
        beyond = (np.abs(got - want.value) > want.bound).any(1)
        differ, agree = predicted(ref.sample(cube, dirs), texels)
        assert differ.sum() > 20 and agree.sum() > 20, name
        assert beyond[differ].all(), name
        assert not beyond[agree].any(), name


# ---- directions outside the reference
@pytest.mark.parametrize("fmt,size", [("rgba32f", 3), ("srgb8", 3), ("rgba32f", 255)])
def test_non_finite_zero_and_subnormal_directions_stay_inside_the_cube(oracle, fmt, size):
    """what the clamp in sample_env promises: a defined tap set inside the cube.  The cube sits between NaN (RGBA32F) / zero (sRGB8: below
    every level of the pattern) guard faces, so a tap read next to the cube shows; the value is a mean of the cube's texels"""
    cube = cases.pattern_cube(size, fmt == "srgb8")
    guarded = np.full((8,) + cube.shape[1:], 0 if fmt == "srgb8" else np.nan, cube.dtype)
    guarded[1:7] = cube
    got = oracle.sample_env_n(guarded[1:7], cases.ODD_DIRS).astype(np.float64)
    lin = ref.srgb8_to_linear(cube[..., :3]) if fmt == "srgb8" else cube[..., :3].astype(np.float64)
    lo, hi = lin.min((0, 1, 2)), lin.max((0, 1, 2))
    assert np.isfinite(got).all()
    assert (got >= lo * (1 - 1e-6)).all() and (got <= hi * (1 + 1e-6)).all()
    again = oracle.sample_env_n(guarded[1:7], cases.ODD_DIRS)
    assert np.array_equal(again.view(np.uint32), oracle.sample_env_n(cube, cases.ODD_DIRS).view(np.uint32))


def test_sanitizer_run_of_the_stand_alone_program(oracle, normalize, tmp_path):
    """pt_oracle.c with its own main under -fsanitize=address,undefined over the direction lists of sizes 3 and 255 and the directions
    outside the reference: no read outside a cube (each is a heap block of its own size), no undefined conversion or shift"""
    exe, dirs_file = str(tmp_path / "env_sampler_sanitize"), str(tmp_path / "dirs.bin")
    src = os.path.join(ROOT, "tests", "env_sampler_sanitize_main.c")
    fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read().split() else []
    subprocess.run(["gcc", "-g", "-O1", "-ffp-contract=off", "-fno-fast-math", *fma, "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", src, "-o", exe, "-lm", "-lpthread"], check=True, capture_output=True)
    dirs = np.concatenate([d for s in (3, 255) for d in cases.direction_sets(s, normalize).values()] + [cases.ODD_DIRS]).astype(np.float32)
    with open(dirs_file, "wb") as f:
        f.write(np.int32(len(dirs)).tobytes())
        f.write(dirs.tobytes())
    p = subprocess.run([exe, dirs_file], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok"), p.stdout + p.stderr
