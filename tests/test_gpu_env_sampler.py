"""The kernels' environment sampler against the independent reference (tests/env_sampler_reference.py) and against the oracle.

An empty scene, spp 1, aperture 0, one frame after a reset: each pixel is exactly sample_env(rd) of its primary ray, and the first-hit
query (sample-0 mode) returns that rd bit for bit - an exact (input, output) pair per pixel, no new export.  The camera block steers the
directions (tests/env_sampler_cases.py): a very narrow field of view aimed at an edge position or a corner (64 x 36 pixels over a few
texels), or an inverse projection whose x and y columns are zero (8 x 8 pixels, one chosen direction: the 26 tie directions, and the NaN /
inf / zero / subnormal ones, which have no reference and are compared with the oracle alone).

The bound is the reference's (its docstring derives it from the operations of sample_env).  The reference arithmetic
(pt_set_arithmetic) evaluates the same coordinate with no more roundings (1 / ma correctly rounded: 0.25; sc * ima and + 0.5 unfused: 0.5 + 1;
* S: 1.75 + 1; - 0.5: 1; in all 3.75 S 2^-24 against 3.51, the difference is inside the extra term its test adds for the ray) and the filter
as two nested fused lerps (b - a and the fma: 3 roundings of values <= 2 M per lerp and two levels, 9 with wu, against 10)."""
import numpy as np
import pytest

import env_sampler_cases as cases
import env_sampler_reference as ref

pytestmark = pytest.mark.gpu

_cubes = {}


def cube_and_table(fmt, size):
    """built once per module and left unchanged (the 2048^2 RGBA32F cube is 403 MB, the 3352^2 sRGB8 one 270 MB)"""
    if (fmt, size) not in _cubes:
        table = ref.neighbour_table(size)
        cube = cases.pattern_cube(size, fmt == "srgb8", table)
        cube.setflags(write=False)
        _cubes[fmt, size] = (cube, table)
    return _cubes[fmt, size]


class Sampler:
    """one handle: empty scene, aperture 0; render(basic) -> (rgb (n, 3), rd (n, 3)) of one frame after a reset"""

    def __init__(self, pkg, cube, width, height, spp=1, variant=None, arithmetic=None):
        self.pt = pkg.PathTracer(cube, width, height, 2, spp, 20.0, 0.0)
        objs = np.zeros(26624, np.uint8)
        self.pt.GameObjectsUBO.SubData(0, objs.nbytes, objs)
        if variant is not None:
            self.pt.SetVariant(variant)
        if arithmetic is not None:
            self.pt.SetArithmetic(arithmetic)

    def render(self, basic):
        self.pt.UploadBasicData(basic)
        self.pt.ResetRenderer()
        self.pt.Render()
        img = self.pt.Result
        rd = self.pt.FirstHit(0)["dir"]
        return img[..., :3].reshape(-1, 3).copy(), rd.reshape(-1, 3).copy()

    def close(self):
        self.pt.Dispose()


def render_all(sampler, basics):
    got = [sampler.render(b) for b in basics]
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_within_bound(what, rgb, rd, cube, table):
    want = ref.sample(cube, rd, table)
    ratio = np.abs(rgb.astype(np.float64) - want.value) / want.bound
    print(f"{what}: {len(rd)} pixels, largest error / bound {ratio.max():.3f}")
    bad = (ratio > 1.0).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(rd)} pixels beyond the bound, first at direction {rd[bad][0]}"
    return want


def assert_equals_oracle(what, oracle, rgb, rd, cube):
    want = oracle.sample_env_n(cube, rd)
    diff = (bits(rgb) != bits(want)).any(1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {len(rd)} pixels differ from pto_sample_env(rd), first at direction {rd[diff][0]}"


def expected_tie_face(d):
    x, y, z = d
    return (5 if z < 0 else 4) if z != 0 else (1 if x < 0 else 0) if x != 0 else (3 if y < 0 else 2)


@pytest.mark.parametrize("fmt,size", [("rgba32f", s) for s in (1, 3, 5, 24, 100, 255, 2048)] + [("srgb8", s) for s in (3, 32, 3352)])
def test_kernel_against_reference_and_oracle(pkg, native_lib, oracle, fmt, size):
    """edge sweeps at the first, second, middle and last texel of all 12 edges (at 3352 these hold every corner-adjacent position where the
    binary32 rule was wrong), corner sweeps of all 8 corners, the 26 tie directions: error <= bound on every pixel and channel, and the
    oracle's value bit for bit; the directions outside the reference: the oracle's value bit for bit"""
    cube, table = cube_and_table(fmt, size)
    s = Sampler(pkg, cube, cases.SWEEP_W, cases.SWEEP_H)
    try:
        rgb, rd = render_all(s, cases.edge_basics(size) + cases.corner_basics(size))
    finally:
        s.close()
    assert np.isfinite(rd).all()
    want = assert_within_bound(f"{fmt} {size} sweeps", rgb, rd, cube, table)
    seam = (want.taps[:, :, 0] != want.face[:, None]).any(1)
    corner = (want.taps[:, :, 0] < 0).any(1)
    print(f"  {int(seam.sum())} pixels with a tap across a seam, {int(corner.sum())} with a corner tap")
    assert seam.sum() > len(rd) // 4 and corner.sum() > 100  # the sweeps are where they were aimed
    assert_equals_oracle(f"{fmt} {size} sweeps", oracle, rgb, rd, cube)

    s = Sampler(pkg, cube, 8, 8)
    try:
        tie_rgb, tie_rd = render_all(s, [cases.exact_basic(v) for v in cases.TIE_VECTORS])
        odd_rgb, odd_rd = render_all(s, [cases.exact_basic(v) for v in cases.ODD_DIRS])
    finally:
        s.close()
    for v, d in zip(cases.TIE_VECTORS, tie_rd[::64]):
        nz = np.abs(d[np.array(v) != 0])
        assert (nz == nz[0]).all() and (d[np.array(v) == 0] == 0).all() and (np.sign(d) == np.array(v)).all()  # equal components stay equal
    assert (bits(tie_rd.reshape(-1, 64, 3)) == bits(tie_rd.reshape(-1, 64, 3)[:, :1])).all()  # one direction per image
    want = assert_within_bound(f"{fmt} {size} ties", tie_rgb, tie_rd, cube, table)
    assert [expected_tie_face(v) for v in cases.TIE_VECTORS] == list(want.face[::64])
    assert_equals_oracle(f"{fmt} {size} ties", oracle, tie_rgb, tie_rd, cube)
    assert not np.isfinite(odd_rd).all()  # (they got into the ray through the matrix)
    assert np.isfinite(odd_rgb).all()
    assert_equals_oracle(f"{fmt} {size} non-finite, zero and subnormal directions", oracle, odd_rgb, odd_rd, cube)


@pytest.mark.parametrize("fmt,size", [("rgba32f", 3), ("srgb8", 3352)])
def test_every_kernel_the_sampler_is_compiled_into(pkg, native_lib, oracle, fmt, size):
    """the corner sweeps on the default kernel and on variant 1 (reference and oracle), in reference arithmetic (reference: the oracle is
    the contract's arithmetic), and on the multi-sample kernels (spp 2: two directions per pixel, compared through the oracle's frame)"""
    cube, table = cube_and_table(fmt, size)
    basics = cases.corner_basics(size)
    N = pkg.native
    for what, kw in (("default", {}), ("variant 1", {"variant": 1})):
        s = Sampler(pkg, cube, cases.SWEEP_W, cases.SWEEP_H, **kw)
        try:
            rgb, rd = render_all(s, basics)
        finally:
            s.close()
        assert_within_bound(f"{fmt} {size} corners, {what}", rgb, rd, cube, table)
        assert_equals_oracle(f"{fmt} {size} corners, {what}", oracle, rgb, rd, cube)
    # Reference arithmetic makes its own primary ray, so the first-hit query's rd is not its input.  Exact directions instead: the matrix
    # hands the kernel the binary32 point D of the face plane unrounded, and the reference looks up D itself (the lookup does not depend on
    # the length).  The kernel's rd is D through normalize, * focal length, normalize: three roundings per component (a factor common to
    # the components cancels in sc / ma), so sc / ma is off by at most 6 * 2^-24 and u by 3 S 2^-24: extra_du = 3.
    grid = np.linspace(-1.2, 1.2, 9)  # texels from the corner, steps of 0.3: 9 of a corner's 81 directions have the corner tap
    dirs = np.concatenate([cases.corner_grid(size, *c, grid=grid) for c in cases.CORNER_LIST]).astype(np.float32)
    s = Sampler(pkg, cube, 8, 8, arithmetic=N.PT_ARITH_REFERENCE)
    try:
        rgb = np.stack([s.render(cases.exact_basic(d))[0] for d in dirs])
    finally:
        s.close()
    assert (bits(rgb) == bits(rgb[:, :1])).all()
    want = ref.sample(cube, dirs, table, extra_du=3.0)
    ratio = np.abs(rgb[:, 0].astype(np.float64) - want.value) / want.bound
    print(f"{fmt} {size} corners, reference arithmetic: {len(dirs)} directions, largest error / bound {ratio.max():.3f}")
    assert (want.taps[:, :, 0] < 0).any(1).sum() >= 48 and not (ratio > 1.0).any()
    kw = dict(num_spheres=0, num_cuboids=0, ray_depth=2, focal_length=20.0, aperture=0.0, threads=16)
    objs = bytes(26624)
    s = Sampler(pkg, cube, cases.SWEEP_W, cases.SWEEP_H, spp=2)
    try:
        for b in basics:
            s.pt.UploadBasicData(b)
            s.pt.ResetRenderer()
            s.pt.Render()
            want = oracle.render(cases.SWEEP_W, cases.SWEEP_H, b, objs, cube, spp=2, **kw)
            diff = (bits(s.pt.Result) != bits(want)).any(-1)
            assert not diff.any(), f"spp 2: {int(diff.sum())} pixels differ from the oracle's frame"
    finally:
        s.close()


def test_swapped_border_texels_show_at_the_predicted_pixels(pkg, native_lib):
    """the cube uploaded with two adjacent border texels swapped, compared with the reference of the unswapped cube: beyond the bound at
    every pixel where the swap moves a quarter of the weight, within it at every pixel whose footprint holds neither texel (the CPU test's
    prediction, tests/test_env_sampler_cpu.py::test_sensitivity)"""
    size = 5
    cube, table = cube_and_table("rgba32f", size)
    a, b = (0, size - 1, 0), (0, size - 1, 1)
    swapped = cube.copy()
    swapped[a[0], a[2], a[1]], swapped[b[0], b[2], b[1]] = cube[b[0], b[2], b[1]].copy(), cube[a[0], a[2], a[1]].copy()
    s = Sampler(pkg, swapped, cases.SWEEP_W, cases.SWEEP_H)
    try:
        rgb, rd = render_all(s, cases.edge_basics(size, edges=[(0, 1)]) + [cases.corner_basics(size)[2]])
    finally:
        s.close()
    want = ref.sample(cube, rd, table)
    beyond = (np.abs(rgb.astype(np.float64) - want.value) > want.bound).any(1)
    w = [np.where((want.taps == np.array(t)).all(-1), want.weights, 0.0).sum(1) for t in (a, b)]
    differ, agree = np.abs(w[0] - w[1]) >= 0.25, np.maximum(w[0], w[1]) == 0.0
    print(f"{int(differ.sum())} pixels must differ, {int(agree.sum())} must agree, {int(beyond.sum())} of {len(rd)} are beyond the bound")
    assert differ.sum() > 100 and agree.sum() > 100
    assert beyond[differ].all() and not beyond[agree].any()
