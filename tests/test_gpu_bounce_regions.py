"""GPU tests of three regions of the bounce (csrc/pt_device.hpp) in which a wavefront issues far more than its lanes need: the
wave-uniform gates around Beer's law, cuboid_normal's selected scale, and sample_env's seam path.  The first two are changed by the
round that added this file; a single tap block for sample_env was built, measured (it raised the vector-instruction count: CHANGELOG.md)
and left out, and its cases stay here as the ground a later form has to stand on: wavefronts that mix interior, seam and corner
footprints at sizes 1, 2, 3 and 256 and in the sRGB8 format, and cuboid hits beside both kinds of misses.  No lane's arithmetic may
change, so every case is compared with the oracle as uint32.  The scenes are aimed at the regions, and what they are aimed at is
checked on the CPU first (pixel-centre pinhole rays: the sub-pixel jitter moves a ray by less than a pixel, and every class asked for
holds many pixels).  The tap rule itself stays with tests/test_gpu_env_sampler.py.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import env_sampler_cases as cases
import env_sampler_reference as ref

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_words(got, want, what):
    diff = (bits(got) != bits(want)).any(-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ from the oracle as uint32, first at {np.argwhere(diff)[:4].tolist()}"


def render_both(pkg, oracle, env, sc, basic, W, H, depth, frames, what, variants=(0, 1)):
    """the oracle's accumulation of `frames` frames against the default kernel and the one-wavefront-per-tile kernel (aperture 0)"""
    objs = sc.ubo_bytes() if sc is not None else bytes(26624)
    ns, nc = (sc.num_spheres, sc.num_cuboids) if sc is not None else (0, 0)
    want = oracle.render(W, H, basic, objs, env, num_spheres=ns, num_cuboids=nc, ray_depth=depth, focal_length=20.0, aperture=0.0, num_frames=frames)
    for variant in variants:
        pt = pkg.PathTracer(env, W, H, depth, 1, 20.0, 0.0)
        try:
            pt.SetVariant(variant)
            if sc is not None:
                pt.UploadScene(sc)
            else:
                z = np.zeros(26624, np.uint8)
                pt.GameObjectsUBO.SubData(0, z.nbytes, z)
            pt.UploadBasicData(basic)
            for _ in range(frames):
                pt.Render()
            got = pt.Result
        finally:
            pt.Dispose()
        assert_same_words(got, want, f"{what}, variant {variant}")
    return want


# ---------------------------------------------------------------------------------------------- CPU side: what a camera is aimed at
def pinhole_rays(basic, W, H):
    """pixel-centre rays of a BasicDataUBO (compute.glsl:352-357), float64: (origin (3,), directions (H, W, 3))"""
    b = np.frombuffer(basic, np.float32).astype(np.float64)
    P, V = b[0:16].reshape(4, 4).T, b[16:32].reshape(4, 4).T  # element (row r, column c) at [4 c + r]
    nx, ny = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    eye = np.stack([nx, ny, -np.ones_like(nx), np.zeros_like(nx)], -1) @ P.T
    wd = np.stack([eye[..., 0], eye[..., 1], -np.ones_like(nx), np.zeros_like(nx)], -1) @ V.T
    d = wd[..., :3]
    return V[:3, 3], d / np.linalg.norm(d, axis=-1, keepdims=True)


def footprint(d, S):
    """sample_env's bilinear footprint of directions (..., 3): (leaves the face in x, leaves it in y, has no fourth tap: a cube corner)"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    zm = az >= np.maximum(ax, ay)
    xm = ~zm & (ax >= ay)
    ma = np.where(zm, az, np.where(xm, ax, ay))
    sc = np.where(zm, np.where(z < 0, -x, x), np.where(xm, np.where(x < 0, z, -z), x))
    tc = np.where(zm | xm, -y, np.where(y < 0, -z, z))
    u, v = (sc / ma * 0.5 + 0.5) * S - 0.5, (tc / ma * 0.5 + 0.5) * S - 0.5
    x0, y0 = np.floor(u), np.floor(v)
    offx, offy = (x0 < 0) | (x0 + 1 >= S), (y0 < 0) | (y0 + 1 >= S)
    corner = ((x0 < 0) | (x0 + 1 >= S)) & ((y0 < 0) | (y0 + 1 >= S))
    return offx, offy, corner


def slab_hits(o, d, cuboids):
    """(H, W) bool: the ray meets one of the cuboids in front of it (compute.glsl:279-294, float64)"""
    hit = np.zeros(d.shape[:-1], bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in cuboids:
            t0, t1 = (c.min.astype(np.float64) - o) / d, (c.max.astype(np.float64) - o) / d
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit |= (near <= far) & (far > 0)
    return hit


# ---------------------------------------------------------------------------------------------- environment
ENV_W = ENV_H = 64
HALF = 2.25  # texels from the centre of the image to its border


def env_cameras(size):
    """looking at a face centre, along a cube edge (face 4, its y = S border, a third of the way along) and into a cube corner"""
    h = 2 * HALF / size
    return {"centre": (4, 0.0, 0.0), "edge": (4, -1.0 / 3.0, 1.0), "corner": (0, 1.0, -1.0)}, h


@pytest.fixture(scope="module")
def cubes():
    out = {}
    for fmt, size in (("rgba32f", 1), ("rgba32f", 2), ("rgba32f", 3), ("rgba32f", 256), ("srgb8", 4)):
        cube = cases.pattern_cube(size, fmt == "srgb8", ref.neighbour_table(size))
        cube.setflags(write=False)
        out[fmt, size] = cube
    return out


@pytest.mark.parametrize("fmt,size", [("rgba32f", 1), ("rgba32f", 2), ("rgba32f", 3), ("rgba32f", 256), ("srgb8", 4)])
def test_environment_only(pkg, native_lib, oracle, cubes, fmt, size):
    """no object: every pixel is sample_env of its primary ray, twice (2 frames).  The edge and the corner camera together hold lanes
    whose footprint leaves the face in x, in y and at a corner, beside interior ones where the size has any."""
    cams, h = env_cameras(size)
    seen = np.zeros(3, int)
    interior = 0
    for name, (face, cs, ct) in cams.items():
        nx, ny = np.meshgrid((np.arange(ENV_W) + 0.5) / ENV_W * 2 - 1, (np.arange(ENV_H) + 0.5) / ENV_H * 2 - 1)
        offx, offy, corner = footprint(cases.point_dirs(face, cs + h * nx, ct + h * ny), size)
        if name != "centre":
            seen += [int((offx & ~corner).sum()), int((offy & ~corner).sum()), int(corner.sum())]
        interior += int((~offx & ~offy).sum())
    print(f"{fmt} {size}: pixels off in x / in y / at a corner {seen.tolist()}, interior {interior}")
    assert seen[2] >= 16 and (size == 1 or (seen[0] >= 16 and seen[1] >= 16))  # (size 1: every footprint is a corner footprint)
    assert size <= 2 or interior >= 16
    for name, (face, cs, ct) in cams.items():
        render_both(pkg, oracle, cubes[fmt, size], None, cases.sweep_basic(face, cs, h, ct, h), ENV_W, ENV_H, 2, 2, f"{fmt} {size}, {name} camera")


def mixed_case(pkg):
    """the default room without its spheres, the camera on the floor's side looking up past the walls into the open ceiling, a 3^2 cube"""
    sc = pkg.scene.Scene()
    sc.cuboids = pkg.scene.default_cuboids()
    cam = pkg.camera.Camera(position=(2.0, -6.0, -9.0), look_x=-70.0, look_y=55.0)
    return sc, pkg.camera.basic_data_ubo(cam, ENV_W, ENV_H)


def test_wavefronts_of_cuboid_hits_and_both_kinds_of_misses(pkg, native_lib, oracle, cubes):
    """one 8 x 8 tile (a wavefront of the tile pass) holds cuboid hits, interior misses and seam misses together"""
    sc, basic = mixed_case(pkg)
    o, d = pinhole_rays(basic, ENV_W, ENV_H)
    hit = slab_hits(o, d, sc.cuboids)
    offx, offy, _ = footprint(d, 3)
    seam, inner = ~hit & (offx | offy), ~hit & ~(offx | offy)
    tiles = lambda m: m.reshape(ENV_H // 8, 8, ENV_W // 8, 8).sum((1, 3))  # noqa: E731
    good = (tiles(hit) >= 8) & (tiles(seam) >= 8) & (tiles(inner) >= 8)
    print(f"mixed case: {int(hit.sum())} hits, {int(seam.sum())} seam misses, {int(inner.sum())} interior misses, {int(good.sum())} tiles hold all three")
    assert good.sum() >= 2
    render_both(pkg, oracle, cubes["rgba32f", 3], sc, basic, ENV_W, ENV_H, 4, 2, "cuboids + open ceiling")


# ---------------------------------------------------------------------------------------------- Beer's law
BEER_W = BEER_H = 32
NZ = F(-0.0)
ABSORBANCE_SETS = {
    # name: (three spheres' absorbances, the glass wall's)
    "zero": ([(0.0, NZ, 0.0), (NZ, NZ, NZ), (0.0, 0.0, NZ)], (0.0, 0.0, 0.0)),
    "equal": ([(0.3, 0.3, 0.3), (1.5, 1.5, 1.5), (0.02, 0.02, 0.02)], (0.01, 0.01, 0.01)),
    "distinct": ([(0.1, 0.2, 0.3), (1.0, 0.5, 0.25), (0.0, 0.4, 0.0)], (0.01, 0.02, 0.03)),
    "mixed": ([(0.0, NZ, 0.0), (0.7, 0.7, 0.7), (0.2, 0.9, 0.4)], (0.01, 0.01, 0.01)),
    "nonfinite": ([(np.inf, 0.1, 0.2), (0.1, np.nan, 0.1), (0.0, 0.0, 0.0)], (0.01, 0.01, 0.01)),
}


def beer_scene(pkg, name, inside=False):
    S = pkg.scene
    spheres, wall = ABSORBANCE_SETS[name]
    sc = S.Scene()
    sc.cuboids = S.default_cuboids()
    sc.cuboids[3].material.absorbance = np.array(wall, F)  # the glass wall behind the spheres
    glass = lambda a, ior: S.Material(albedo=S.vec3(1.0), absorbance=np.array(a, F), specular_chance=0.02, ior=ior,  # noqa: E731
                                      refraction_chance=0.97, refraction_roughness=0.05)
    for i, a in enumerate(spheres):
        sc.spheres.append(S.Sphere(S.vec3(-3.0 + 3.0 * i, 0.0, -15.0), F(1.3), i, glass(a, 1.05 + 0.2 * i)))
    cam = pkg.camera.Camera(position=(0.0, 0.0, -11.0), look_x=-90.0, look_y=0.0)
    if inside:  # the camera sits in a fourth sphere: fromInside at the first hit of every path
        sc.spheres.append(S.Sphere(S.vec3(0.2, 0.1, -11.3), F(1.0), 3, glass((0.5, 0.25, 1.0), 1.3)))
    return sc, pkg.camera.basic_data_ubo(cam, BEER_W, BEER_H)


@pytest.mark.parametrize("name,inside", [(n, False) for n in ABSORBANCE_SETS] + [("mixed", True), ("zero", True)],
                         ids=lambda v: v if isinstance(v, str) else ("inside" if v else "outside"))
def test_beer_gates(pkg, native_lib, oracle, name, inside):
    """three glass spheres in front of the glass wall: absorbances that take no exponential (+-0 channels), one (equal channels), three,
    all of these in one image, and an infinite and a NaN channel; then the same with the camera inside a fourth sphere"""
    sc, basic = beer_scene(pkg, name, inside)
    o, d = pinhole_rays(basic, BEER_W, BEER_H)
    c = np.array([s.position for s in sc.spheres[:3]], np.float64)
    b = np.einsum("hwk,sk->hws", d, c - o)
    on = (b > 0) & (np.linalg.norm(c - o, axis=1) ** 2 - b ** 2 < 1.3 ** 2)  # pixel-centre rays that meet each sphere
    wall = slab_hits(o, d, [sc.cuboids[3]]) & ~on.any(-1)
    print(f"{name}: pixels on the three spheres {on.sum((0, 1)).tolist()}, on the glass wall beside them {int(wall.sum())}")
    assert (on.sum((0, 1)) >= 30).all() and wall.sum() >= 100
    env = pkg.envmap.synthetic_sky_rgba32f(16)
    want = render_both(pkg, oracle, env, sc, basic, BEER_W, BEER_H, 4, 2, f"Beer, {name}{', camera inside' if inside else ''}")
    assert float(np.nan_to_num(want[..., :3], nan=0.0, posinf=0.0).max()) > 0.0


# ---------------------------------------------------------------------------------------------- cuboid normals
NORM_W = NORM_H = 32


def unit_cuboid(pkg, dims=(1.0, 1.0, 1.0)):
    S = pkg.scene
    sc = S.Scene()
    sc.cuboids.append(S.Cuboid(S.vec3(0.0, 0.0, -5.0), np.array(dims, F), 0,
                               S.Material(albedo=S.vec3(0.8, 0.6, 0.4), specular_chance=0.3, specular_roughness=0.2)))
    return sc


def normal_cameras():
    """narrow views from the origin at the cuboid's front face (z = -4.5): 0.008 wide, centred on the edge x = 0.5 and on the corner
    x = y = 0.5, so that a band of pixels hits within EPSILON = 0.001 of them.  Face 5 of the sweep is the plane z = -1: (s, t) -> (-s, -t, -1)"""
    e, h = -0.5 / 4.5, 0.004 / 4.5
    return {"edge": cases.sweep_basic(5, e, h, 0.02, h), "corner": cases.sweep_basic(5, e, h, e, h)}


def oracle_normals(oracle, sc, basic):
    o, d = pinhole_rays(basic, NORM_W, NORM_H)
    mn, mx = sc.cuboids[0].min, sc.cuboids[0].max
    counts = []
    for dir_ in d.reshape(-1, 3).astype(F):
        hit, t1, _ = oracle.ray_cuboid(o.astype(F), dir_, mn, mx)
        if not hit:
            continue
        n = np.asarray(oracle.cuboid_normal(mn, mx, (o.astype(F) + dir_ * F(t1)).astype(F)))
        counts.append(int((n != 0).sum()) if np.isfinite(n).all() else -1)
    return np.bincount(np.array(counts) + 1, minlength=5)  # [NaN normal, 0, 1, 2, 3 non-zero components]


def test_cuboid_normals_on_edges_and_corners(pkg, native_lib, oracle):
    """hit points within EPSILON of an edge and of a corner: normals of two and of three non-zero components (scale f_rsqrt(2), f_rsqrt(3))
    beside the ordinary ones, in one wavefront"""
    sc = unit_cuboid(pkg)
    env = pkg.envmap.synthetic_sky_rgba32f(16)
    seen = np.zeros(5, int)
    for name, basic in normal_cameras().items():
        n = oracle_normals(oracle, sc, basic)
        print(f"{name} camera: oracle normals with NaN / 0 / 1 / 2 / 3 non-zero components: {n.tolist()}")
        seen += n
        render_both(pkg, oracle, env, sc, basic, NORM_W, NORM_H, 2, 2, f"unit cuboid, {name} camera")
    assert seen[2] >= 16 and seen[3] >= 16 and seen[4] >= 4


def test_degenerate_cuboid(pkg, native_lib, oracle):
    """min == max: whatever reaches it is within EPSILON of all three faces or at the centre itself (a zero vector, scale +inf)"""
    sc = unit_cuboid(pkg, dims=(0.0, 0.0, 0.0))
    env = pkg.envmap.synthetic_sky_rgba32f(16)
    h = 1e-6
    for what, basic in (("straight at it", cases.exact_basic((0.0, 0.0, -1.0))), ("around it", cases.sweep_basic(5, 0.0, h, 0.0, h)),
                        ("default camera", pkg.camera.basic_data_ubo(pkg.camera.Camera(), NORM_W, NORM_H))):
        render_both(pkg, oracle, env, sc, basic, NORM_W, NORM_H, 2, 2, f"degenerate cuboid, {what}")
