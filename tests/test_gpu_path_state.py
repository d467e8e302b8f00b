"""GPU tests of a lane's path state at its transitions in the persistent kernels' main loop (csrc/pt_integrate_persistent.hip): a lane
pops a path while its neighbours continue theirs, a path hits or misses, a finished path waits for its pixel's previous frame (in its
lane or parked), a tile is partly outside the image, and a wavefront goes through an iteration with nothing to trace.  The state (ray,
throughput, radiance, RNG state) has ONE home register per value: the pop writes it under the lane mask and the bounce redefines it in
place, and an iteration without active lanes runs through the bounce region with every lane switched off (docs/kernels.md, "Path state
in place").  None of that touches a lane's arithmetic or the order of its draws, so every image equals the oracle bit for bit
(compute.glsl:101-180).
Run with `pytest -m gpu` on an MI355X.  Nothing here reads /root/reference."""
import numpy as np
import pytest

import configs
from test_gpu_parity import assert_bit_exact, bits, oracle_render

pytestmark = pytest.mark.gpu

# the carrying kernel (row 3 of docs/kernels.md, the default workload's) needs at least 12,000 tiles per frame: 125 x 96 is the edge
EDGE_W, EDGE_H = 1000, 768


def render(pkg, w, *, frames, batch=None, variant=0):
    """`frames` Render() calls on a fresh handle; batch None = the library's own choice (pt_set_frame_batch never called)"""
    sc, basic, objs, env, kw = configs.inputs(w)
    pt = pkg.PathTracer(env, w.width, w.height, w.ray_depth, w.spp, w.focal_length, w.aperture)
    pt.SetVariant(variant)
    if batch is not None:
        pt.SetFrameBatch(batch)
    pt.UploadScene(sc)
    pt.UploadBasicData(basic)
    for _ in range(frames):
        pt.Render()
    got = pt.Result
    assert pt.Samples == frames
    pt.Dispose()
    return got


def render_scene(pkg, oracle, sc, cam, what, *, width=104, height=60, depth=8, frames=3):
    """an explicit scene and camera, default tuning, against the oracle"""
    basic = pkg.camera.basic_data_ubo(cam, width, height)
    env = configs.load_env("sky_f32_32")
    want = oracle.render(width, height, basic, sc.ubo_bytes(), env, num_spheres=sc.num_spheres, num_cuboids=sc.num_cuboids, ray_depth=depth,
                         spp=1, focal_length=20.0, aperture=0.14, num_frames=frames)
    pt = pkg.PathTracer(env, width, height, depth, 1, 20.0, 0.14)
    pt.UploadScene(sc)
    pt.UploadBasicData(basic)
    for _ in range(frames):
        pt.Render()
    got = pt.Result
    pt.Dispose()
    assert_bit_exact(got, want, what)
    return want


# ------------------------------------------------------------------------------------------------ the headline row
@pytest.mark.parametrize("size", [(EDGE_W, EDGE_H), (EDGE_W + 1, EDGE_H + 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_carrying_kernel_equals_oracle(pkg, native_lib, oracle, size):
    """12,000 tiles exactly, and 126 x 97 tiles whose right column and bottom row are seven eighths empty (lanes without a pixel
    beside lanes that pop, continue and resolve)."""
    w = configs.Workload("carry_edge", "default", size[0], size[1], 8, "sky_f32_32", frames=3)
    assert ((size[0] + 7) // 8) * ((size[1] + 7) // 8) >= 12000
    assert_bit_exact(render(pkg, w, frames=3), oracle_render(oracle, w), f"default scene {size}, depth 8, 3 frames")


def test_carrying_kernel_two_chained_launches(pkg, native_lib):
    """70 frames = a launch of 64 and a chained launch of 6: paths of the second launch wait for pixels the first one still holds.
    Against the kernel with one wavefront per tile and one launch per frame (variant 1), as uint32."""
    w = configs.Workload("carry_chain", "default", EDGE_W, EDGE_H, 8, "sky_f32_32")
    got = render(pkg, w, frames=70)
    want = render(pkg, w, frames=70, variant=1)
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ from variant 1"


# ------------------------------------------------------------------------------------------------ the small-image row
SMALL = [((8, 8), 70), ((20, 12), 9), ((104, 60), 5)]
_small_want = {}


def small_want(oracle, size, frames, depth):
    key = (size, frames, depth)
    if key not in _small_want:
        w = configs.Workload("small", "default", size[0], size[1], depth, "sky_f32_32", frames=frames)
        _small_want[key] = oracle_render(oracle, w)
        _small_want[key].setflags(write=False)
    return _small_want[key]


@pytest.mark.parametrize("batch", [None, 1], ids=["default_batch", "batch1"])
@pytest.mark.parametrize("depth", [1, 2, 8], ids=lambda d: f"depth{d}")
@pytest.mark.parametrize("size,frames", SMALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"{v}frames")
def test_small_images_equal_oracle(pkg, native_lib, oracle, size, frames, depth, batch):
    """The same main loop with parked resolves.  8 x 8: one tile, so consecutive frames of the same tile are always in flight and lanes
    hold results that wait while others pop; 20 x 12 and 104 x 60: ragged tiles.  Depth 1: every path ends in the tile pass (the
    main loop only ever runs iterations with nothing to trace); depth 2: every popped path ends after one generic bounce.
    pt_set_frame_batch(1): the frame-fed launches."""
    w = configs.Workload("small", "default", size[0], size[1], depth, "sky_f32_32", frames=frames)
    got = render(pkg, w, frames=frames, batch=batch)
    assert_bit_exact(got, small_want(oracle, size, frames, depth), f"{size} x{frames}, depth {depth}, batch {batch}")


# ------------------------------------------------------------------------------------------------ glass
def test_glass_scene_depth_32(pkg, native_lib, oracle):
    """Long paths: a lane keeps its state over up to 32 iterations while its neighbours pop several paths."""
    w = configs.Workload("glass", "glass", 104, 60, 32, "sky_f32_32", frames=2)
    assert_bit_exact(render(pkg, w, frames=2), oracle_render(oracle, w), "glass scene 104x60, depth 32, 2 frames")


# ------------------------------------------------------------------------------------------------ extreme scenes
def test_no_object_in_view(pkg, native_lib, oracle):
    """The default scene seen from above the room, looking up: every primary ray misses, every path ends in the tile pass, the ring
    stays empty and the main loop never holds an active lane."""
    cam = pkg.camera.Camera(position=(0.0, 60.0, -10.0), look_x=-90.0, look_y=80.0)
    want = render_scene(pkg, oracle, pkg.scene.default_scene(), cam, "no object in view")
    assert np.isfinite(want[..., :3]).all()


def closed_room(pkg):
    """six overlapping diffuse slabs around the default camera (the ceiling glows) and a few diffuse spheres: no ray leaves"""
    S = pkg.scene
    sc = S.Scene()
    grey = lambda a: S.Material(albedo=S.vec3(a, a * 0.9, a * 0.8))
    slabs = [((0.0, -12.5, -10.0), (44.0, 1.0, 28.0), grey(0.7)),
             ((0.0, 12.5, -10.0), (44.0, 1.0, 28.0), S.Material(albedo=S.vec3(0.5), emissiv=S.vec3(2.0, 1.8, 1.5))),
             ((-21.5, 0.0, -10.0), (1.0, 26.0, 28.0), grey(0.6)), ((21.5, 0.0, -10.0), (1.0, 26.0, 28.0), grey(0.8)),
             ((0.0, 0.0, -23.5), (44.0, 26.0, 1.0), grey(0.5)), ((0.0, 0.0, 3.5), (44.0, 26.0, 1.0), grey(0.9))]
    for pos, dim, m in slabs:
        sc.cuboids.append(S.Cuboid(np.asarray(pos, np.float32), np.asarray(dim, np.float32), len(sc.cuboids), m))
    rng = np.random.RandomState(11)
    for i in range(9):
        pos = np.array([-14.0 + 3.5 * i, -8.0 + 14.0 * rng.rand(), -18.0 + 12.0 * rng.rand()], np.float32)
        sc.spheres.append(S.Sphere(pos, np.float32(1.0 + rng.rand()), i, grey(0.4 + 0.5 * rng.rand())))
    return sc


def test_closed_diffuse_room(pkg, native_lib, oracle):
    """No path misses, at its first bounce or later: paths end by Russian roulette or at full depth only, so nearly every tile fills
    the ring and no lane ever takes the miss side of the bounce."""
    want = render_scene(pkg, oracle, closed_room(pkg), pkg.camera.Camera(), "closed diffuse room")
    assert float(want[..., :3].max()) > 0.0
