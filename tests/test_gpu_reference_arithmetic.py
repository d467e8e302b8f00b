"""pt_set_arithmetic(h, PT_ARITH_REFERENCE) on the GPU: the reference-arithmetic kernel (csrc/pt_integrate_reference.hip) renders what
the oracle renders with llvmpipe's arithmetic choices (witness build, base variant 951) BIT FOR BIT — over the parity workloads, the
parameter extremes, partial images and group handles — and therefore misses the reference's own fixtures exactly where that restatement
does (49 pixel-frames outside the band, contract 787).  Mode switches keep deferred frames in the arithmetic they were issued under."""
import math

import numpy as np
import pytest

import __graft_entry__ as graft
import configs
import fixtures
import tolerances as tol

pytestmark = pytest.mark.gpu

LLVMPIPE = graft.load_oracle().LLVMPIPE  # (951) every one of llvmpipe's choices the oracle restates: oracle/pt_oracle.py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_exact(got, want, what):
    same = bits(got) == bits(want)
    if not same.all():
        bad = ~same.all(-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ from the oracle; first at {np.argwhere(bad)[:5].tolist()}")


@pytest.fixture(scope="module")
def ref_oracle():
    import __graft_entry__ as graft
    o = graft.load_oracle().Oracle(perturb=True)
    o.set_base_variant(LLVMPIPE)
    yield o
    o.set_base_variant(0)


def tracer(pkg, w, mode=1, **extra):
    sc, basic, objs, env, kw = configs.inputs(w)
    pt = pkg.PathTracer(env, w.width, w.height, w.ray_depth, w.spp, w.focal_length, w.aperture, **extra)
    pt.SetArithmetic(mode)
    pt.UploadScene(sc)
    pt.UploadBasicData(basic)
    return pt


def oracle_render(o, w, frames=None, **extra):
    sc, basic, objs, env, kw = configs.inputs(w)
    return o.render(w.width, w.height, basic, objs, env, num_frames=w.frames if frames is None else frames, threads=16, **kw, **extra)


def hip_render(pkg, w, frames=None, **extra):
    pt = tracer(pkg, w, **extra)
    for _ in range(w.frames if frames is None else frames):
        pt.Render()
    out = pt.Result
    pt.Dispose()
    return out


# ------------------------------------------------------------------------------------------------ (1) bit-exact with the oracle
@pytest.mark.parametrize("w", configs.SMALL_FRAMES + configs.ENV_ONLY, ids=lambda w: w.name)
def test_reference_mode_equals_oracle_951_bit_exact(pkg, native_lib, ref_oracle, w):
    assert_bit_exact(hip_render(pkg, w), oracle_render(ref_oracle, w), w.name)


@pytest.mark.parametrize("w", [
    configs.Workload("depth50", "default", 40, 24, 50, "sky_f32_32"),
    configs.Workload("spp10", "default", 40, 24, 8, "sky_f32_32", spp=10),
    configs.Workload("wide_aperture", "default", 64, 36, 8, "sky_f32_32", aperture=3.0, focal_length=5.0),
    configs.Workload("ragged_77x53", "default", 77, 53, 8, "sky_f32_32", frames=2),
    configs.Workload("inside_glass", "edge", 64, 36, 24, "sky_srgb_32", frames=2),
], ids=lambda w: w.name)
def test_reference_mode_parameter_extremes(pkg, native_lib, ref_oracle, w):
    assert_bit_exact(hip_render(pkg, w), oracle_render(ref_oracle, w), w.name)


def test_reference_mode_full_ubo(pkg, native_lib, ref_oracle):
    """256 spheres AND 64 cuboids: the whole GameObjectsUBO, every object visited by every ray."""
    s = pkg.scene
    sc = s.stress_scene(256)
    rng = np.random.RandomState(5)
    sc.cuboids = []
    for i in range(64):
        c = rng.uniform([-18, -11, -21], [18, 11, 1])
        sc.cuboids.append(s.Cuboid(c.astype(np.float32), rng.uniform(0.2, 1.5, 3).astype(np.float32), i,
                                   s.Material(albedo=rng.rand(3), specular_chance=rng.rand() * 0.5, specular_roughness=rng.rand(),
                                              ior=1 + rng.rand(), refraction_chance=rng.rand() * 0.5)))
    W, H = 96, 54
    basic = pkg.camera.basic_data_ubo(pkg.camera.Camera(), W, H)
    env = configs.load_env("sky_f32_32")
    pt = pkg.PathTracer(env, W, H, 8, 1, 20.0, 0.14)
    pt.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
    pt.UploadScene(sc)
    pt.UploadBasicData(basic)
    pt.Render()
    got = pt.Result
    pt.Dispose()
    want = ref_oracle.render(W, H, basic, sc.ubo_bytes(), env, num_spheres=256, num_cuboids=64, ray_depth=8, threads=16)
    assert_bit_exact(got, want, "256 spheres + 64 cuboids")


def test_reference_mode_2048_srgb_cube(pkg, native_lib, ref_oracle):
    """The reference's 2048^2 x 6 SRGB8_A8 cube (MainWindow.cs:177-187): texel indices up to 25.2 M."""
    env = pkg.envmap.synthetic_sky_srgb8(2048)
    w = configs.Workload("sky2048", "default", 160, 90, 8, "unused")
    sc = configs.make_scene(w.scene)
    basic = pkg.camera.basic_data_ubo(pkg.camera.Camera(position=w.position, look_x=w.look[0], look_y=w.look[1]), w.width, w.height)
    pt = pkg.PathTracer(env, w.width, w.height, w.ray_depth, 1, w.focal_length, w.aperture)
    pt.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
    pt.UploadScene(sc)
    pt.UploadBasicData(basic)
    pt.Render()
    got = pt.Result
    pt.Dispose()
    want = ref_oracle.render(w.width, w.height, basic, sc.ubo_bytes(), env, num_spheres=sc.num_spheres, num_cuboids=sc.num_cuboids,
                             ray_depth=w.ray_depth, threads=16)
    assert_bit_exact(got, want, "2048^2 sRGB8 cube")


def test_reference_mode_partial_images(pkg, native_lib, ref_oracle):
    """pt_set_tile (the oracle's y0 / rows) and pt_set_interleaved_tile (block-cyclic bands): the kernel renders global rows."""
    from opentk_pathtracer_amd import distributed as D
    w = configs.Workload("tiles", "default", 120, 70, 8, "sky_f32_32", frames=2)
    full = oracle_render(ref_oracle, w)
    for y0, rows in [(13, 29), (0, 8), (61, 9)]:
        pt = tracer(pkg, w)
        pt.SetTile(y0, rows)
        for _ in range(w.frames):
            pt.Render()
        got = pt.Result
        pt.Dispose()
        assert_bit_exact(got, oracle_render(ref_oracle, w, y0=y0, rows=rows), f"tile y0={y0} rows={rows}")
    for rank, world, band in [(0, 3, 8), (2, 3, 8), (1, 2, 16)]:
        pt = tracer(pkg, w)
        pt.SetInterleavedTile(rank, world, band)
        for _ in range(w.frames):
            pt.Render()
        got = pt.Result
        pt.Dispose()
        assert_bit_exact(got, full[D.interleaved_rows(w.height, rank, world, band)], f"interleaved {rank}/{world} band {band}")


def test_reference_mode_group_handle(pkg, native_lib, ref_oracle):
    """A same-device group [0, 0]: pt_set_arithmetic fans out to the parts, the gather is unchanged."""
    w = configs.Workload("group", "default", 200, 117, 8, "sky_f32_32", frames=3)
    pt = tracer(pkg, w, devices=[0, 0])
    for _ in range(w.frames):
        pt.Render()
    got = pt.Result
    pt.Dispose()
    assert_bit_exact(got, oracle_render(ref_oracle, w), "group handle [0, 0]")


# ------------------------------------------------------------------------------------------------ (2) against the reference's fixtures
def test_reference_mode_against_the_reference_fixtures(pkg, native_lib, ref_oracle):
    """Every frame_* and sparse_* fixture, HIP frame by frame: the pixel-frames outside the band are the oracle's (<= 49; contract 787),
    and the first frames of the float-environment fixtures equal the reference bit for bit in >= 97 % of the pixels."""
    def outside(exp, got, band):
        ok = tol.within(exp, got, band) | (np.isnan(exp).any(-1) & np.isnan(got).any(-1))
        return int((~ok).sum()), ok.size

    hip_out = ora_out = n = 0
    same = {0: 0, 1: 0}
    npix = 0
    for name in fixtures.names("frame_") + fixtures.names("sparse_"):
        fx = fixtures.load(name)
        kw = fixtures.kwargs(fx)
        band = tol.SRGB_REL_TOL if fx["env"].dtype == np.uint8 else tol.REL_TOL
        if name.startswith("sparse_"):
            pt = fixtures.hip_tracer(pkg, fx)
            pt.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
            pt.Render()
            img = pt.Result
            pt.Dispose()
            xy = fx["xy"]
            got = img[xy[:, 1], xy[:, 0], :3][None]
            want = ref_oracle.render_pixels(fx["width"], fx["height"], fx["basic"], fx["objects"], fx["env"], xy, frame=0, **kw)[None][..., :3]
            exp = fx["expected"][None]
        else:
            idx = [int(f) for f in fx["frame_indices"]]
            dumps = ref_oracle.render(fx["width"], fx["height"], fx["basic"], fx["objects"], fx["env"], num_frames=fx["frames"],
                                      dump_each=True, threads=16, **kw)
            want, exp = dumps[idx][..., :3], fx["expected"]
            got = []
            for mode in (pkg.native.PT_ARITH_REFERENCE, pkg.native.PT_ARITH_CONTRACT):
                pt = fixtures.hip_tracer(pkg, fx)
                pt.SetArithmetic(mode)
                frames = []
                for f in range(fx["frames"]):
                    pt.Render()
                    if f in idx:
                        frames.append(pt.Result[..., :3].copy())
                pt.Dispose()
                if mode == pkg.native.PT_ARITH_REFERENCE:
                    got = np.stack(frames)
                first = frames[0]
                if fx["env"].dtype != np.uint8 and idx[0] == 0:
                    same[mode] += int((bits(first) == bits(exp[0])).all(-1).sum())
            if fx["env"].dtype != np.uint8 and idx[0] == 0:
                npix += exp[0].shape[0] * exp[0].shape[1]
        assert_bit_exact(got, want, f"{name} (reference mode vs oracle 951)")
        for k in range(got.shape[0]):
            h, m = outside(exp[k], got[k], band)
            o, _ = outside(exp[k], want[k], band)
            hip_out += h
            ora_out += o
            n += m
    share_ref, share_contract = same[1] / npix, same[0] / npix
    print(f"\n  outside the band: {hip_out} of {n} pixel-frames (oracle 951: {ora_out}); first frames bit for bit equal to the reference: "
          f"reference mode {share_ref:.1%}, default mode {share_contract:.1%}")
    assert n > 150000
    assert hip_out == ora_out and hip_out <= 49
    assert share_ref >= 0.97 and share_contract <= 0.5


# ------------------------------------------------------------------------------------------------ (3) mode switches
def test_mode_switch_keeps_deferred_frames_in_their_arithmetic(pkg, native_lib, oracle, ref_oracle):
    w = configs.Workload("switch", "default", 128, 72, 8, "sky_f32_32")
    pt = tracer(pkg, w, mode=pkg.native.PT_ARITH_CONTRACT)
    pt.SetFrameBatch(8)
    for _ in range(3):
        pt.Render()                                            # (deferred: issued under the contract)
    pt.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
    for _ in range(2):
        pt.Render()
    got = pt.Result
    want = oracle_render(oracle, w, frames=3)
    want = oracle_render(ref_oracle, w, frames=2, frame_start=3, image=want)
    assert_bit_exact(got, want, "contract frames [0, 3) then reference frames [3, 5)")
    # pt_present_rgba8 in reference mode: the classic tone map of the accumulation
    assert np.array_equal(pt.Present(), oracle.postprocess(got)[1])
    # back to the contract, then a clean image
    pt.SetArithmetic(pkg.native.PT_ARITH_CONTRACT)
    pt.ResetRenderer()
    for _ in range(2):
        pt.Render()
    assert_bit_exact(pt.Result, oracle_render(oracle, w, frames=2), "contract again after pt_reset")
    pt.Dispose()


def test_bad_mode_is_rejected(pkg, native_lib):
    w = configs.Workload("bad", "default", 16, 16, 1, "sky_f32_32")
    pt = tracer(pkg, w, mode=pkg.native.PT_ARITH_CONTRACT)
    assert native_lib.pt_set_arithmetic(pt._h, 2) == pkg.native.PT_E_BAD_ARGUMENT
    assert native_lib.pt_set_arithmetic(pt._h, -1) == pkg.native.PT_E_BAD_ARGUMENT
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ (4) rate
def test_rate_of_both_modes(pkg, native_lib):
    """1080p, 8 bounces, 1 spp, default scene: Msamples/s of both modes (printed; recorded in DESIGN.md)."""
    rates = {}
    for mode, label in ((pkg.native.PT_ARITH_CONTRACT, "contract"), (pkg.native.PT_ARITH_REFERENCE, "reference")):
        pt = tracer(pkg, configs.C2, mode=mode)
        for _ in range(3):
            pt.Render()
        pt.TimerBegin()
        for _ in range(20):
            pt.Render()
        ms = pt.TimerEnd()
        pt.Dispose()
        rates[label] = 20 * configs.C2.width * configs.C2.height / (ms * 1e-3) / 1e6
    print(f"\n  1080p / 8 bounces / 1 spp: contract {rates['contract']:.0f} Msamples/s, reference {rates['reference']:.0f} Msamples/s "
          f"({rates['contract'] / rates['reference']:.1f}x)")
    assert all(math.isfinite(r) and r > 0 for r in rates.values())
