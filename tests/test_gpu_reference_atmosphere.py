"""pt_atmosphere_set_arithmetic(h, PT_ARITH_REFERENCE) on the GPU: atmo_precompute_reference_kernel (csrc/pt_integrate_reference.hip,
csrc/pt_atmosphere_reference.hpp) computes the cube the oracle computes with llvmpipe's arithmetic choices (witness build, base variant
951) BIT FOR BIT, and is therefore within 1e-4 of the reference's own cubes on every texel, where the contract kernel's frozen marks are
99.3 / 97.5 / 99.6 % of the texels.  The switch is independent of pt_set_arithmetic and sticky; together the two switches render the
reference's start-up sequence (MainWindow.OnLoad) in the reference's arithmetic end to end."""
import math

import numpy as np
import pytest

import __graft_entry__ as graft
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
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} texels / pixels differ from the oracle; first at {np.argwhere(bad)[:5].tolist()}")


@pytest.fixture(scope="module")
def ref_oracle():
    import __graft_entry__ as graft
    o = graft.load_oracle().Oracle(perturb=True)
    o.set_base_variant(LLVMPIPE)
    yield o
    o.set_base_variant(0)


@pytest.fixture
def pt(pkg, native_lib):
    t = pkg.PathTracer(None, 16, 16, 1, 1, 1.0, 0.0)
    yield t
    t.Dispose()


def hip_cube(pkg, pt, size, ubo, lp, intensity=15.0, isteps=50, jsteps=15, mode=1):
    at = pkg.AtmosphericScatterer(size, ubo, lp, pt)
    at.ISteps, at.JSteps, at.LightIntensity = isteps, jsteps, intensity
    at.SetArithmetic(mode)
    pt.EnvironmentMap = at  # (renders)
    return at.Result


def fixture_case(name):
    fx = fixtures.load(name)
    size, isteps, jsteps = (int(v) for v in fx["params"])
    return fx, (size, fx["ubo"].tobytes(), np.asarray(fx["light_pos"], np.float32), float(fx["intensity"]), isteps, jsteps)


# ------------------------------------------------------------------------------------------------ (4) bit-exact with the oracle at 951
@pytest.mark.parametrize("name", ["atmo_24_few_steps", "atmo_32_default", "atmo_48_noon"])
def test_reference_mode_equals_oracle_951_on_the_fixtures(pkg, pt, ref_oracle, name):
    assert name in fixtures.names("atmo_")
    _, case = fixture_case(name)
    got = hip_cube(pkg, pt, *case)
    assert (got[..., 3] == 1.0).all()
    assert_bit_exact(got, ref_oracle.atmosphere(*case, threads=16), name)


@pytest.mark.parametrize("what,size,t,sun_x,intensity,isteps,jsteps", [
    ("odd size", 33, 0.3, None, 15.0, 50, 15),
    ("whole wavefronts outside the grid", 512, 0.5, None, 15.0, 50, 15),
    ("sun off the plane x = 0", 96, 0.4, 3.0e10, 15.0, 50, 15),
    ("one step each", 64, 0.52, None, 22.0, 1, 1),
    ("one sun-ray step", 40, 0.25, None, 15.0, 9, 1),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_reference_mode_equals_oracle_951_shapes_and_extremes(pkg, pt, ref_oracle, what, size, t, sun_x, intensity, isteps, jsteps):
    ubo = pkg.camera.atmospheric_data_ubo()
    lp = np.array(pkg.camera.atmosphere_light_pos(t), dtype=np.float32)
    if sun_x is not None:
        lp[0] = sun_x
    got = hip_cube(pkg, pt, size, ubo, lp, intensity, isteps, jsteps)
    assert_bit_exact(got, ref_oracle.atmosphere(size, ubo, lp, intensity, isteps, jsteps, threads=16), what)


def test_reference_mode_rerender_with_changed_parameters_and_2048(pkg, pt, ref_oracle):
    """The GUI's knobs on one handle (Gui.cs:89-145): re-rendering with changed parameters == a fresh computation; the largest size the
    GUI offers runs, is finite everywhere and has alpha 1."""
    ubo = pkg.camera.atmospheric_data_ubo()
    at = pkg.AtmosphericScatterer(128, ubo, pkg.camera.atmosphere_light_pos(0.5), pt)
    at.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
    pt.EnvironmentMap = at
    first = at.Result
    at.LightPos = pkg.camera.atmosphere_light_pos(0.15)
    at.LightIntensity, at.ISteps, at.JSteps = 22.0, 30, 8
    at.Render()
    changed = at.Result
    want = ref_oracle.atmosphere(128, ubo, pkg.camera.atmosphere_light_pos(0.15), 22.0, 30, 8, threads=16)
    assert_bit_exact(changed, want, "re-render with changed parameters")
    assert not np.array_equal(bits(changed), bits(first))
    at.Size, at.ISteps, at.JSteps = 2048, 50, 15
    pt.TimerBegin()
    at.Render()
    ms = pt.TimerEnd()
    big = at.Result
    assert big.shape == (6, 2048, 2048, 4) and np.isfinite(big).all() and (big[..., 3] == 1).all() and 0.0 < ms < 10000.0


# ------------------------------------------------------------------------------------------------ (5) within 1e-4 of the reference everywhere
@pytest.mark.parametrize("name", ["atmo_24_few_steps", "atmo_32_default", "atmo_48_noon"])
def test_reference_mode_within_1e4_of_the_reference_everywhere(pkg, pt, name):
    fx, case = fixture_case(name)
    got = hip_cube(pkg, pt, *case)
    err = tol.atmo_error(fx["expected"], got[..., :3])
    share = float((err < 1e-4).mean())
    print(f"\n  {name}: worst texel {err.max():.3g}, median {np.median(err):.3g}, share within 1e-4 {share:.4f} "
          f"(frozen contract mark {tol.ATMO_MARKS[name][1]})")
    assert err.max() < 1e-4 and share == 1.0, f"{name}: worst {err.max():.3g}, share {share:.4f}"


# ------------------------------------------------------------------------------------------------ (6) the switch
def test_the_switch_is_independent_and_sticky(pkg, native_lib, pt, oracle, ref_oracle):
    N = pkg.native
    _, case = fixture_case("atmo_32_default")
    contract, reference = oracle.atmosphere(*case, threads=16), ref_oracle.atmosphere(*case, threads=16)
    assert not np.array_equal(bits(contract), bits(reference))
    lp = np.ascontiguousarray(case[2], np.float32)

    def render_raw():  # pt_atmosphere_render alone: whatever mode the handle holds
        buf = np.frombuffer(case[1], dtype=np.uint8)
        N.check(native_lib.pt_atmosphere_upload_data(pt._h, 0, buf.nbytes, buf.ctypes.data), pt._h)
        N.check(native_lib.pt_atmosphere_render(pt._h, case[0], case[4], case[5], lp.ctypes.data_as(native_lib.pt_atmosphere_render.argtypes[4]),
                                                case[3]), pt._h)
        return pt.ReadEnvironment()

    assert_bit_exact(render_raw(), contract, "default mode before")
    assert native_lib.pt_atmosphere_set_arithmetic(pt._h, N.PT_ARITH_REFERENCE) == N.PT_OK
    assert_bit_exact(pt.ReadEnvironment(), contract, "the switch does not touch the current environment")
    assert_bit_exact(render_raw(), reference, "reference mode")
    assert_bit_exact(render_raw(), reference, "reference mode is sticky")
    # pt_set_arithmetic in either state changes neither the cube that exists nor the next one
    pt.SetArithmetic(N.PT_ARITH_REFERENCE)
    assert_bit_exact(pt.ReadEnvironment(), reference, "pt_set_arithmetic(REFERENCE) leaves the cube")
    assert_bit_exact(render_raw(), reference, "pt_set_arithmetic(REFERENCE), atmosphere still in reference mode")
    pt.SetArithmetic(N.PT_ARITH_CONTRACT)
    assert_bit_exact(render_raw(), reference, "pt_set_arithmetic(CONTRACT), atmosphere still in reference mode")
    # bad modes are rejected and leave the mode in force
    for bad in (2, -1):
        assert native_lib.pt_atmosphere_set_arithmetic(pt._h, bad) == N.PT_E_BAD_ARGUMENT
    assert_bit_exact(render_raw(), reference, "after rejected modes: still reference")
    assert native_lib.pt_atmosphere_set_arithmetic(pt._h, N.PT_ARITH_CONTRACT) == N.PT_OK
    pt.SetArithmetic(N.PT_ARITH_REFERENCE)
    assert_bit_exact(render_raw(), contract, "contract mode after, with pt_set_arithmetic(REFERENCE)")
    for bad in (2, -1):
        assert native_lib.pt_atmosphere_set_arithmetic(pt._h, bad) == N.PT_E_BAD_ARGUMENT
        assert native_lib.pt_set_arithmetic(pt._h, bad) == N.PT_E_BAD_ARGUMENT
    assert_bit_exact(render_raw(), contract, "after rejected modes: still contract")


def test_the_mode_travels_with_the_scatterer(pkg, native_lib, ref_oracle):
    """AtmosphericScatterer.SetArithmetic is remembered on the object and applied before each Render(): re-attached to a fresh tracer
    (whose handle is in the default mode) it still renders in reference arithmetic."""
    _, case = fixture_case("atmo_24_few_steps")
    want = ref_oracle.atmosphere(*case, threads=16)
    a, b = pkg.PathTracer(None, 16, 16, 1, 1, 1.0, 0.0), pkg.PathTracer(None, 16, 16, 1, 1, 1.0, 0.0)
    at = pkg.AtmosphericScatterer(case[0], case[1], case[2], a)
    at.ISteps, at.JSteps, at.LightIntensity = case[4], case[5], case[3]
    at.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
    a.EnvironmentMap = at
    assert_bit_exact(a.ReadEnvironment(), want, "first tracer")
    b.EnvironmentMap = at
    assert_bit_exact(b.ReadEnvironment(), want, "second tracer")
    a.Dispose()
    b.Dispose()


# ------------------------------------------------------------------------------------------------ (7) end to end
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["single", "group_0_0"])
def test_startup_sequence_in_reference_arithmetic(pkg, native_lib, ref_oracle, devices):
    """MainWindow.OnLoad (MainWindow.cs:174-189,203) as tests/test_gpu_parity.py's test_default_startup_sequence, with both switches on:
    atmosphere cube at 256 in reference arithmetic -> PathTracer(env = atmosphere, rayDepth 13, spp 1, f 20, aperture 0.14) in reference
    arithmetic -> LoadScene -> two frames == the oracle at 951 fed with the cube the oracle at 951 computed."""
    W, H = 208, 208
    sc, cam = pkg.scene.default_scene(), pkg.camera.Camera()
    basic = pkg.camera.basic_data_ubo(cam, W, H)
    ubo, lp = pkg.camera.atmospheric_data_ubo(), pkg.camera.atmosphere_light_pos(0.5)
    extra = {} if devices is None else {"devices": devices}
    pt = pkg.PathTracer(None, W, H, 13, 1, 20.0, 0.14, **extra)
    at = pkg.AtmosphericScatterer(256, ubo, lp, pt)
    at.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
    pt.EnvironmentMap = at
    pt.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)
    pt.UploadScene(sc)
    pt.UploadBasicData(basic)
    pt.Render()
    pt.Render()
    got, cube = pt.Result, pt.ReadEnvironment()
    pt.Dispose()
    env = ref_oracle.atmosphere(256, ubo, lp, threads=16)
    assert_bit_exact(cube, env, "atmosphere 256")
    want = ref_oracle.render(W, H, basic, sc.ubo_bytes(), env, num_spheres=48, num_cuboids=7, ray_depth=13, num_frames=2, threads=16)
    assert_bit_exact(got, want, "startup sequence in reference arithmetic")


# ------------------------------------------------------------------------------------------------ (9) cost
def test_cost_of_both_modes(pkg, pt):
    """2048^2 x 6 texels, 50 x 15 steps: GPU milliseconds of both kernels through pt_timer_* (fastest of three; printed, recorded in
    DESIGN.md section 4.1)."""
    ubo, lp = pkg.camera.atmospheric_data_ubo(), pkg.camera.atmosphere_light_pos(0.5)
    ms = {}
    for mode, label in ((pkg.native.PT_ARITH_CONTRACT, "contract"), (pkg.native.PT_ARITH_REFERENCE, "reference")):
        at = pkg.AtmosphericScatterer(2048, ubo, lp, pt)
        at.SetArithmetic(mode)
        pt.EnvironmentMap = at  # (renders once: allocation, code object load)
        times = []
        for _ in range(3):
            pt.TimerBegin()
            at.Render()
            times.append(pt.TimerEnd())
        ms[label] = min(times)
    print(f"\n  atmosphere 2048^2, 50 x 15 steps: contract {ms['contract']:.2f} ms, reference {ms['reference']:.2f} ms "
          f"({ms['reference'] / ms['contract']:.2f}x)")
    assert all(math.isfinite(v) and v > 0 for v in ms.values())
