"""Adaptive sampling on the GPU (pt_adaptive_set_params / pt_adaptive_render / pt_adaptive_status / pt_adaptive_read_tiles /
pt_adaptive_read_noise; pt_adaptive_kernel in csrc/pt_adaptive.hip) against its definition: after any number of passes every tile's
pixels equal the uniform image U_k of the tile's own count k bit for bit, and the tile records and the per-pixel (M2, e) equal the numpy
float32 restatement (tests/adaptive_reference.py; its own properties: tests/test_adaptive_cpu.py) fed with the uniform images a second
handle rendered with pt_render; passes over a finished image write nothing; a changed threshold takes effect at once; tilings; the
rules of a live state; the argument checks; quality (asserted) and cost (measured), both recorded in DESIGN.md 3.5."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import adaptive_reference as ar
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
F32 = np.float32
K, MIN, MAX = 24, 4, 24
LOOKS = (3, 9, 26)  # passes after which everything is compared


@dataclass(frozen=True)
class ACase:
    name: str
    case: fh.Case
    F: int = 0
    spp: int = 1
    tiling: tuple = ()


def _d43(ap):
    return fh.Case(f"default_43x27_ap{ap}", "default", 43, 27, aperture=ap)


CASES = [ACase(f"43x27_F{F}_spp{spp}_ap{ap}", _d43(ap), F, spp) for F in (0, 5) for spp in (1, 3) for ap in (0.0, 0.14)] + [
    ACase("75x43", fh.BY_NAME["default_75x43_f0"]),
    ACase("8x8", fh.BY_NAME["default_8x8"]),
    ACase("1x1", fh.BY_NAME["default_1x1"]),
    ACase("stress256_16x16", fh.Case("stress256_16x16", "stress256", 16, 16)),  # (its uniform frames come from the sphere-grid kernel)
]
TILED = [ACase("43x27_tile_8_16", _d43(0.14), tiling=("tile", 8, 16)), ACase("43x27_interleaved_1_2_8", _d43(0.14), tiling=("interleaved", 1, 2, 8))]
NON_VACUOUS = [c.name for c in CASES if c.name.startswith(("43x27", "75x43"))]
BY = {c.name: c for c in CASES + TILED}

_env = None
_uniform = {}
_runs = {}


def env():
    global _env
    if _env is None:
        _env = pkg.envmap.synthetic_sky_rgba32f(32)
    return _env


def same(a, b):
    """bit for bit, NaN == NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def tracer(ac, tiled=True):
    pt = fh.make_tracer(ac.case, env=env(), ray_depth=8)
    if ac.spp != 1:
        pt.SPP = ac.spp
    if tiled and ac.tiling:
        if ac.tiling[0] == "tile":
            pt.SetTile(*ac.tiling[1:])
        else:
            pt.SetInterleavedTile(*ac.tiling[1:])
    return pt


def local_rows(ac):
    """the image rows the handle of the case owns, in the order it stores them"""
    h = ac.case.height
    if not ac.tiling:
        return list(range(h))
    if ac.tiling[0] == "tile":
        return list(range(ac.tiling[1], ac.tiling[1] + ac.tiling[2]))
    rank, world, band = ac.tiling[1:]
    return [y for y in range(h) if (y // band) % world == rank]


def uniform(ac):
    """U_0 .. U_K of the whole image: read back after each of K pt_render frames on a handle of its own.  Made once, never changed."""
    key = (ac.case, ac.spp)
    if key not in _uniform:
        pt = tracer(ac, tiled=False)
        U = [pt.Result.copy()]
        for _ in range(K):
            pt.Render()
            U.append(pt.Result.copy())
        pt.Dispose()
        U = np.stack(U)
        U.setflags(write=False)
        _uniform[key] = U
    return _uniform[key]


def look(pt):
    return dict(image=pt.Result.copy(), tiles=pt.AdaptiveTiles(), e=pt.AdaptiveNoise(), m2=N.debug_adaptive_m2(pt._h, pt.rows, pt.Width),
                status=pt.AdaptiveStatus(), frame=pt.FrameIndex)


def want(sim, U, thr, spp):
    m2, e = sim.stats()
    return dict(image=sim.image(U), tiles=sim.records(), e=e, m2=m2, status=sim.status(thr, MIN, MAX, spp), counts=sim.k.copy())


def run(ac):
    """One handle through the whole sequence, with the restatement beside it: F pt_render frames, then 3 / 9 / 26 passes, two more, two
    with the threshold lowered to 0, three with it raised to FLT_MAX.  -> {step: (got, want)}, thr, the local U."""
    if ac.name in _runs:
        return _runs[ac.name]
    U = uniform(ac)[:, local_rows(ac)]
    table = ar.tabulate(U, ac.F)
    thr = ar.median_threshold(table, 8)
    pt = tracer(ac)
    assert pt.rows == U.shape[1]
    for _ in range(ac.F):
        pt.Render()
    pt.SetAdaptive(float(thr), MIN, MAX)
    sim = ar.Sim(table)
    steps, done = {}, 0
    for p in LOOKS:
        pt.RenderAdaptive(p - done)
        sim.run(p - done, thr, MIN, MAX)
        done = p
        steps[p] = (look(pt), want(sim, U, thr, ac.spp))
    pt.RenderAdaptive(2)
    steps["idle"] = (look(pt), want(sim.run(2, thr, MIN, MAX), U, thr, ac.spp))
    pt.SetAdaptive(0.0, MIN, MAX)
    steps["zero_status"] = (pt.AdaptiveStatus(), sim.status(F32(0.0), MIN, MAX, ac.spp))
    pt.RenderAdaptive(2)
    steps["zero"] = (look(pt), want(sim.run(2, F32(0.0), MIN, MAX), U, F32(0.0), ac.spp))
    pt.SetAdaptive(float(ar.FLT_MAX), MIN, MAX)
    pt.RenderAdaptive(3)
    steps["max"] = (look(pt), want(sim.run(3, ar.FLT_MAX, MIN, MAX), U, ar.FLT_MAX, ac.spp))
    pt.Dispose()
    _runs[ac.name] = (steps, thr, U)
    return _runs[ac.name]


def assert_look(got, exp, what):
    assert same(got["image"], exp["image"]).all(), f"{what}: image, {(~same(got['image'], exp['image'])).any(-1).sum()} pixels differ"
    for f in ("k", "k0", "n"):
        assert (got["tiles"][f] == exp["tiles"][f]).all(), (what, f, got["tiles"][f], exp["tiles"][f])
    assert same(got["tiles"]["err"], exp["tiles"]["err"]).all(), (what, got["tiles"]["err"], exp["tiles"]["err"])
    assert same(got["m2"], exp["m2"]).all(), f"{what}: M2, {(~same(got['m2'], exp['m2'])).sum()} pixels differ"
    assert same(got["e"], exp["e"]).all(), f"{what}: e, {(~same(got['e'], exp['e'])).sum()} pixels differ"
    assert got["status"] == exp["status"], (what, got["status"], exp["status"])


@pytest.mark.parametrize("name", NON_VACUOUS)
def test_expected_counts_are_not_vacuous(name):
    steps, _, _ = run(BY[name])
    counts = steps[26][1]["counts"]
    assert ar.non_vacuous(counts, MIN, MAX), np.unique(counts)


@pytest.mark.parametrize("name", [c.name for c in CASES + TILED])
def test_every_tile_shows_its_own_uniform_image(name):
    """check 1 (and 5 for the tiled handles): after 26 passes a tile's pixels are U_count of that tile, bit for bit"""
    ac = BY[name]
    steps, _, U = run(ac)
    got, exp = steps[26]
    counts = np.repeat(np.repeat(got["tiles"]["k"], 8, 0), 8, 1)[:U.shape[1], :U.shape[2]]
    mine = np.take_along_axis(np.asarray(U), counts[None, :, :, None], 0)[0]  # by the handle's OWN counts ...
    assert same(got["image"], mine).all()
    assert (got["tiles"]["k"] == exp["counts"]).all()                           # ... which are the expected ones
    assert (got["image"][..., 3] == 1).all() and got["frame"] == ac.F


@pytest.mark.parametrize("name", [c.name for c in CASES + TILED])
@pytest.mark.parametrize("passes", LOOKS)
def test_records_and_statistics_equal_the_restatement(name, passes):
    """check 2: tile records, per-pixel (M2, e), the image and pt_adaptive_status after 3, 9 and 26 passes"""
    steps, _, _ = run(BY[name])
    assert_look(*steps[passes], f"{name} after {passes} passes")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_passes_over_a_finished_image_write_nothing(name):
    """check 3: two more passes; image, records and statistics are bit-equal"""
    steps, _, _ = run(BY[name])
    before, after = steps[26][0], steps["idle"][0]
    assert before["status"]["active_tiles"] == 0
    for f in ("image", "tiles", "e", "m2"):
        assert before[f].tobytes() == after[f].tobytes(), f
    assert_look(*steps["idle"], name)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_a_changed_threshold_takes_effect_at_once(name):
    """check 4: thr = 0 reactivates every tile below max (with a positive err), the passes follow the restatement; +FLT_MAX stops
    every tile that has min samples"""
    ac = BY[name]
    steps, _, _ = run(ac)
    got, exp = steps["zero_status"]
    assert got == exp
    rec = steps["idle"][0]["tiles"]
    assert got["active_tiles"] == int(((rec["k"] < MAX) & (rec["err"] > 0)).sum())
    if name in NON_VACUOUS:
        assert got["active_tiles"] > 0
    assert_look(*steps["zero"], f"{name}, thr = 0")
    moved = steps["zero"][0]["tiles"]["k"] - rec["k"]
    assert (moved[(rec["k"] < MAX) & (rec["err"] > 0)] >= 1).all() and (moved[(rec["k"] == MAX) | ~(rec["err"] > 0)] == 0).all()
    assert_look(*steps["max"], f"{name}, thr = FLT_MAX")
    last = steps["max"][0]
    assert last["status"]["active_tiles"] == 0
    assert (last["tiles"]["k"] == steps["zero"][0]["tiles"]["k"]).all()  # (every tile had min samples already: none moved)


@pytest.mark.parametrize("F", (0, 5))
def test_flt_max_stops_every_tile_at_min_samples(F):
    """check 4, second half, from a fresh state: under thr = +FLT_MAX a tile runs until it has min samples since k0 and no further"""
    ac = BY[f"43x27_F{F}_spp1_ap0.14"]
    pt = tracer(ac)
    for _ in range(F):
        pt.Render()
    pt.SetAdaptive(float(ar.FLT_MAX), MIN, MAX)
    pt.RenderAdaptive(10)
    rec, image = pt.AdaptiveTiles(), pt.Result
    pt.Dispose()
    k0 = max(F, 1)
    assert (rec["k"] == k0 + MIN - 1).all() and (rec["k0"] == k0).all()
    assert image.tobytes() == uniform(ac)[k0 + MIN - 1].tobytes()


def test_tiles_equal_the_cpu_oracle_directly(oracle):
    """check 1, second half: the tiles of two distinct counts against oracle frames rendered here, not against the GPU's uniform images"""
    ac = BY["43x27_F0_spp1_ap0.14"]
    steps, _, _ = run(ac)
    got = steps[26][0]
    counts = got["tiles"]["k"]
    values = np.unique(counts)
    assert len(values) >= 2
    blob, ns, nc, basic = fh.inputs(ac.case)
    for k in (values[0], values[-2]):
        img = oracle.render(ac.case.width, ac.case.height, basic, blob, env(), num_spheres=ns, num_cuboids=nc, ray_depth=8, spp=1,
                            focal_length=ac.case.focal_length, aperture=ac.case.aperture, num_frames=int(k))
        for ty, tx in zip(*np.nonzero(counts == k)):
            sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
            assert same(got["image"][sl], img[sl]).all(), (k, ty, tx)


def test_live_state_rules():
    """check 6"""
    ac = BY["43x27_F5_spp1_ap0.14"]
    fp = C.POINTER(C.c_float)
    pt = tracer(ac)
    pt.SetAdaptive(5e-4, MIN, MAX)  # (alone: changes nothing pt_render produces)
    for _ in range(5):
        pt.Render()
    assert pt.Result.tobytes() == uniform(ac)[5].tobytes()
    pt.RenderAdaptive(6)
    before = look(pt)
    assert before["frame"] == 5 and len(np.unique(before["tiles"]["k"])) >= 2
    total = C.c_int(-7)
    assert pt._lib.pt_render(pt._h, C.byref(total)) == N.PT_E_BAD_ARGUMENT and total.value == -7
    assert b"adaptive accumulation in progress: pt_reset first" in pt._lib.pt_last_error(pt._h)
    pt.SetDenoiseTemporal(True)
    assert pt._lib.pt_denoise_render(pt._h, 0) == N.PT_E_BAD_ARGUMENT
    pt.SetDenoiseTemporal(False)
    pt.SetDenoiseMoments(True)
    assert pt._lib.pt_denoise_render(pt._h, 0) == N.PT_E_BAD_ARGUMENT
    pt.SetDenoiseMoments(False)
    after = look(pt)
    for f in ("image", "tiles", "e", "m2"):
        assert before[f].tobytes() == after[f].tobytes(), f
    assert after["frame"] == 5 and after["status"] == before["status"]
    # whatever only reads the image works unchanged: against a second handle given the same image through pt_write_result
    twin = tracer(ac)
    twin.WriteResult(before["image"], 5)
    assert pt.Present().tobytes() == twin.Present().tobytes()
    assert pt.Denoise(0).tobytes() == twin.Denoise(0).tobytes()                      # the fixed mode
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
    twin.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
    assert pt.Denoise(0).tobytes() == twin.Denoise(0).tobytes()                      # the variance mode
    assert pt.FirstHit(3).tobytes() == twin.FirstHit(3).tobytes()
    assert look(pt)["image"].tobytes() == before["image"].tobytes()
    # the state ends with the reset epoch, and with pt_bind_result_buffer
    pt.ResetRenderer()
    assert pt._lib.pt_adaptive_status(pt._h, None, None, None, None, None) == N.PT_E_BAD_ARGUMENT
    buf = np.empty((pt.rows, pt.Width), F32)
    assert pt._lib.pt_adaptive_read_noise(pt._h, buf.ctypes.data_as(fp), 0) == N.PT_E_BAD_ARGUMENT
    assert pt._lib.pt_adaptive_read_tiles(pt._h, buf.ctypes.data_as(C.c_void_p)) == N.PT_E_BAD_ARGUMENT
    for _ in range(8):
        pt.Render()
    assert pt.Result.tobytes() == uniform(ac)[8].tobytes() and pt.FrameIndex == 8   # (a fresh handle's eight frames)
    pt.RenderAdaptive(1)
    assert pt.AdaptiveStatus()["min_count"] == 9
    pt.BindResultBuffer(None)
    assert pt._lib.pt_adaptive_status(pt._h, None, None, None, None, None) == N.PT_E_BAD_ARGUMENT
    twin.WriteResult(before["image"], 5)
    twin.RenderAdaptive(1)
    twin.SetSize(43, 27)
    assert twin._lib.pt_adaptive_status(twin._h, None, None, None, None, None) == N.PT_E_BAD_ARGUMENT
    twin.Render()
    pt.Dispose()
    twin.Dispose()


def test_argument_checks():
    """check 7"""
    ac = BY["8x8"]
    pt = tracer(ac)
    L, h = pt._lib, pt._h
    bad, oor = N.PT_E_BAD_ARGUMENT, N.PT_E_OUT_OF_RANGE
    for thr in (float("nan"), float("inf"), -float("inf"), -1e-30):
        assert L.pt_adaptive_set_params(h, thr, 8, 1024) == bad
    for mn, mx in ((1, 8), (0, 8), (-3, 8), (65536, 65536), (8, 7), (8, 65536), (2, 1)):
        assert L.pt_adaptive_set_params(h, 1e-4, mn, mx) == oor, (mn, mx)
    for mn, mx in ((2, 2), (2, 65535), (65535, 65535)):
        assert L.pt_adaptive_set_params(h, 0.0, mn, mx) == N.PT_OK
    assert L.pt_adaptive_set_params(h, float(ar.FLT_MAX), 8, 1024) == N.PT_OK
    # without a live state
    buf = np.empty((pt.rows, pt.Width), F32)
    fp = C.POINTER(C.c_float)
    assert L.pt_adaptive_status(h, None, None, None, None, None) == bad
    assert L.pt_adaptive_read_tiles(h, buf.ctypes.data_as(C.c_void_p)) == bad
    assert L.pt_adaptive_read_noise(h, buf.ctypes.data_as(fp), 0) == bad
    for passes in (0, -1, 65536):
        assert L.pt_adaptive_render(h, passes) == oor
    pt.SetArithmetic(N.PT_ARITH_REFERENCE)
    assert L.pt_adaptive_render(h, 1) == bad
    pt.SetArithmetic(N.PT_ARITH_CONTRACT)
    assert L.pt_adaptive_status(h, None, None, None, None, None) == bad  # (the refused calls started nothing)
    # the defaults: a failed set leaves the previous values in force
    pt.SetAdaptive(0.25, 3, 5)
    assert L.pt_adaptive_set_params(h, float("nan"), 2, 2) == bad and L.pt_adaptive_set_params(h, 0.0, 1, 2) == oor
    pt.RenderAdaptive(7)
    st = pt.AdaptiveStatus()
    assert st["tiles"] == 1 and st["min_count"] == st["max_count"] and 3 <= st["max_count"] <= 5 and st["pixel_samples"] == 64 * st["max_count"]
    # NULL rules and pitches with a live state
    assert L.pt_adaptive_status(h, None, None, None, None, None) == N.PT_OK
    one = C.c_int(-1)
    assert L.pt_adaptive_status(h, None, C.byref(one), None, None, None) == N.PT_OK and one.value == 1
    assert L.pt_adaptive_read_tiles(h, None) == bad
    assert L.pt_adaptive_read_noise(h, None, 0) == bad
    assert L.pt_adaptive_read_noise(h, buf.ctypes.data_as(fp), 31) == bad
    wide = np.full((8, 10), -1.0, F32)
    assert L.pt_adaptive_read_noise(h, wide.ctypes.data_as(fp), 40) == N.PT_OK
    assert (wide[:, 8:] == -1).all() and wide[:, :8].tobytes() == pt.AdaptiveNoise().tobytes()
    pt.Dispose()
    # no environment; a group handle
    bare = fh.make_tracer(ac.case, env=None, ray_depth=8)
    assert bare._lib.pt_adaptive_render(bare._h, 1) == N.PT_E_NO_ENVIRONMENT
    bare.Dispose()
    group = fh.make_tracer(_d43(0.14), devices=[0, 0])
    assert group._lib.pt_adaptive_render(group._h, 1) == bad
    assert group._lib.pt_adaptive_set_params(group._h, 1e-4, 8, 1024) == bad
    assert group._lib.pt_adaptive_status(group._h, None, None, None, None, None) == bad
    group.Dispose()


def _u(img):
    l = ar.lum(img).astype(np.float64)
    return l / (1.0 + l)


def test_quality_and_cost_are_recorded():
    """check 8.  Default scene, 160x90, aperture 0, depth 8; truth = the handle's 1024-frame image.  The adaptive run: the defaults with
    max_samples = 256, from frame 0, until no tile is active.  Asserted: mean samples per pixel < 256, and the MSE of u against the truth
    below the uniform image's at min_samples frames.  Printed (recorded in DESIGN.md 3.5): the equal-budget comparison, the grid of
    thresholds behind the default, and at 1920x1080 the cost of one pass with every tile active against one variant-1 frame on the same
    handle, and of one pass with no tile active (pt_timer_*, fastest of three)."""
    case = fh.Case("default_160x90_ap0", "default", 160, 90, aperture=0.0)
    ref = fh.make_tracer(case, env=env(), ray_depth=8)
    for _ in range(1024):
        ref.Render()
    truth = _u(ref.Result)
    ref.Dispose()

    def uniform_mse(frames):
        pt = fh.make_tracer(case, env=env(), ray_depth=8)
        for _ in range(frames):
            pt.Render()
        mse = float(((_u(pt.Result) - truth) ** 2).mean())
        pt.Dispose()
        return mse

    lines = []
    results = {}
    for thr in (1e-3, 1e-4, 1e-5):
        pt = fh.make_tracer(case, env=env(), ray_depth=8)
        pt.SetAdaptive(thr, ar.DEFAULT_MIN, 256)
        for _ in range(256 // 4 + 1):
            pt.RenderAdaptive(4)
            st = pt.AdaptiveStatus()
            if st["active_tiles"] == 0:
                break
        assert st["active_tiles"] == 0
        mean = st["pixel_samples"] / (160 * 90)
        mse = float(((_u(pt.Result) - truth) ** 2).mean())
        budget = int(np.ceil(mean))
        same_budget = uniform_mse(budget)
        results[thr] = (mean, mse, same_budget)
        lines.append(f"adaptive quality 160x90: thr {thr:g}: mean samples/pixel {mean:.2f} (counts {st['min_count']}..{st['max_count']}), MSE(u) {mse:.4e}; "
                     f"uniform at {budget} frames {same_budget:.4e} (ratio {same_budget / mse:.3f})")
        pt.Dispose()
    at_min = uniform_mse(ar.DEFAULT_MIN)
    lines.append(f"adaptive quality 160x90: uniform at min_samples = {ar.DEFAULT_MIN} frames: MSE(u) {at_min:.4e}")

    big = fh.Case("default_1080p_ap0", "default", 1920, 1080, aperture=0.0)
    pt = fh.make_tracer(big, env=env(), ray_depth=8)
    pt.SetVariant(1)
    pt.Render()
    pt.Render()

    def fastest(fn):
        ms = []
        for _ in range(3):
            pt.Synchronize()
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)
    times = {"one pt_set_variant(h, 1) frame": fastest(pt.Render)}
    pt.SetAdaptive(0.0, 65535, 65535)  # (every tile is short of min_samples)
    pt.RenderAdaptive(2)  # (buffers allocated, code loaded)
    assert pt.AdaptiveStatus()["active_tiles"] == pt.AdaptiveStatus()["tiles"] == 240 * 135
    times["one pass, every tile active"] = fastest(lambda: pt.RenderAdaptive(1))
    pt.SetAdaptive(float(ar.FLT_MAX), 2, 65535)
    assert pt.AdaptiveStatus()["active_tiles"] == 0
    times["one pass, no tile active"] = fastest(lambda: pt.RenderAdaptive(1))
    pt.Dispose()
    lines += [f"adaptive cost 1080p: {k} {v:.4f} ms" for k, v in times.items()]
    print("\n  " + "\n  ".join(lines))
    mean, mse, _ = results[1e-4]
    assert mean < 256
    assert mse < at_min
    assert all(v > 0 for v in times.values())
