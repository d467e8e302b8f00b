"""The adaptive sampler's noise as the denoiser's noise source on the GPU (pt_denoise_set_adaptive_noise / pt_denoise_read_variance_used;
pt_adaptive_blend_kernel in csrc/pt_denoise_adaptive.hip) against its definition: on a live adaptive state var_0 and the denoised image
equal the numpy float32 restatement (tests/denoise_adaptive_reference.py; its own properties: tests/test_denoise_adaptive_cpu.py) fed
with the handle's own tile records, per-pixel estimate, V0 and guides, on every pixel, bit for bit; wherever stage A does not run the
result is what it is with the switch off; the stage writes neither the adaptive state nor the image; the argument checks; the read-out
of stage B's var_0; quality against the variance mode (asserted) and cost (measured), both recorded in DESIGN.md 3.5."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import adaptive_reference as ar
import denoise_adaptive_reference as da
import denoise_lens_reference as dl
import denoise_moments_reference as dm
import denoise_reference as dr
import denoise_variance_reference as dv
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
F32 = np.float32
DEFAULTS = dr.Params()
SIGMA = dv.DEFAULT_SIGMA_VARIANCE
K, MIN, MAX, PASSES = 24, 4, 24, 26  # the schedule of tests/test_gpu_adaptive.py
PRIOR = da.DEFAULT_PRIOR_SAMPLES


@dataclass(frozen=True)
class DCase:
    name: str
    case: fh.Case
    F: int = 0
    spp: int = 1
    lens: bool = False


def _default(w, h, ap):
    return fh.Case(f"default_{w}x{h}_ap{ap}", "default", w, h, aperture=ap)


CASES = [
    DCase("43x27_ap0", _default(43, 27, 0.0)),
    DCase("43x27_ap0.14_lens", _default(43, 27, 0.14), lens=True),
    DCase("43x27_F5_spp3", _default(43, 27, 0.0), F=5, spp=3),
    DCase("37x19", _default(37, 19, 0.0)),  # ragged 8x8 and 16x16 tiles
    DCase("8x8", fh.BY_NAME["default_8x8"]),
    DCase("1x1", fh.BY_NAME["default_1x1"]),
]
NON_VACUOUS = [c.name for c in CASES if c.name.startswith(("43x27", "37x19"))]
BY = {c.name: c for c in CASES}

_env = None
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


def tracer(dc, variance=True, params=DEFAULTS):
    pt = fh.make_tracer(dc.case, env=env(), ray_depth=8)
    if dc.spp != 1:
        pt.SPP = dc.spp
    pt.SetDenoise(params.iterations, params.sigma_color, params.sigma_plane, params.normal_log2_power)
    if variance:
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
    if dc.lens:
        pt.SetDenoiseLens(True, dl.DEFAULT_COC_SCALE)
    return pt


def coc_k(dc):
    if not dc.lens:
        return dr.F(0.0)
    m5 = np.frombuffer(fh.inputs(dc.case)[3], np.float32)[5]
    return dl.cock_of(dl.DEFAULT_COC_SCALE, dc.case.aperture, dc.case.focal_length, dc.case.height, m5)


def uniform(dc):
    """U_0 .. U_K: read back after each of K pt_render frames on a handle of its own"""
    pt = tracer(dc)
    U = [pt.Result.copy()]
    for _ in range(K):
        pt.Render()
        U.append(pt.Result.copy())
    pt.Dispose()
    return np.stack(U)


def look(pt):
    return dict(image=pt.Result.copy(), tiles=pt.AdaptiveTiles(), e=pt.AdaptiveNoise(), m2=N.debug_adaptive_m2(pt._h, pt.rows, pt.Width))


def used_refused(pt):
    buf = np.empty((pt.rows, pt.Width), F32)
    rc = pt._lib.pt_denoise_read_variance_used(pt._h, buf.ctypes.data_as(C.POINTER(C.c_float)), 0)
    assert rc in (N.PT_OK, N.PT_E_BAD_ARGUMENT)
    return rc == N.PT_E_BAD_ARGUMENT


def adaptive_handle(dc, **kw):
    """-> (the handle after F pt_render frames and 26 passes under the median threshold, the restatement's replay beside it, U, thr)"""
    U = uniform(dc)
    table = ar.tabulate(U, dc.F)
    thr = ar.median_threshold(table, 8)
    pt = tracer(dc, **kw)
    for _ in range(dc.F):
        pt.Render()
    pt.SetAdaptive(float(thr), MIN, MAX)
    pt.RenderAdaptive(PASSES)
    sim = ar.Sim(table).run(PASSES, thr, MIN, MAX)
    return pt, sim, U, thr


def run(dc):
    """One handle per case: the adaptive schedule, a render with the switch off, one with it on, three more passes.  Made once."""
    if dc.name in _runs:
        return _runs[dc.name]
    pt, sim, U, thr = adaptive_handle(dc)
    r = dict(before=look(pt))
    r["off"] = pt.Denoise(0)
    r["off_refused"] = used_refused(pt)
    pt.SetDenoiseAdaptiveNoise(True, PRIOR)
    r["between"] = look(pt)
    r["out"] = pt.Denoise(0)
    r["var0"], r["v0"], r["guides"] = pt.DenoiseVarianceUsed(), pt.DenoiseVariance(), pt.DenoiseGuides()
    r["after"] = look(pt)
    pt.RenderAdaptive(3)
    r["later"] = look(pt)
    sim.run(3, thr, MIN, MAX)
    m2, e = sim.stats()
    r["want_later"] = dict(image=sim.image(U), tiles=sim.records(), e=e, m2=m2)
    pt.Dispose()
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _runs[dc.name] = r
    return r


def differing_neighbours(tiles, ids):
    """the hit pixels with a 3x3 neighbour of their own id whose tile holds another count"""
    H, W = ids.shape
    k, _ = da.pixel_counts(tiles, (H, W))
    found = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sh = dv._shift(H, W, dy, dx)
            if sh is None:
                continue
            P, Q = sh
            found[P] |= (ids[Q] == ids[P]) & (k[Q] != k[P])
    return found & (ids >= 0)


# ------------------------------------------------------------------------------------------------ 1 - 3. var_0 and the image, bit for bit
@pytest.mark.parametrize("dc", CASES, ids=lambda c: c.name)
def test_var0_and_output_equal_the_restatement_on_every_pixel(dc):
    r = run(dc)
    g, tiles = r["guides"], r["after"]["tiles"]
    ids = g["id"]
    image = r["after"]["image"]
    assert r["off_refused"]  # (with the switch off nothing was blended)
    # pt_denoise_read_variance still returns V0
    assert same(r["v0"], dv.estimate(image, g)).all()
    # check 1: var_0 from the handle's own records, e, V0 and ids
    want_var0 = da.blend(r["after"]["e"], tiles, r["v0"], ids, PRIOR)
    bad = ~same(r["var0"], want_var0)
    print(f"{dc.name}: var_0: {int(bad.sum())} of {bad.size} pixels differ; counts {np.unique(tiles['k']).tolist()}; "
          f"{int(differing_neighbours(tiles, ids).sum())} hit pixels with a same-id neighbour of another count; "
          f"var_0 != V0 on {int((~same(r['var0'], r['v0'])).sum())} pixels")
    assert r["var0"].shape == ids.shape and r["var0"].dtype == np.float32
    assert not bad.any(), f"{dc.name}: var_0 first at (y, x) = {np.argwhere(bad)[:4].tolist()}: gpu {r['var0'][bad][:4].tolist()} restatement {want_var0[bad][:4].tolist()}"
    # check 2: the passes on that var_0
    want, _, _ = da.denoise(image, g, None, None, DEFAULTS, SIGMA, PRIOR, coc_k(dc), dc.case.focal_length, var0=r["var0"])
    bad = ~same(r["out"], want).all(-1)
    changed = ~same(r["out"], r["off"]).all(-1)
    print(f"{dc.name}: image: {int(bad.sum())} of {bad.size} pixels differ; {int(changed.sum())} differ from the switch-off result")
    assert not bad.any(), f"{dc.name}: image first at (y, x) = {np.argwhere(bad)[:4].tolist()}"
    # check 3 (a 1x1 image passes through the filter whatever var_0 is: the difference is asked where the condition holds)
    if dc.name in NON_VACUOUS:
        assert len(np.unique(tiles["k"])) >= 3, np.unique(tiles["k"])
        assert differing_neighbours(tiles, ids).sum() >= 32
        assert changed.any()
        miss = ids == -1
        assert same(r["var0"][miss], r["v0"][miss]).all()


# ------------------------------------------------------------------------------------------------ 5. the stage writes nothing but var_0
@pytest.mark.parametrize("dc", CASES, ids=lambda c: c.name)
def test_the_adaptive_state_and_the_image_are_not_written(dc):
    r = run(dc)
    for f in ("image", "tiles", "e", "m2"):
        assert r["before"][f].tobytes() == r["between"][f].tobytes() == r["after"][f].tobytes(), f
    got, want = r["later"], r["want_later"]
    assert same(got["image"], want["image"]).all()
    for f in ("k", "k0", "n"):
        assert (got["tiles"][f] == want["tiles"][f]).all(), f
    assert same(got["tiles"]["err"], want["tiles"]["err"]).all()
    assert same(got["m2"], want["m2"]).all() and same(got["e"], want["e"]).all()


# ------------------------------------------------------------------------------------------------ 4. wherever stage A does not run
def test_every_other_setting_is_bit_for_bit_the_switch_off_result():
    dc = BY["43x27_ap0"]
    pt, _, _, _ = adaptive_handle(dc)
    image = pt.Result.copy()
    twin = tracer(dc)
    twin.WriteResult(image, dc.F)

    def both(what, live_differs=False):
        a, b = pt.Denoise(0), twin.Denoise(0)
        assert pt.DenoiseGuides().tobytes() == twin.DenoiseGuides().tobytes(), what
        if live_differs:
            assert a.tobytes() != b.tobytes(), what
            assert not used_refused(pt), what
        else:
            assert a.tobytes() == b.tobytes(), what
            assert used_refused(pt), what
        assert used_refused(twin), what

    both("switch off")
    pt.SetDenoiseAdaptiveNoise(True)
    both("switch on, live state, variance mode", live_differs=True)  # (the control: here it does run)
    pt.SetDenoiseMode(N.PT_DENOISE_FIXED)
    twin.SetDenoiseMode(N.PT_DENOISE_FIXED)
    both("switch on in PT_DENOISE_FIXED")
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
    twin.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
    pt.SetDenoise(0)
    twin.SetDenoise(0)
    both("switch on with iterations = 0")
    pt.SetDenoise()
    twin.SetDenoise()
    both("switch on again", live_differs=True)
    pt.SetDenoiseAdaptiveNoise(False)
    both("switch off again")
    pt.SetDenoiseAdaptiveNoise(True)
    pt.ResetRenderer()
    pt.WriteResult(image, dc.F)
    assert pt._lib.pt_adaptive_status(pt._h, None, None, None, None, None) == N.PT_E_BAD_ARGUMENT  # no live state
    both("switch on after pt_reset")
    twin.SetDenoiseAdaptiveNoise(True)
    both("both switched on, neither live")
    pt.Dispose()
    twin.Dispose()


def test_the_timing_aid_s_pass_0_reads_what_the_last_full_render_s_pass_0_read():
    dc = BY["37x19"]
    pt, _, _, _ = adaptive_handle(dc, params=dr.Params(iterations=1))
    out = np.empty((pt.rows, pt.Width, 4), F32)

    def stage0():
        N.debug_denoise_stage(pt._h, 0, 0)
        N.check(pt._lib.pt_denoise_read(pt._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), pt._h)
        return out.copy()
    off = pt.Denoise(0)
    assert stage0().tobytes() == off.tobytes()
    pt.SetDenoiseAdaptiveNoise(True)
    assert stage0().tobytes() == off.tobytes()  # (the switch alone changes nothing: the last full render blended nothing)
    on = pt.Denoise(0)
    assert on.tobytes() != off.tobytes() and stage0().tobytes() == on.tobytes()
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ 6. error codes and stage B's read-out
def test_error_codes_and_refusals_leave_the_previous_values_in_force():
    dc = BY["37x19"]
    pt, _, _, _ = adaptive_handle(dc)
    L, h = pt._lib, pt._h
    Hh, Ww = dc.case.height, dc.case.width
    buf = np.empty((Hh, Ww), F32)
    bp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pt_denoise_read_variance_used(h, bp, 0) == N.PT_E_BAD_ARGUMENT  # nothing rendered yet
    assert L.pt_denoise_set_adaptive_noise(h, 1, 16) == N.PT_OK
    for bad in (-1, 2, 7):
        assert L.pt_denoise_set_adaptive_noise(h, bad, 8) == N.PT_E_BAD_ARGUMENT, bad
    for bad in (0, -1, 65536):
        assert L.pt_denoise_set_adaptive_noise(h, 0, bad) == N.PT_E_OUT_OF_RANGE, bad
    assert L.pt_denoise_set_adaptive_noise(h, 1, 65535) == N.PT_OK and L.pt_denoise_set_adaptive_noise(h, 1, 1) == N.PT_OK
    assert L.pt_denoise_set_adaptive_noise(h, 1, 16) == N.PT_OK
    assert L.pt_denoise_set_adaptive_noise(h, 0, 0) == N.PT_E_OUT_OF_RANGE and L.pt_denoise_set_adaptive_noise(h, 2, 8) == N.PT_E_BAD_ARGUMENT
    pt.Denoise(0)  # still on, still 16
    want = da.blend(pt.AdaptiveNoise(), pt.AdaptiveTiles(), pt.DenoiseVariance(), pt.DenoiseGuides()["id"], 16)
    assert L.pt_denoise_read_variance_used(h, bp, 0) == N.PT_OK and same(buf, want).all()
    assert not same(want, da.blend(pt.AdaptiveNoise(), pt.AdaptiveTiles(), pt.DenoiseVariance(), pt.DenoiseGuides()["id"], 8)).all()
    assert L.pt_denoise_read_variance_used(h, None, 0) == N.PT_E_BAD_ARGUMENT
    assert L.pt_denoise_read_variance_used(h, bp, Ww * 4 - 1) == N.PT_E_BAD_ARGUMENT
    pitched = np.full((Hh, Ww + 3), -1.0, F32)
    assert L.pt_denoise_read_variance_used(h, pitched.ctypes.data_as(C.POINTER(C.c_float)), (Ww + 3) * 4) == N.PT_OK
    assert same(pitched[:, :Ww], want).all() and (pitched[:, Ww:] == -1.0).all()
    # the temporal stage and the moments stay refused on a live state, switch on or off
    for switch in (lambda on: pt.SetDenoiseTemporal(on), lambda on: pt.SetDenoiseMoments(on)):
        switch(True)
        assert L.pt_denoise_render(h, 0) == N.PT_E_BAD_ARGUMENT
        switch(False)
    # tiled handles are refused by both calls
    for tile in (lambda: pt.SetTile(8, 8), lambda: pt.SetInterleavedTile(1, 3, 8)):
        tile()
        assert L.pt_denoise_set_adaptive_noise(h, 1, 8) == N.PT_E_BAD_ARGUMENT
        assert L.pt_denoise_read_variance_used(h, bp, 0) == N.PT_E_BAD_ARGUMENT
    pt.SetTile(0, Hh)  # all rows again: the handle owns the whole image, and nothing was rendered since the re-tiling
    assert L.pt_denoise_set_adaptive_noise(h, 1, 8) == N.PT_OK and used_refused(pt)
    pt.Dispose()
    g = fh.make_tracer(dc.case, devices=[0, 0])
    assert g._lib.pt_denoise_set_adaptive_noise(g._h, 1, 8) == N.PT_E_BAD_ARGUMENT
    assert g._lib.pt_denoise_read_variance_used(g._h, bp, 0) == N.PT_E_BAD_ARGUMENT
    g.Dispose()


def test_the_read_out_returns_stage_b_s_var0_with_the_moments_on():
    """no adaptive state: pt_denoise_read_variance_used is the public read-out of the moments' blend"""
    dc = BY["37x19"]
    pt = tracer(dc)
    pt.SetDenoiseMoments(True, 16)
    pt.SetDenoiseAdaptiveNoise(True)  # (no live state: nothing of it runs)
    ms = dm.MomentSet()
    for f in (1, 2):
        pt.Render()
        image = pt.Result.copy()
        out = pt.Denoise(0)
        ms = dm.observe(ms, image, f)
        assert used_refused(pt) == (f < 2)  # (one observation: stage B does not run)
    want, _, _, want_var0 = dm.denoise(image, pt.DenoiseGuides(), ms, 2, DEFAULTS, SIGMA, 16)
    got = pt.DenoiseVarianceUsed()
    assert same(got, want_var0).all() and same(out, want).all()
    assert same(got, N.debug_denoise_var0(pt._h, pt.rows, pt.Width)).all()
    assert not same(got, pt.DenoiseVariance()).all()
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ quality (asserted) and cost (measured)
def test_quality_against_the_variance_mode_and_cost_are_recorded():
    """Default scene, 160x90, aperture 0, ray depth 8; truth = the handle's 1024-frame image; MSE of u over the pixels with id >= 0.
    (a) an adaptive run from frame 0 with the defaults and max_samples = 256 until no tile is active: MSE(stage A) < MSE(variance mode
    on the same image) and < MSE(noisy).  (b) every tile at 16 samples (threshold 0, min = max = 16): MSE(stage A) <= 1.05 MSE(variance
    mode), the early-frame allowance of the moments test.  The ratios for prior_samples 8 and 32 are printed.  Cost at
    1920x1080 on a live state after two passes: pt_denoise_render with the switch on against off on the same handle, pt_timer_*, the
    fastest of three; printed, no bound.

    Measured (MI355X), MSE as a fraction of the noisy image's — variance mode / stage A prior 8 / prior 32: (a) 0.9338 / 0.4661 /
    0.5241 at 125.63 samples per pixel; (b) 0.1961 / 0.1967 / 0.1952.  Cost: 0.764 ms on, 0.732 ms off."""
    case = fh.Case("default_160x90_ap0", "default", 160, 90, aperture=0.0)
    ref = fh.make_tracer(case, env=env(), ray_depth=8)
    for _ in range(1024):
        ref.Render()
    truth = dr.u_of(ref.Result[..., :3]).astype(np.float64)
    ref.Dispose()
    lines, rows = [], {}

    def measure(state, pt):
        st = pt.AdaptiveStatus()
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
        noisy = pt.Result.copy()
        var = pt.Denoise(0)
        hit = pt.DenoiseGuides()["id"] >= 0
        assert hit.sum() > hit.size / 2

        def mse(img):
            return float(((dr.u_of(img[..., :3]).astype(np.float64) - truth)[hit] ** 2).mean())
        got = {}
        for prior in (8, 32):
            pt.SetDenoiseAdaptiveNoise(True, prior)
            got[prior] = mse(pt.Denoise(0))
            v0, used = pt.DenoiseVariance(), pt.DenoiseVarianceUsed()
        pt.SetDenoiseAdaptiveNoise(True)  # the default prior
        by_default = mse(pt.Denoise(0))
        assert by_default == got[da.DEFAULT_PRIOR_SAMPLES]
        m_noisy, m_var = mse(noisy), mse(var)
        rows[state] = (m_noisy, m_var, by_default)
        lines.append(f"denoise adaptive quality 160x90 {state}: mean samples/pixel {st['pixel_samples'] / (160 * 90):.2f} (counts {st['min_count']}..{st['max_count']}); "
                     f"MSE(u) noisy {m_noisy:.6g}; ratio variance mode {m_var / m_noisy:.4f}, stage A prior 8 {got[8] / m_noisy:.4f}, prior 32 {got[32] / m_noisy:.4f} "
                     f"(prior 8 / variance mode {got[8] / m_var:.4f}, prior 32 / variance mode {got[32] / m_var:.4f}); "
                     f"mean V0 {float(v0.astype(np.float64)[hit].mean()):.6g}, mean var_0 (prior 32) {float(used.astype(np.float64)[hit].mean()):.6g}")

    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    pt.SetAdaptive(float(ar.DEFAULT_THRESHOLD), ar.DEFAULT_MIN, 256)
    for _ in range(256 // 4 + 1):
        pt.RenderAdaptive(4)
        if pt.AdaptiveStatus()["active_tiles"] == 0:
            break
    assert pt.AdaptiveStatus()["active_tiles"] == 0
    measure("(a) defaults, max 256, finished", pt)
    pt.Dispose()
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    pt.SetAdaptive(0.0, 16, 16)
    pt.RenderAdaptive(16)
    st = pt.AdaptiveStatus()
    assert st["active_tiles"] == 0 and st["min_count"] == st["max_count"] == 16
    measure("(b) every tile at 16", pt)
    pt.Dispose()

    big = fh.Case("default_1080p_ap0", "default", 1920, 1080, aperture=0.0)
    pt = fh.make_tracer(big, env=env(), ray_depth=8)
    pt.SetAdaptive(0.0, 65535, 65535)
    pt.RenderAdaptive(2)
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)

    def render():
        N.check(pt._lib.pt_denoise_render(pt._h, 0), pt._h)

    def fastest(fn):
        ms = []
        for _ in range(3):
            pt.Synchronize()
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)
    times = {}
    for on in (True, False):
        pt.SetDenoiseAdaptiveNoise(on)
        render()  # (buffers allocated, code loaded)
        times["on" if on else "off"] = fastest(render)
        assert used_refused(pt) == (not on)
    pt.Dispose()
    lines.append(f"denoise adaptive cost 1080p: pt_denoise_render switch on {times['on']:.4f} ms, off {times['off']:.4f} ms, difference {times['on'] - times['off']:.4f} ms; "
                 f"pt_adaptive_blend_kernel moves 20.25 bytes per pixel (8 (M2, e) + 4 id + 4 V0 read, 4 written, 16 per 64-pixel tile record)")
    print("\n  " + "\n  ".join(lines))
    m_noisy, m_var, m_a = rows["(a) defaults, max 256, finished"]
    assert m_a < m_var
    assert m_a < m_noisy
    m_noisy, m_var, m_a = rows["(b) every tile at 16"]
    assert m_a <= 1.05 * m_var
    assert all(v > 0 for v in times.values())
