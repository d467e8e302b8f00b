"""The temporal moments of the preview denoiser on the GPU (pt_denoise_set_moments / pt_denoise_read_noise / pt_denoise_noise_level;
pt_moments_kernel, pt_moments_blend_kernel and pt_moments_level_kernel in csrc/pt_denoise_moments.hip) against their definition: the
noise map Vm, the blended variance var_0 and the denoised image equal the numpy float32 restatement (tests/denoise_moments_reference.py;
its own properties: tests/test_denoise_moments_cpu.py) fed with the GPU's own images and guides, on every pixel, bit for bit, look after
look; with the switch off nothing changes; the moment set is forgotten when it must be; pt_render does not notice; the argument checks;
the noise level; accuracy and quality against the variance mode (asserted) and cost (measured), both recorded in DESIGN.md 3.5."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import denoise_lens_reference as dl
import denoise_moments_reference as dm
import denoise_reference as dr
import denoise_variance_reference as dv
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
DEFAULTS = dr.Params()
SIGMA = dv.DEFAULT_SIGMA_VARIANCE
BY = fh.BY_NAME
EVERY, BLOCKS = (1, 1, 1, 1, 1), (1, 3, 4, 8)  # frames between looks


@dataclass(frozen=True)
class MCase:
    name: str
    case: fh.Case
    pattern: tuple
    spp: int = 1
    variance: bool = True
    lens: bool = False
    temporal: bool = False
    params: dr.Params = DEFAULTS
    prior: int = dm.DEFAULT_PRIOR_SAMPLES


def _default(w, h, **kw):
    return fh.Case(f"default_{w}x{h}", "default", w, h, **kw)


D75 = BY["default_75x43_f0"]  # not a multiple of 16: every tile edge case of the 16x16 kernel, and a ragged last block of 256 pixels
CASES = [
    MCase("75x43_every", D75, EVERY),
    MCase("75x43_blocks", D75, BLOCKS),
    MCase("75x43_every_spp4", D75, EVERY, spp=4),
    MCase("75x43_blocks_spp4", D75, BLOCKS, spp=4),
    MCase("75x43_every_fixed", D75, EVERY, variance=False),
    MCase("75x43_blocks_lens", D75, BLOCKS, lens=True),
    MCase("75x43_every_lens_fixed", D75, EVERY, lens=True, variance=False),
    MCase("75x43_every_temporal", D75, EVERY, temporal=True),
    MCase("75x43_blocks_iterations1_prior1", D75, BLOCKS, params=dr.Params(iterations=1), prior=1),
    MCase("75x43_every_iterations0", D75, EVERY, params=dr.Params(iterations=0)),
    MCase("17x33_blocks", _default(17, 33), BLOCKS),
    MCase("17x33_every", _default(17, 33), EVERY),
    MCase("8x8_every", BY["default_8x8"], EVERY),
    MCase("8x8_blocks", BY["default_8x8"], BLOCKS),
    MCase("1x1_every", BY["default_1x1"], EVERY),
    MCase("1x1_blocks", BY["default_1x1"], BLOCKS),
]
NON_VACUOUS = ("75x43_every", "75x43_blocks", "75x43_blocks_spp4", "75x43_blocks_lens", "17x33_blocks")
BY_M = {m.name: m for m in CASES}

_env = None
_runs = {}


def env():
    global _env
    if _env is None:
        _env = pkg.envmap.synthetic_sky_rgba32f(32)
    return _env


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit for bit, NaN == NaN"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def noise_refused(pt):
    buf = np.empty((pt.rows, pt.Width), np.float32)
    a = pt._lib.pt_denoise_read_noise(pt._h, buf.ctypes.data_as(C.POINTER(C.c_float)), 0)
    b = pt._lib.pt_denoise_noise_level(pt._h, None, None, None)
    assert (a == N.PT_OK) == (b == N.PT_OK)
    assert a in (N.PT_OK, N.PT_E_BAD_ARGUMENT) and b in (N.PT_OK, N.PT_E_BAD_ARGUMENT)
    return a == N.PT_E_BAD_ARGUMENT


def tracer(mc, moments):
    pt = fh.make_tracer(mc.case, env=env(), ray_depth=8)
    if mc.spp != 1:
        pt.SPP = mc.spp
    p = mc.params
    pt.SetDenoise(p.iterations, p.sigma_color, p.sigma_plane, p.normal_log2_power)
    if mc.variance:
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
    if mc.lens:
        pt.SetDenoiseLens(True, dl.DEFAULT_COC_SCALE)
    if mc.temporal:
        pt.SetDenoiseTemporal(True)
    if moments:
        pt.SetDenoiseMoments(True, mc.prior)
    return pt


def coc_k(mc):
    if not mc.lens:
        return dr.F(0.0)
    m5 = np.frombuffer(fh.inputs(mc.case)[3], np.float32)[5]
    return dl.cock_of(dl.DEFAULT_COC_SCALE, mc.case.aperture, mc.case.focal_length, mc.case.height, m5)


def run(mc):
    """-> one dict per look: what the handle with the switch on gave (out, vm, var0, v0, level), what a twin with the switch off gave after
    the same calls (off), and the restatement (want_*), made once per case."""
    if mc.name in _runs:
        return _runs[mc.name]
    on, off = tracer(mc, True), tracer(mc, False)
    ms = dm.MomentSet()
    cock = coc_k(mc)
    looks = []
    for step in mc.pattern:
        for _ in range(step):
            on.Render()
            off.Render()
        image = on.Result.copy()
        assert image.tobytes() == off.Result.tobytes()
        n = on.FrameIndex * mc.spp
        r = dict(n=n, image=image, out=on.Denoise(0), off=off.Denoise(0), guides=on.DenoiseGuides())
        assert r["guides"].tobytes() == off.DenoiseGuides().tobytes()
        ids = r["guides"]["id"]
        ms = dm.observe(ms, image, n, mc.spp)
        r["K"] = ms.K
        r["refused"] = noise_refused(on)
        r["vm"] = None if r["refused"] else on.DenoiseNoise()
        r["level"] = None if r["refused"] else on.DenoiseNoiseLevel()
        r["var0"] = N.debug_denoise_var0(on._h, on.rows, on.Width)
        r["v0"] = on.DenoiseVariance() if mc.variance and mc.params.iterations > 0 else None
        r["want_vm"] = dm.noise(ms, image, ids, n)
        if mc.variance and not mc.temporal:
            r["want"], r["want_v0"], _, r["want_var0"] = dm.denoise(image, r["guides"], ms, n, mc.params, SIGMA, mc.prior, cock, mc.case.focal_length)
            if ms.K < 2:
                r["want_var0"] = None  # (stage B does not run: pass 0 reads V0 itself)
        else:
            r["want"], r["want_v0"], r["want_var0"] = r["off"], None, None  # (the filter's result is what it is with the switch off)
        assert on.Result.tobytes() == image.tobytes() and on.FrameIndex * mc.spp == n  # (the image and the counter are where they were)
        looks.append(r)
    on.Dispose()
    off.Dispose()
    for r in looks:
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _runs[mc.name] = looks
    return looks


# ------------------------------------------------------------------------------------------------ 1. Vm, var_0 and the image, bit for bit
@pytest.mark.parametrize("mc", CASES, ids=lambda m: m.name)
def test_noise_map_blend_and_output_equal_the_restatement_on_every_pixel(mc):
    looks = run(mc)
    assert [r["K"] for r in looks] == list(range(1, len(mc.pattern) + 1))
    for r in looks:
        K, g = r["K"], r["guides"]
        hit = g["id"] >= 0
        what = f"{mc.name}, look {K} at n = {r['n']}"
        assert r["refused"] == (K < 2), what  # fewer than two observations: both read-outs are refused
        if K >= 2:
            vm, want_vm = r["vm"], r["want_vm"]
            assert vm.shape == g.shape and vm.dtype == np.float32
            bad = ~same(vm, want_vm)
            print(f"{what}: Vm: {int(bad.sum())} of {bad.size} pixels differ; Vm > 0 on {int(((vm > 0) & hit).sum())} of the {int(hit.sum())} with id >= 0")
            assert not bad.any(), f"{what}: Vm first at (y, x) = {np.argwhere(bad)[:4].tolist()}: gpu {vm[bad][:4].tolist()} restatement {want_vm[bad][:4].tolist()}"
            assert not vm[g["id"] == -1].any()
        if r["want_var0"] is None:
            assert r["var0"] is None, what  # stage B did not run
        else:
            bad = ~same(r["var0"], r["want_var0"])
            print(f"{what}: var_0: {int(bad.sum())} of {bad.size} pixels differ")
            assert not bad.any(), f"{what}: var_0 first at (y, x) = {np.argwhere(bad)[:4].tolist()}"
        if r["want_v0"] is not None:
            assert same(r["v0"], r["want_v0"]).all(), what  # pt_denoise_read_variance still returns V0
        bad = ~same(r["out"], r["want"]).all(-1)
        print(f"{what}: image: {int(bad.sum())} of {bad.size} pixels differ")
        assert not bad.any(), f"{what}: image first at (y, x) = {np.argwhere(bad)[:4].tolist()}"
        if K < 2:
            assert same(r["out"], r["off"]).all(), what
    last = looks[-1]
    if mc.name in NON_VACUOUS:
        hit = last["guides"]["id"] >= 0
        assert ((last["vm"] > 0) & hit).sum() > hit.sum() / 2
        assert (~same(last["var0"], last["v0"]) & hit).sum() > hit.sum() / 2
        assert (~same(last["out"], last["off"]).all(-1) & hit).sum() > hit.sum() / 4  # the blend reaches the picture


def test_the_other_modes_filter_as_with_the_switch_off_and_still_observe():
    for name in ("75x43_every_fixed", "75x43_every_lens_fixed", "75x43_every_temporal", "75x43_every_iterations0"):
        looks = run(BY_M[name])
        for r in looks:
            assert same(r["out"], r["off"]).all(), name
            assert r["var0"] is None, name
        hit = looks[-1]["guides"]["id"] >= 0
        assert ((looks[-1]["vm"] > 0) & hit).sum() > hit.sum() / 2, name
    # the fixed mode of these handles is still the fixed restatement
    r = run(BY_M["75x43_every_fixed"])[-1]
    assert same(r["out"], dr.denoise(r["image"], r["guides"], DEFAULTS)).all()


# ------------------------------------------------------------------------------------------------ 2. switch off
def test_switch_off_is_the_variance_mode_as_it_was():
    """Never on, and on for three looks and off again: image, V0 and guides of the same calls are equal bit for bit, and equal to the
    restatement of the variance mode (which tests/test_gpu_denoise_variance.py holds the kernels to)."""
    def go(toggle):
        pt = fh.make_tracer(D75, env=env(), ray_depth=8)
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
        got = []
        for f in range(5):
            pt.Render()
            if toggle:
                pt.SetDenoiseMoments(f < 3)
            got.append((pt.Result.copy(), pt.Denoise(0), pt.DenoiseVariance(), pt.DenoiseGuides()))
            if not toggle or f >= 3:
                assert noise_refused(pt) and N.debug_denoise_var0(pt._h, pt.rows, pt.Width) is None
        pt.Dispose()
        return got
    never, toggled = go(False), go(True)
    for f in (3, 4):
        (image, out, v0, guides), other = never[f], toggled[f]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(never[f], other)), f
        want, want_v0 = dv.denoise(image, guides, DEFAULTS, SIGMA)
        assert same(out, want).all() and same(v0, want_v0).all()
    assert not same(never[2][1], toggled[2][1]).all()  # (while it was on, it did change the picture)


# ------------------------------------------------------------------------------------------------ 3. state rules
def test_the_moment_set_is_forgotten_when_it_must_be():
    pt = fh.make_tracer(D75, env=env(), ray_depth=8)
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
    pt.SetDenoiseMoments(True)

    def two_looks(what):
        """From a forgotten set: the read-outs are refused until two observations exist."""
        assert noise_refused(pt), what
        pt.Render()
        pt.Denoise(0)
        assert noise_refused(pt), what
        pt.Render()
        pt.Denoise(0)
        assert not noise_refused(pt), what
        assert pt.DenoiseNoiseLevel()[1] == 2, what

    pt.Denoise(0)  # n = 0: no observation
    two_looks("fresh handle")
    # a repeated look at the same n counts nothing twice and changes nothing
    vm = pt.DenoiseNoise()
    pt.Denoise(0)
    assert pt.DenoiseNoiseLevel()[1] == 2 and pt.DenoiseNoise().tobytes() == vm.tobytes()
    pt.Render()
    pt.Denoise(0)
    assert pt.DenoiseNoiseLevel()[1] == 3
    pt.ResetRenderer()
    two_looks("pt_reset")
    pt.SPP = 2
    two_looks("a changed spp")
    image = pt.Result.copy()
    pt.WriteResult(image, 1)
    two_looks("pt_write_result with a smaller frame index")
    pt.SetSize(75, 43)
    two_looks("pt_set_size")
    pt.Dispose()


@pytest.mark.parametrize("name, batch1", [("default_8x8", False), ("default_75x43_f0", False), ("default_75x43_f0", True)])
def test_render_does_not_notice_the_moments(name, batch1):
    case = BY[name]

    def go(with_moments):
        pt = fh.make_tracer(case, env=env(), ray_depth=8)
        if batch1:
            pt.SetFrameBatch(1)  # the frame-fed path
        if with_moments:
            pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
            pt.SetDenoiseMoments(True)
        for f in range(8):
            pt.Render()
            if with_moments and f < 7:
                pt.Denoise(f)
        if with_moments:
            assert pt.DenoiseNoiseLevel()[1] == 7
        img, frames = pt.Result.copy(), pt.FrameIndex
        pt.Dispose()
        return img, frames
    plain, with_m = go(False), go(True)
    assert plain[1] == with_m[1] == 8
    assert (_bits(plain[0]) == _bits(with_m[0])).all()
    assert np.isfinite(plain[0]).all() and plain[0][..., :3].max() > 0


# ------------------------------------------------------------------------------------------------ 4. error codes
def test_error_codes_and_refusals_leave_the_previous_values_in_force():
    pt = fh.make_tracer(D75, env=env(), ray_depth=2)
    L, h = pt._lib, pt._h
    buf = np.empty((43, 75), np.float32)
    bp = buf.ctypes.data_as(C.POINTER(C.c_float))
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
    assert L.pt_denoise_set_moments(h, 1, 16) == N.PT_OK
    for bad in (-1, 2, 7):
        assert L.pt_denoise_set_moments(h, bad, 32) == N.PT_E_BAD_ARGUMENT, bad
    for bad in (0, -1, 65536):
        assert L.pt_denoise_set_moments(h, 0, bad) == N.PT_E_OUT_OF_RANGE, bad
    assert L.pt_denoise_set_moments(h, 1, 65535) == N.PT_OK and L.pt_denoise_set_moments(h, 1, 1) == N.PT_OK
    assert L.pt_denoise_set_moments(h, 1, 16) == N.PT_OK
    assert L.pt_denoise_set_moments(h, 0, 0) == N.PT_E_OUT_OF_RANGE  # still on, still 16
    assert noise_refused(pt)  # nothing rendered yet
    ms = dm.MomentSet()
    for f in (1, 2):
        pt.Render()
        image = pt.Result.copy()
        out = pt.Denoise(0)
        ms = dm.observe(ms, image, f)
        assert noise_refused(pt) == (f < 2)
    want, _, want_vm, want_var0 = dm.denoise(image, pt.DenoiseGuides(), ms, 2, DEFAULTS, SIGMA, 16)
    assert same(out, want).all() and same(N.debug_denoise_var0(h, 43, 75), want_var0).all()
    assert L.pt_denoise_read_noise(h, bp, 0) == N.PT_OK and same(buf, want_vm).all()
    assert L.pt_denoise_read_noise(h, None, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_read_noise(h, bp, 75 * 4 - 1) == N.PT_E_BAD_ARGUMENT
    pitched = np.full((43, 80), -1.0, np.float32)
    assert L.pt_denoise_read_noise(h, pitched.ctypes.data_as(C.POINTER(C.c_float)), 80 * 4) == N.PT_OK
    assert same(pitched[:, :75], want_vm).all() and (pitched[:, 75:] == -1.0).all()
    k = C.c_int()
    assert L.pt_denoise_noise_level(h, None, C.byref(k), None) == N.PT_OK and k.value == 2  # any pointer may be NULL
    assert L.pt_denoise_noise_level(h, None, None, None) == N.PT_OK
    # a render with the switch off: both read-outs are refused, and the set stays
    pt.SetDenoiseMoments(False, 16)
    pt.Denoise(0)
    assert noise_refused(pt)
    pt.SetDenoiseMoments(True, 16)
    pt.Denoise(0)
    assert not noise_refused(pt) and pt.DenoiseNoiseLevel()[1] == 2 and same(pt.DenoiseNoise(), want_vm).all()
    # tiled handles are refused by all three calls
    for tile in (lambda: pt.SetTile(8, 16), lambda: pt.SetInterleavedTile(1, 3, 8)):
        tile()
        assert L.pt_denoise_set_moments(h, 1, 32) == N.PT_E_BAD_ARGUMENT
        assert L.pt_denoise_read_noise(h, bp, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_noise_level(h, None, None, None) == N.PT_E_BAD_ARGUMENT
    pt.SetTile(0, 43)  # all rows again: the handle owns the whole image, and nothing was rendered since the re-tiling
    assert L.pt_denoise_set_moments(h, 1, 32) == N.PT_OK and noise_refused(pt)
    pt.Dispose()
    g = fh.make_tracer(D75, devices=[0, 0])
    assert g._lib.pt_denoise_set_moments(g._h, 1, 32) == N.PT_E_BAD_ARGUMENT
    assert g._lib.pt_denoise_read_noise(g._h, bp, 0) == N.PT_E_BAD_ARGUMENT and g._lib.pt_denoise_noise_level(g._h, None, None, None) == N.PT_E_BAD_ARGUMENT
    g.Dispose()


# ------------------------------------------------------------------------------------------------ 5. noise level
@pytest.mark.parametrize("name", ["75x43_every", "75x43_blocks_spp4", "75x43_every_temporal", "17x33_blocks", "8x8_every", "1x1_blocks"])
def test_noise_level_is_the_mean_of_the_map_over_the_hit_pixels(name):
    """Within a relative 255 * 2^-24: the bound of a 256-term binary32 sum of non-negative terms (the double sum of the partials adds
    nothing at this size).  The counts are exact."""
    for r in run(BY_M[name])[1:]:
        mean, k, count = r["level"]
        hit = r["guides"]["id"] >= 0
        assert k == r["K"] and count == int(hit.sum())
        want = float(r["vm"].astype(np.float64)[hit].mean()) if count else 0.0
        print(f"{name}, look {k}: noise level {mean:.9g}, float64 mean of the map {want:.9g}, {count} pixels")
        assert abs(mean - want) <= 255 * 2.0 ** -24 * want
        assert abs(float(dm.noise_level(r["vm"], r["guides"]["id"])[0]) - want) <= 255 * 2.0 ** -24 * want


# ------------------------------------------------------------------------------------------------ 6. accuracy and quality
QUALITY_FRAMES = (2, 4, 16, 64, 256)
TRUTH_FRAMES = 1024


def test_measured_variance_tracks_the_noise_and_the_blend_beats_the_variance_mode_late():
    """Default scene, 160x90, aperture 0, ray depth 8, the image observed every frame; truth = the 1024-frame image of the same handle;
    MSE of u(c) over the pixels with id >= 0 (handle, scene and metric of test_variance_mode_beats_the_fixed_default_and_the_noisy_image).
    (a) at F = 64, 256 the mean of Vm is closer in log ratio than the mean of V0 to MSE(noisy) / (1 - F / 1024), the noisy image's MSE
    corrected for the truth's own noise; (b) MSE(moments) < MSE(variance mode) at F = 64, 256; (c) MSE(moments) <= 1.05 MSE(variance
    mode) at F = 4, 16.  The table is printed."""
    case = fh.Case("default_160x90_ap0", "default", 160, 90, aperture=0.0)
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
    pt.SetDenoiseMoments(True)
    got = {}
    for f in range(1, TRUTH_FRAMES + 1):
        pt.Render()
        if f in QUALITY_FRAMES:
            with_m, vm, v0 = pt.Denoise(0), pt.DenoiseNoise(), pt.DenoiseVariance()
            assert pt.DenoiseNoiseLevel()[1] == f
            pt.SetDenoiseMoments(False)
            got[f] = (pt.Result.copy(), pt.Denoise(0), with_m, vm, v0)  # (a render with the switch off leaves the set as it is)
            pt.SetDenoiseMoments(True)
        elif f <= QUALITY_FRAMES[-1]:
            N.check(pt._lib.pt_denoise_render(pt._h, 0), pt._h)  # an observation
    hit = pt.DenoiseGuides()["id"] >= 0
    truth = dr.u_of(pt.Result[..., :3]).astype(np.float64)
    pt.Dispose()
    assert hit.sum() > hit.size / 2

    def mse(img):
        return float(((dr.u_of(img[..., :3]).astype(np.float64) - truth)[hit] ** 2).mean())
    rows = {}
    print()
    for f, (noisy, var, mom, vm, v0) in got.items():
        m_noisy, m_var, m_mom = mse(noisy), mse(var), mse(mom)
        target = m_noisy / (1.0 - f / TRUTH_FRAMES)
        mean_vm, mean_v0 = float(vm.astype(np.float64)[hit].mean()), float(v0.astype(np.float64)[hit].mean())
        rows[f] = (m_noisy, m_var, m_mom, target, mean_vm, mean_v0)
        print(f"  denoise moments F = {f}: MSE(u) noisy {m_noisy:.6g} (/ (1 - F/1024): {target:.6g}); mean V0 {mean_v0:.6g} ({mean_v0 / target:.3f} x), "
              f"mean Vm {mean_vm:.6g} ({mean_vm / target:.3f} x); ratio variance mode {m_var / m_noisy:.4f}, moments {m_mom / m_noisy:.4f} "
              f"(moments / variance mode {m_mom / m_var:.4f})")
    for f in (64, 256):
        m_noisy, m_var, m_mom, target, mean_vm, mean_v0 = rows[f]
        assert abs(np.log(mean_vm / target)) < abs(np.log(mean_v0 / target)), f  # (a)
        assert m_mom < m_var, f                                                    # (b)
    for f in (4, 16):
        m_noisy, m_var, m_mom = rows[f][:3]
        assert m_mom <= 1.05 * m_var, f                                            # (c)


# ------------------------------------------------------------------------------------------------ 7. cost (measured, recorded in DESIGN.md)
def test_cost_is_recorded():
    """1920x1080, default scene, default parameters, PT_DENOISE_VARIANCE, pt_timer_*, fastest of three: pt_denoise_render with the switch
    on (an observation and the blend in every render: a frame is rendered between them, outside the timed region) and with it off on the
    same handle, and pt_denoise_noise_level.  Printed; no threshold."""
    case = fh.Case("default_1080p", "default", 1920, 1080)
    pt = fh.make_tracer(case, env=env(), ray_depth=13)
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
    pt.SetDenoiseMoments(True)
    for _ in range(2):
        pt.Render()
        pt.Denoise(0)
    pt.DenoiseNoiseLevel()
    pt.Synchronize()  # (everything warmed up: buffers allocated, code loaded, K = 2)

    def fastest(fn, between=lambda: None):
        ms = []
        for _ in range(3):
            between()
            pt.Synchronize()
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)

    def render():
        N.check(pt._lib.pt_denoise_render(pt._h, 0), pt._h)
    times = {"pt_denoise_render, moments on (observation + blend)": fastest(render, pt.Render),
             "pt_denoise_render, moments on (no new samples: Vm + blend)": fastest(render),
             "pt_denoise_noise_level (blocking)": fastest(pt.DenoiseNoiseLevel)}
    pt.SetDenoiseMoments(False)
    render()
    times["pt_denoise_render, moments off"] = fastest(render)
    pt.Dispose()
    print("\n  " + "\n  ".join(f"denoise moments cost 1080p: {k} {v:.4f} ms" for k, v in times.items()))
    assert all(v > 0 for v in times.values())
