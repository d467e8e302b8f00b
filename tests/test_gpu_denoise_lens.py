"""The lens mode of the preview denoiser on the GPU (pt_denoise_set_lens; csrc/pt_denoise.hip: pt_guides_ray_kernel<true>,
pt_atrous_kernel<S, VARIANCE, true>) against its restatement (tests/denoise_lens_reference.py; its own properties:
tests/test_denoise_lens_cpu.py): the guides are the pinhole first-hit record's ray; the output, V0 and the temporal stage's I equal the
restatement on every pixel, bit for bit with NaN == NaN, on the renderer's own image and on the adversarial images of
tests/denoise_inputs.py; every case with coc_scale > 0 shows on the restatement alone that it exercises the rule; the switch leaves
nothing behind; quality is measured and asserted as an ordering.

The lens of the cases.  The blur radius scales with the image height: under the reference's lens (focal length 20, aperture 0.14) cocK is
0.06 pixels at 43 rows, so no tap but the centre is ever relaxed at the sizes a quick test uses, and a pixel in focus (t = 20) has c = 0
whatever coc_scale is.  The cases that must exercise the rule therefore use a lens of their own: focal length 0.25 — in front of every
object, so |t - F| / t is within a few percent of 1 on every hit — and aperture 2.4 / H, which makes cocK = 1.91 pixels at coc_scale 1
(taps of r = 1 relaxed, r >= 2 not) and 122 at coc_scale 64 (every tap of every pass: r <= 64).  The reference's lens is used where
the rule is off: coc_scale 0 (pinhole guides under the old tap rules), the guides, the switch discipline and the quality table."""
import ctypes as C
import dataclasses
from dataclasses import dataclass

import numpy as np
import pytest

import denoise_input_cases as dc
import denoise_inputs as di
import denoise_lens_reference as dl
import denoise_reference as dr
import denoise_temporal_reference as dt
import denoise_variance_reference as dv
import first_hit_cases as fh
import test_gpu_denoise_temporal as tt

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
same, bits = dc.same, dc.bits
SIGMA = dv.DEFAULT_SIGMA_VARIANCE
SHAPES = ((1, 40), (40, 1), (33, 17), (75, 43), (130, 9))  # (W, H): tile edges, halos, the 64x4 tiles
R = di.Recipe
RECIPES = (R("finite_specials", boundary=True), R("nonfinite_seed"), R("subnormal_block", boundary=True))

dc.assert_ieee_arithmetic()


def view_of(shape, reference_lens):
    W, H = shape
    if reference_lens:
        return fh.Case(f"default_{W}x{H}_F20_A0.14", "default", W, H, focal_length=20.0, aperture=0.14)
    return fh.Case(f"default_{W}x{H}_F0.25", "default", W, H, focal_length=0.25, aperture=round(2.4 / H, 5))


@dataclass(frozen=True)
class LCase:
    shape: tuple
    variance: bool
    iterations: int
    coc_scale: float
    source: object = "render"      # "render": the renderer's own image (one frame), or a Recipe of tests/denoise_inputs.py
    reference_lens: bool = False
    temporal: bool = False

    @property
    def name(self):
        src = self.source if isinstance(self.source, str) else self.source.name
        return (f"{'variance' if self.variance else 'fixed'}-{self.shape[0]}x{self.shape[1]}-it{self.iterations}-coc{self.coc_scale:g}-{src}"
                + ("-F20" if self.reference_lens else "") + ("-temporal" if self.temporal else ""))


def _cases():
    out, k = [], 0
    # every shape x mode x coc_scale, the iterations and the image cycling through 1..6 and render / the three recipes
    for shape in SHAPES:
        for variance in (False, True):
            for coc in (0.0, 1.0, 64.0):
                src = "render" if k % 2 == 0 else RECIPES[(k // 2) % 3]
                out.append(LCase(shape, variance, 1 + k % 6, coc, src, reference_lens=(coc == 0.0 and src == "render")))
                k += 1
    # every depth on the anchor shape in both modes under the mixed regime, render and recipe alternating the other way
    for variance in (False, True):
        for it in range(1, 7):
            c = LCase((75, 43), variance, it, 1.0, RECIPES[(it // 2) % 3] if it % 2 == 0 else "render")
            if c not in out:
                out.append(c)
    return out


CASES = _cases()
TEMPORAL_CASES = [
    LCase((75, 43), False, 3, 1.0, temporal=True),
    LCase((75, 43), True, 5, 64.0, temporal=True),
    # (with every tap relaxed no id bounds what the blend's n * C and m' * Hc overflow from FLT_MAX: the recipe without huge values)
    LCase((130, 9), False, 2, 64.0, RECIPES[2], temporal=True),
    LCase((33, 17), True, 4, 1.0, RECIPES[0], temporal=True),
    LCase((75, 43), False, 5, 0.0, reference_lens=True, temporal=True),
    LCase((40, 1), True, 1, 1.0, temporal=True),
]

_env = None
_runs = {}


def env():
    global _env
    if _env is None:
        _env = pkg.envmap.synthetic_sky_rgba32f(32)
    return _env


def params_of(case):
    return dr.Params(iterations=case.iterations)


def coc_k(case, view):
    m5 = np.frombuffer(fh.inputs(view)[3], np.float32)[5]
    return dl.cock_of(case.coc_scale, view.aperture, view.focal_length, view.height, m5)


def tracer(case, view):
    pt = fh.make_tracer(view, env=env(), ray_depth=8)
    p = params_of(case)
    pt.SetDenoise(p.iterations, p.sigma_color, p.sigma_plane, p.normal_log2_power)
    if case.variance:
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
    pt.SetDenoiseLens(True, case.coc_scale)
    return pt


def put_image(pt, case, view, seed, n):
    """The image of a case on the handle, frame counter n: rendered, or built from the id map of the handle's own lens-mode guides and
    written.  -> the plan of a written image, or None"""
    if case.source == "render":
        for _ in range(n):
            pt.Render()
        return None
    pt.WriteResult(np.zeros((view.height, view.width, 4), np.float32), 0)
    temporal = case.temporal
    if temporal:
        pt.SetDenoiseTemporal(False)  # (learning the id map must not touch the sets)
    pt.Denoise(0)
    ids = pt.DenoiseGuides()["id"]
    if temporal:
        pt.SetDenoiseTemporal(True)
    pl = di.plan(ids, case.source, seed)
    pt.WriteResult(pl.image, n)
    return pl


def restate(case, view, image, guides, stats=None):
    """-> (expected image, expected V0 or None)"""
    return dl.denoise(image, guides, params_of(case), SIGMA if case.variance else None, coc_k(case, view), view.focal_length, stats=stats)


def run(case):
    """-> dict(view, plan, image, out, v0, guides, pinhole, want, want_v0, stats): made once per case and left unchanged."""
    if case.name not in _runs:
        view = view_of(case.shape, case.reference_lens)
        pt = tracer(case, view)
        pl = put_image(pt, case, view, 7, 1)
        image = pt.Result.copy()
        out = pt.Denoise(3)  # (the guide frame is validated and does not enter)
        guides = pt.DenoiseGuides()
        v0 = pt.DenoiseVariance() if case.variance else None
        pt.SetFirstHitRay(N.PT_RAY_PINHOLE)
        pinhole = pt.FirstHit(0)
        assert pt.FrameIndex == 1 and pt.Result.tobytes() == image.tobytes()  # (the image and the counter are where they were)
        pt.Dispose()
        stats = dl.new_stats()
        want, want_v0 = restate(case, view, image, guides, stats)
        _runs[case.name] = dict(view=view, plan=pl, image=image, out=out, v0=v0, guides=guides, pinhole=pinhole, want=want, want_v0=want_v0, stats=stats)
    return _runs[case.name]


def assert_exercises_the_rule(case, stats, image, want, ids):
    """On the restatement alone: a case with coc_scale > 0 relaxes taps that cross an id, the coc_scale 64 case relaxes every in-image
    tap of every hit pixel, coc_scale 0 none; at most a quarter of the hit pixels expect a non-finite colour."""
    nonfinite, _, hits = dc.shares(image, want, ids)
    assert hits > 0 and stats["taps"] > 0
    assert nonfinite <= 0.25, f"{case.name}: {nonfinite:.3f} of the hit pixels expect a non-finite colour: NaN == NaN compares nothing there"
    if case.coc_scale > 0:
        assert stats["crossing"] > 0, f"{case.name}: no relaxed tap crosses an id"
    else:
        assert stats["relaxed"] == 0
    if case.coc_scale == 64.0:
        assert stats["relaxed"] == stats["taps"], f"{case.name}: {stats['relaxed']} of {stats['taps']} taps relaxed"
    elif case.coc_scale == 1.0:
        assert stats["relaxed"] < stats["taps"]  # the mixed regime: both kinds of tap in one image


# ------------------------------------------------------------------------------------------------ 1. the guides
GUIDE_CASES = [c for c in CASES if c.source == "render" and c.variance is False][:6]


def check_normals(g, view):
    """As test_normals of tests/test_gpu_denoise.py: spheres within 1e-5 of (pos - centre) / radius in float64; cuboid components within
    2^-21 of 0, +-1, +-sqrt(1/2), +-sqrt(1/3), or all three NaN."""
    blob, ns, _, _ = fh.inputs(view)
    f = np.frombuffer(blob, np.float32).astype(np.float64)
    sph = (g["id"] >= 0) & (g["id"] < fh.PT_MAX_SPHERES)
    if sph.any():
        geo = f[:20 * ns].reshape(ns, 20)[:, :4][g["id"][sph]]
        want = (g["pos"][sph].astype(np.float64) - geo[:, :3]) / geo[:, 3:4]
        assert np.abs(g["normal"][sph].astype(np.float64) - want).max() <= 1e-5
    cub = g["id"] >= fh.PT_MAX_SPHERES
    if cub.any():
        n = g["normal"][cub].astype(np.float64)
        nan = np.isnan(n)
        assert (nan.all(-1) | ~nan.any(-1)).all()
        allowed = np.array([0.0, 1.0, np.sqrt(0.5), np.sqrt(1.0 / 3.0)])
        dist = np.abs(np.abs(n[~nan])[:, None] - allowed[None, :]).min(-1)
        assert dist.size == 0 or dist.max() <= 2.0 ** -21


@pytest.mark.parametrize("case", GUIDE_CASES, ids=lambda c: c.name)
def test_guides_are_the_pinhole_first_hit_records_ray(case):
    r = run(case)
    g, f = r["guides"], r["pinhole"]
    want = dl.guides_from_records(f, g["normal"])
    hit = g["id"] >= 0
    assert (g["id"] == want["id"]).all() and (bits(g["t"]) == bits(want["t"])).all()
    assert (bits(g["pos"]) == bits(want["pos"])).all()  # P = dir * t + origin in two roundings; 0 on a miss
    miss = ~hit
    assert (bits(g["normal"][miss]) == 0).all() and np.isposinf(g["t"][miss]).all()
    assert hit.any()
    check_normals(g, r["view"])
    column = np.frombuffer(fh.inputs(r["view"])[3], np.float32)[28:31]
    assert (bits(f["origin"]) == bits(column)).all()


def test_guides_do_not_depend_on_the_frame_or_the_lens_and_differ_from_sample_0():
    view = view_of((75, 43), True)
    pt = fh.make_tracer(view, env=env(), ray_depth=2)
    pt.Render()
    pt.SetDenoise(1)
    pt.Denoise(0)
    sample0 = pt.DenoiseGuides()
    pt.SetDenoiseLens(True, 0.0)
    pt.Denoise(0)
    g0 = pt.DenoiseGuides()
    pt.Denoise(7)
    g7 = pt.DenoiseGuides()
    pt.Dispose()
    other = fh.make_tracer(dataclasses.replace(view, focal_length=5.0, aperture=2.0), env=env(), ray_depth=2)
    other.Render()
    other.SetDenoise(1)
    other.SetDenoiseLens(True, 0.0)
    other.Denoise(0)
    g_other = other.DenoiseGuides()
    other.Dispose()
    assert g0.tobytes() == g7.tobytes() == g_other.tobytes()
    assert g0.tobytes() != sample0.tobytes()


# ------------------------------------------------------------------------------------------------ 2. the kernels, bit for bit
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_output_and_variance_equal_the_restatement_on_every_pixel(case):
    r = run(case)
    image, out, want, g, stats = r["image"], r["out"], r["want"], r["guides"], r["stats"]
    ids = g["id"]
    W, H = case.shape
    assert out.shape == (H, W, 4) and ids.shape == (H, W)
    bad = ~same(out, want).all(-1)
    vbad = ~same(r["v0"], r["want_v0"]) if case.variance else np.zeros(ids.shape, bool)
    nonfinite, changed, hits = dc.shares(image, want, ids)
    print(f"{case.name}: {int(bad.sum())} of {bad.size} pixels differ from the restatement" + (f", V0: {int(vbad.sum())}" if case.variance else "")
          + f"; cocK {float(coc_k(case, r['view'])):.4g}; {hits} hit pixels, {len(np.unique(ids))} ids; taps {stats['taps']}, relaxed {stats['relaxed']}, "
          f"relaxed across an id {stats['crossing']}; {nonfinite:.3f} expect a non-finite colour, the filter changes {changed:.3f} of the finite ones")
    assert_exercises_the_rule(case, stats, image, want, ids)
    assert not bad.any(), f"{case.name}: first at (y, x) = {np.argwhere(bad)[:4].tolist()}: gpu {out[bad][:2].tolist()} restatement {want[bad][:2].tolist()}"
    assert not vbad.any(), f"{case.name}: V0 first at (y, x) = {np.argwhere(vbad)[:4].tolist()}"
    assert (out[..., 3] == 1.0).all()
    assert same(out[ids == -1][:, :3], image[ids == -1][:, :3]).all()  # a miss still passes through
    if case.coc_scale == 0:  # pinhole guides under the old tap rules: the existing restatements
        p = params_of(case)
        old = dv.denoise(image, g, p, SIGMA)[0] if case.variance else dr.denoise(image, g, p)
        assert same(out, old).all()


_truns = {}


def run_temporal(case):
    """Two epochs on one handle (a camera shift between them) -> one dict per epoch, as run_temporal of tests/test_gpu_denoise_inputs.py."""
    if case.name not in _truns:
        view = view_of(case.shape, case.reference_lens)
        pt = tracer(case, view)
        pt.SetDenoiseTemporal(True, 32)
        steps = []
        for k, n in enumerate((2, 1)):
            if k == 1:
                view = tt.moved(view, ("shift", tt.SHIFT))
                tt.new_view(pt, view)
            put_image(pt, case, view, 11 + k, n)
            image = pt.Result.copy()
            out = pt.Denoise(0)
            steps.append(dict(view=view, image=image, n=n, out=out, I=pt.DenoiseIntegrated(), guides=pt.DenoiseGuides(),
                              v0=pt.DenoiseVariance() if case.variance else None, history=pt.DenoiseHistory() if k == 1 else None))
            if k == 0:
                assert tt.history_refused(pt)
            assert pt.FrameIndex == n
        pt.Dispose()
        for s in steps:
            hi, hg, B, O = s["history"] if s["history"] else (None, None, None, None)
            s["want_I"] = dt.integrate(s["image"], s["n"], s["guides"], hi, hg, B, O, params_of(case), 32)
            c0 = s["want_I"].copy()
            c0[..., 3] = np.float32(1.0)  # (as denoise_temporal_reference.filter: the count in I's alpha is not the passes' input)
            s["stats"] = dl.new_stats()
            s["want_out"], s["want_v0"] = restate(case, s["view"], c0, s["guides"], s["stats"])
        _truns[case.name] = steps
    return _truns[case.name]


@pytest.mark.parametrize("case", TEMPORAL_CASES, ids=lambda c: c.name)
def test_integrated_image_and_output_equal_the_restatement_on_every_pixel(case):
    a, b = run_temporal(case)
    hi, hg, B, O = b["history"]
    assert hi.tobytes() == a["I"].tobytes() and hg.tobytes() == a["guides"].tobytes()  # promotion: epoch A's set, byte for byte
    _, wantB, wantO = dt.camera(fh.inputs(a["view"])[3])
    assert (bits(B) == bits(wantB)).all() and (bits(O) == bits(wantO)).all()  # the history camera is epoch A's pinhole
    for k, s in enumerate((a, b)):
        ids = s["guides"]["id"]
        hit = ids >= 0
        bad_I, bad_out = ~same(s["I"], s["want_I"]).all(-1), ~same(s["out"], s["want_out"]).all(-1)
        vbad = ~same(s["v0"], s["want_v0"]) if case.variance else np.zeros(ids.shape, bool)
        found = (s["want_I"][..., 3] > np.float32(s["n"])) & hit
        st = s["stats"]
        print(f"{case.name} epoch {'AB'[k]}: I: {int(bad_I.sum())} of {bad_I.size} pixels differ from the restatement, output: {int(bad_out.sum())}, "
              f"V0: {int(vbad.sum())}; {int(hit.sum())} hit pixels, {int(found.sum())} found history; taps {st['taps']}, relaxed {st['relaxed']}, "
              f"relaxed across an id {st['crossing']}")
        c0 = s["want_I"].copy()
        c0[..., 3] = np.float32(1.0)
        assert_exercises_the_rule(case, st, c0, s["want_out"], ids)
        assert dc.shares(s["image"], s["want_I"], ids)[0] <= 0.25
        assert not bad_I.any(), f"{case.name}/{k}: I first at (y, x) = {np.argwhere(bad_I)[:4].tolist()}"
        assert not bad_out.any(), f"{case.name}/{k}: output first at (y, x) = {np.argwhere(bad_out)[:4].tolist()}"
        assert not vbad.any()
        assert (s["out"][..., 3] == 1.0).all()
        if k == 0:
            assert same(s["I"][..., :3], s["image"][..., :3]).all() and (s["I"][..., 3] == s["n"]).all()  # no history: I == (C, n)
        elif case.shape[1] > 1:
            assert found.sum() > hit.sum() / 2, (case.name, int(found.sum()), int(hit.sum()))


# ------------------------------------------------------------------------------------------------ 3. the switch
def _both_modes(pt, temporal):
    pt.SetDenoiseTemporal(temporal)
    pt.SetDenoiseMode(N.PT_DENOISE_FIXED)
    f, gf = pt.Denoise(1), pt.DenoiseGuides()
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
    return f, gf, pt.Denoise(1), pt.DenoiseVariance(), pt.DenoiseGuides()


def test_off_again_is_a_handle_that_never_enabled_it_and_render_does_not_notice():
    view = view_of((75, 43), True)

    def go(with_lens):
        pt = fh.make_tracer(view, env=env(), ray_depth=8)
        pt.Render()
        pt.Render()
        if with_lens:
            pt.SetDenoiseLens(True, 2.0)
            _both_modes(pt, False)
            _both_modes(pt, True)
            pt.SetDenoiseLens(False, 2.0)
            pt.ClearDenoiseHistory()
        res = _both_modes(pt, False) + _both_modes(pt, True) + (pt.DenoiseIntegrated(),)
        # the pt_render path: the result buffer of the denoiser stays where it is while frames and lens-mode renders alternate
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        seen = set()
        if with_lens:
            pt.SetDenoiseLens(True, 2.0)
        pt.SetDenoiseTemporal(False)
        pt.SetDenoiseMode(N.PT_DENOISE_FIXED)
        for f in range(6):
            pt.Render()
            pt.Denoise(f)
            N.check(pt._lib.pt_denoise_device_ptr(pt._h, C.byref(ptr), C.byref(nbytes)), pt._h)
            seen.add((ptr.value, nbytes.value))
        img, frames = pt.Result.copy(), pt.FrameIndex
        pt.Dispose()
        return res, img, frames, seen
    plain, lens = go(False), go(True)
    for a, b in zip(plain[0], lens[0]):
        assert a.tobytes() == b.tobytes()
    assert plain[2] == lens[2] == 8 and plain[1].tobytes() == lens[1].tobytes()
    assert len(lens[3]) == 1 and len(plain[3]) == 1  # one buffer, one size: nothing was allocated along the way


def test_error_codes_and_refusals_leave_the_previous_values_in_force():
    case = LCase((75, 43), False, 2, 3.0)
    view = view_of(case.shape, False)
    pt = tracer(case, view)  # pt_denoise_set_lens(h, 1, 3.0)
    L, h = pt._lib, pt._h
    pt.Render()
    for bad in (-1, 2):
        assert L.pt_denoise_set_lens(h, bad, 1.0) == N.PT_E_BAD_ARGUMENT, bad
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert L.pt_denoise_set_lens(h, 0, bad) == N.PT_E_BAD_ARGUMENT, bad
    for bad in (-0.5, -1e-30):
        assert L.pt_denoise_set_lens(h, 0, bad) == N.PT_E_OUT_OF_RANGE, bad
    image = pt.Result.copy()
    out, g = pt.Denoise(0), pt.DenoiseGuides()
    stats = dl.new_stats()
    want, _ = restate(case, view, image, g, stats)
    assert stats["crossing"] > 0 and same(out, want).all()  # enable 1, coc_scale 3 still in force
    assert not same(out, dr.denoise(image, g, params_of(case))).all()
    assert L.pt_denoise_render(h, -1) == N.PT_E_BAD_ARGUMENT  # the guide frame is still validated
    assert L.pt_denoise_set_lens(h, 1, 0.0) == N.PT_OK
    assert same(pt.Denoise(0), dr.denoise(image, pt.DenoiseGuides(), params_of(case))).all()  # coc_scale 0: pinhole guides, the old rules
    assert pt.DenoiseGuides().tobytes() == g.tobytes()
    for tile in (lambda: pt.SetTile(8, 16), lambda: pt.SetInterleavedTile(1, 3, 8)):
        tile()
        assert L.pt_denoise_set_lens(h, 1, 1.0) == N.PT_E_BAD_ARGUMENT
    pt.Dispose()
    grp = fh.make_tracer(view, devices=[0, 0])
    assert grp._lib.pt_denoise_set_lens(grp._h, 1, 1.0) == N.PT_E_BAD_ARGUMENT
    grp.Dispose()


# ------------------------------------------------------------------------------------------------ 4. quality (measured; asserted as an ordering)
QUALITY_LENSES = {"reference (F 20, A 0.14)": (20.0, 0.14), "strong (F 20, A 2)": (20.0, 2.0)}
QUALITY_FRAMES = (1, 4, 16)
QUALITY_GRID = (0.5, 1.0, 2.0)
TRUTH_FRAMES = 4096


def quality_table(truth_frames=TRUTH_FRAMES, also_at=()):
    """Default scene, 160x90, ray depth 8.  -> {(lens, mode, setting, frames): MSE(denoised) / MSE(noisy)} with MSE of u(c) over the
    pixels whose pinhole id >= 0 against the truth_frames-frame image of the same handle, and {(lens, frames): MSE(noisy)}; also_at:
    further truth lengths -> {(lens, length, frames): MSE(noisy)} for judging the truth."""
    ratios, noisy_mse, truth_check = {}, {}, {}
    for lens, (focal, aperture) in QUALITY_LENSES.items():
        view = fh.Case("default_160x90", "default", 160, 90, focal_length=focal, aperture=aperture)
        pt = fh.make_tracer(view, env=env(), ray_depth=8)
        pt.SetDenoiseLens(True, 0.0)
        pt.SetDenoise(0)
        pt.Denoise(0)
        hit = pt.DenoiseGuides()["id"] >= 0
        pt.SetDenoise()
        got = {}
        marks = sorted(set(also_at) | {truth_frames})
        truths = {}
        for f in range(1, marks[-1] + 1):
            pt.Render()
            if f in QUALITY_FRAMES:
                res = {"noisy": pt.Result.copy()}
                for mode, mname in ((N.PT_DENOISE_FIXED, "fixed"), (N.PT_DENOISE_VARIANCE, "variance")):
                    pt.SetDenoiseMode(mode, SIGMA)
                    pt.SetDenoiseLens(False, 1.0)
                    res[mname, "sample 0"] = pt.Denoise(0)
                    for coc in (0.0,) + QUALITY_GRID:
                        pt.SetDenoiseLens(True, coc)
                        res[mname, f"lens {coc:g}"] = pt.Denoise(0)
                got[f] = res
            if f in marks:
                truths[f] = dr.u_of(pt.Result[..., :3]).astype(np.float64)
        pt.Dispose()
        assert hit.sum() > hit.size / 2

        def mse(img, truth):
            return float(((dr.u_of(img[..., :3]).astype(np.float64) - truth)[hit] ** 2).mean())
        for f, res in got.items():
            for m in marks:
                truth_check[lens, m, f] = mse(res["noisy"], truths[m])
            noisy_mse[lens, f] = mse(res["noisy"], truths[truth_frames])
            for key, img in res.items():
                if key != "noisy":
                    ratios[(lens,) + key + (f,)] = mse(img, truths[truth_frames]) / noisy_mse[lens, f]
    return ratios, noisy_mse, truth_check


def print_quality(ratios, noisy_mse):
    settings = ["sample 0", "lens 0"] + [f"lens {c:g}" for c in QUALITY_GRID]
    for lens in QUALITY_LENSES:
        print(f"\n  denoise lens quality, {lens}: MSE(u) noisy " + ", ".join(f"F = {f}: {noisy_mse[lens, f]:.6g}" for f in QUALITY_FRAMES))
        for mode in ("fixed", "variance"):
            for s in settings:
                print(f"  denoise lens quality, {lens}, {mode}, {s}: ratio " + "  ".join(f"F = {f}: {ratios[lens, mode, s, f]:.4f}" for f in QUALITY_FRAMES))


def test_lens_mode_beats_sample_0_guides_with_the_lens_open():
    """The ratio MSE(denoised) / MSE(noisy) at 1, 4 and 16 frames for sample-0 guides, lens mode with coc_scale 0 and the grid 0.5, 1, 2,
    in both filter modes under both lenses: printed (DESIGN.md 3.5 holds the table); asserted: lens mode at the shipped default
    coc_scale is below sample-0 guides at 4 and 16 frames."""
    ratios, noisy_mse, _ = quality_table()
    print_quality(ratios, noisy_mse)
    default = f"lens {dl.DEFAULT_COC_SCALE:g}"
    for lens in QUALITY_LENSES:
        for mode in ("fixed", "variance"):
            for f in (4, 16):
                assert ratios[lens, mode, default, f] < ratios[lens, mode, "sample 0", f], (lens, mode, f)
