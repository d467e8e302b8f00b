"""The denoiser kernels (csrc/pt_denoise.hip) on adversarial images and parameter extremes against their restatements, bit for bit with
NaN == NaN on every pixel: the output, V0 and — with the temporal stage on — the integrated image.  The image of a case is built on the
host from the id map of the kernels' own guides (tests/denoise_inputs.py: NaN, +-inf, negative luminance, subnormals, values near
FLT_MAX, on tile and halo boundaries and on misses) and written with pt_write_result; the restatement is fed pt.Result read back after
the write and the GPU's guides.  What these inputs decide: x > 0 ? x : 0 and not fmax, the correctly rounded divide, nothing fused, no
flush to zero, a tap of weight 0 still multiplies its colour ("Non-finite and out-of-range colour";
tests/test_denoise_inputs_cpu.py shows that passes which break one of these rules equal the restatement on the renderer's kind of image
and differ on these).  Every case checks on the restatement's output alone that it can fail: at most a quarter of the hit pixels expect
a non-finite colour, and the filter changes more than half of the finite ones (dc.assert_case_can_fail).  No test renders a frame."""
import numpy as np
import pytest

import denoise_input_cases as dc
import denoise_inputs as di
import denoise_temporal_reference as dt
import first_hit_cases as fh
import test_gpu_denoise_temporal as tt

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
same, bits = dc.same, dc.bits

dc.assert_ieee_arithmetic()  # (the GPU machine runs the reference too: it must not be the side that flushes)


def tracer(case, view=None):
    """A handle with the case's parameters and a defined (zero) image; no frame is rendered."""
    view = view or dc.scene_case(case.shape)
    pt = fh.make_tracer(view)
    pt.SetDenoise(case.iterations, case.sigma_color, case.sigma_plane, case.normal_log2_power)
    if case.variance:
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, case.sigma_variance)
    pt.WriteResult(np.zeros((view.height, view.width, 4), np.float32), 0)
    return pt


def id_map(pt):
    pt.Denoise(0)
    return pt.DenoiseGuides()["id"]


_runs = {}


def run(case):
    """-> dict(plan, image, out, v0, guides, want, want_v0): written, denoised and restated once per case."""
    if case.name not in _runs:
        pt = tracer(case)
        pl = di.plan(id_map(pt), case.recipe, case.seed)
        pt.WriteResult(pl.image, 1)
        image = pt.Result.copy()
        out = pt.Denoise(0)
        guides = pt.DenoiseGuides()
        v0 = pt.DenoiseVariance() if case.variance else None
        pt.Dispose()
        want, want_v0 = dc.restate(case, image, guides)
        _runs[case.name] = dict(plan=pl, image=image, out=out, v0=v0, guides=guides, want=want, want_v0=want_v0)
    return _runs[case.name]


# ------------------------------------------------------------------------------------------------ 1. both modes, recipes and extremes
@pytest.mark.parametrize("case", dc.CASES + dc.EXTREMES, ids=lambda c: c.name)
def test_output_and_variance_equal_the_restatement_on_every_pixel(case):
    r = run(case)
    pl, image, out, want, g = r["plan"], r["image"], r["out"], r["want"], r["guides"]
    ids = g["id"]
    W, H = case.shape
    assert out.shape == (H, W, 4) and ids.shape == (H, W)
    assert same(image[..., :3], pl.image[..., :3]).all() and (image[..., 3] == 1).all()  # the write is verbatim, alpha forced to 1
    bad = ~same(out, want).all(-1)
    vbad = ~same(r["v0"], r["want_v0"]) if case.variance else np.zeros(ids.shape, bool)
    nonfinite, changed, hits = dc.shares(image, want, ids)
    print(f"{case.name}: {int(bad.sum())} of {bad.size} pixels differ from the restatement" + (f", V0: {int(vbad.sum())}" if case.variance else "")
          + f"; {hits} hit pixels, {nonfinite:.3f} of them expect a non-finite colour, the filter changes {changed:.3f} of the finite ones; "
          f"{int(pl.special.sum())} special pixels ({int((pl.special & (ids >= 0)).sum())} on hits)"
          + (f"; seeds {pl.seeds}, {pl.distance} from the id's edge" if pl.seeds else "") + (f"; block {pl.block}" if pl.block else ""))
    dc.assert_case_can_fail(case, image, want, ids, pl.special)
    assert not bad.any(), f"{case.name}: first at (y, x) = {np.argwhere(bad)[:4].tolist()}: gpu {out[bad][:2].tolist()} restatement {want[bad][:2].tolist()} input {image[bad][:2].tolist()}"
    assert not vbad.any(), f"{case.name}: V0 first at (y, x) = {np.argwhere(vbad)[:4].tolist()}: gpu {r['v0'][vbad][:4].tolist()} restatement {r['want_v0'][vbad][:4].tolist()}"
    assert (out[..., 3] == 1.0).all()
    assert same(out[ids == -1][:, :3], image[ids == -1][:, :3]).all()  # a miss passes through, whatever it holds
    if case.variance:
        assert not r["v0"][ids == -1].any()
    if case.sigma_color == 1e-40 or case.recipe.kind in ("flat", "zero"):
        assert same(out, image).all()  # inv_sigma = inf / equal colours: every pixel comes back as it went in
    if case.recipe.kind in ("flat", "zero") and case.variance:
        assert not r["v0"].any()       # V0 = 0 everywhere: inv_p = 1 / 1e-8
    if case.recipe.kind == "nonfinite_seed" and ids[pl.seeds[0]] >= 0:
        y, x = pl.seeds[0]
        lost = ~np.isfinite(out[..., :3]).all(-1) & (ids >= 0)
        print(f"{case.name}: {int(lost.sum())} non-finite hit pixels in the output, all of id {int(ids[y, x])} ({int((ids == ids[y, x]).sum())} pixels)")
        assert lost[y, x] and (ids[lost] == ids[y, x]).all()  # the object bounds the spread


# ------------------------------------------------------------------------------------------------ 2. the temporal stage
_truns = {}


def run_temporal(tc):
    """Two epochs on one handle -> (A, B): dicts of image, n, out, I, guides (B also: history) and the restatement's want_I / want_out.
    The id map of a view is learnt by a denoise with the stage off, which touches neither set."""
    if tc.name not in _truns:
        params = dc.Case(tc.shape, tc.current, tc.variance, iterations=tc.iterations)
        view = dc.scene_case(tc.shape)
        pt = tracer(params, view)
        steps = []
        for k, (recipe, n) in enumerate(((tc.history, tc.n_history), (tc.current, tc.n))):
            if k == 1:
                view = tt.moved(view, ("shift", tt.SHIFT))
                tt.new_view(pt, view)
            pt.SetDenoiseTemporal(False, tc.max_history)
            ids = id_map(pt)
            pl = di.plan(ids, recipe, tc.seed + k)
            pt.SetDenoiseTemporal(True, tc.max_history)
            pt.WriteResult(pl.image, n)
            image = pt.Result.copy()
            out = pt.Denoise(0)
            steps.append(dict(recipe=recipe, plan=pl, ids=ids, image=image, n=n, out=out, I=pt.DenoiseIntegrated(), guides=pt.DenoiseGuides(),
                              history=pt.DenoiseHistory() if k == 1 else None))
            if k == 0:
                assert tt.history_refused(pt)
            assert pt.FrameIndex == n
        pt.Dispose()
        p = dc.params_of(params)
        for s in steps:
            hi, hg, B, O = s["history"] if s["history"] else (None, None, None, None)
            s["want_I"] = dt.integrate(s["image"], s["n"], s["guides"], hi, hg, B, O, p, tc.max_history)
            s["want_out"] = dt.filter(s["want_I"], s["guides"], p, params.sigma_variance if tc.variance else None)
        _truns[tc.name] = steps
    return _truns[tc.name]


@pytest.mark.parametrize("tc", dc.TEMPORAL_CASES, ids=lambda t: t.name)
def test_integrated_image_and_output_equal_the_restatement_on_every_pixel(tc):
    a, b = run_temporal(tc)
    hi, hg, _, _ = b["history"]
    assert hi.tobytes() == a["I"].tobytes() and hg.tobytes() == a["guides"].tobytes()  # promotion: epoch A's set, byte for byte
    for k, s in enumerate((a, b)):
        ids = s["guides"]["id"]
        hit = ids >= 0
        bad_I, bad_out = ~same(s["I"], s["want_I"]).all(-1), ~same(s["out"], s["want_out"]).all(-1)
        found = (s["want_I"][..., 3] > np.float32(s["n"])) & hit
        pl = s["plan"]
        assert same(s["image"][..., :3], pl.image[..., :3]).all() and (s["ids"] == ids).all()  # (the plan is that of what was filtered)
        nonfinite_I, nonfinite, changed = dc.shares(s["image"], s["want_I"], ids)[0], *dc.shares(s["image"], s["want_out"], ids)[:2]
        print(f"{tc.name} epoch {'AB'[k]}: I: {int(bad_I.sum())} of {bad_I.size} pixels differ from the restatement, output: {int(bad_out.sum())}; "
              f"{int(hit.sum())} hit pixels, {int(found.sum())} found history, {nonfinite_I:.3f} expect a non-finite I, {nonfinite:.3f} a non-finite output, "
              f"the stage and the filter change {changed:.3f} of the finite ones; {int(pl.special.sum())} special pixels "
              f"({int((pl.special & hit).sum())} on hits, {int((pl.special & ~hit).sum())} on misses)")
        dc.assert_temporal_case_can_fail(tc, s["recipe"], s["image"], s["want_I"], s["want_out"], ids, pl.special)
        assert not bad_I.any(), f"{tc.name}/{k}: I first at (y, x) = {np.argwhere(bad_I)[:4].tolist()}: gpu {s['I'][bad_I][:2].tolist()} restatement {s['want_I'][bad_I][:2].tolist()}"
        assert not bad_out.any(), f"{tc.name}/{k}: output first at (y, x) = {np.argwhere(bad_out)[:4].tolist()}: gpu {s['out'][bad_out][:2].tolist()} restatement {s['want_out'][bad_out][:2].tolist()}"
        assert (s["out"][..., 3] == 1.0).all()
        assert same(s["I"][~hit][:, :3], s["image"][~hit][:, :3]).all() and (s["I"][~hit][:, 3] == s["n"]).all()  # a miss passes through
        if k == 0:
            assert same(s["I"][..., :3], s["image"][..., :3]).all() and (s["I"][..., 3] == s["n"]).all()  # no history: I == (C, n)
        else:
            assert found.sum() > hit.sum() / 2, (tc.name, int(found.sum()), int(hit.sum()))
        assert (s["recipe"].kind == "noise") == (not pl.special.any())


# ------------------------------------------------------------------------------------------------ 3. the present
PRESENT = [c for c in dc.CASES if c.shape == (131, 67) and c.iterations == 3 and not c.variance
           and (c.recipe.kind == "nonfinite_seed" or (c.recipe.kind == "finite_specials" and c.normal_log2_power == 0))]


@pytest.mark.parametrize("mode", [N.PT_ARITH_CONTRACT, N.PT_ARITH_REFERENCE], ids=["contract", "reference"])
@pytest.mark.parametrize("case", PRESENT, ids=lambda c: c.name)
def test_present_is_the_tone_map_of_the_denoised_image(case, mode):
    assert sorted(c.recipe.kind for c in PRESENT) == ["finite_specials", "nonfinite_seed"]
    pt = tracer(case)
    pt.WriteResult(di.build(id_map(pt), case.recipe, case.seed), 1)
    pt.SetPresentArithmetic(mode)
    out = pt.Denoise(0)
    shown = pt.PresentDenoised()
    raw = pt.Present()
    pt.Dispose()
    other = fh.make_tracer(dc.scene_case(case.shape))
    other.SetPresentArithmetic(mode)
    other.WriteResult(out, 1)
    want = other.Present()
    other.Dispose()
    assert same(out, run(case)["out"]).all()
    differ = (shown != want).any(-1)
    print(f"{case.name}: {int(differ.sum())} of {differ.size} presented pixels differ; {int((~np.isfinite(out[..., :3]).all(-1)).sum())} non-finite pixels shown")
    assert shown.tobytes() == want.tobytes()
    assert shown.tobytes() != raw.tobytes()  # (and it is not the raw image's present)
