"""The variance-guided mode of the preview denoiser on the GPU (pt_denoise_set_mode / pt_denoise_read_variance; pt_variance_kernel and
pt_atrous_kernel<S, true> in csrc/pt_denoise.hip) against its definition: the estimate and the passes equal the numpy float32 restatement
(tests/denoise_variance_reference.py; its own properties: tests/test_denoise_variance_cpu.py) on the GPU's own image and guides on every
pixel, bit for bit; the fixed mode and pt_render do not notice; the argument checks; quality against the fixed mode (asserted) and cost
(measured), both recorded in DESIGN.md 3.5."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import denoise_reference as dr
import denoise_variance_reference as dv
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
DEFAULTS = dr.Params()
SIGMA = dv.DEFAULT_SIGMA_VARIANCE


@dataclass(frozen=True)
class VCase:
    name: str
    case: fh.Case
    frames: int = 1
    params: dr.Params = DEFAULTS
    sigma_variance: float = SIGMA
    guide_frame: int = 0


def _default(w, h, **kw):
    return fh.Case(f"default_{w}x{h}", "default", w, h, **kw)


BY = fh.BY_NAME
CASES = [
    # several workgroups in both directions (16x16 and 64x4 tiles), ragged right and top edge, in-image taps at step 16
    VCase("default_131x67_F1", _default(131, 67), 1),
    VCase("default_131x67_F3", _default(131, 67), 3, guide_frame=2),
    VCase("default_75x43", BY["default_75x43_f0"], 1),
    VCase("default_8x8", BY["default_8x8"], 1),        # the 7x7 window and every far tap fall off the image
    VCase("default_1x1", BY["default_1x1"], 1),        # n = 0: V0 = 0
    VCase("full_64x36", BY["full_64x36"], 2),
    VCase("edge_64x36", BY["edge_64x36"], 2),          # camera inside sphere 0
    VCase("incuboid_64x36", BY["incuboid_64x36"], 2),  # camera inside cuboid 6: NaN normals on its edges
    VCase("empty_16x9", BY["empty_16x9"], 1),          # no objects: output == input, V0 = 0
    VCase("iterations0", BY["default_75x43_f0"], 1, dr.Params(iterations=0)),  # a copy; pt_denoise_read_variance is refused
    VCase("iterations1", BY["default_75x43_f0"], 1, dr.Params(iterations=1)),  # the first pass is the last: V0 buffer in, alpha 1 out
    VCase("iterations2", BY["default_75x43_f0"], 1, dr.Params(iterations=2)),  # the last pass is the step-2 instantiation
    VCase("iterations6", _default(131, 67), 1, dr.Params(iterations=6)),
    VCase("sigma3_plane_power", BY["default_75x43_f0"], 2, dr.Params(iterations=4, sigma_plane=0.05, normal_log2_power=2), 3.0),
    VCase("sigma8_plane_power", BY["default_75x43_ap0"], 1, dr.Params(iterations=3, sigma_plane=0.004, normal_log2_power=7), 8.0),
]
NON_VACUOUS = ("default_131x67_F1", "default_75x43", "default_8x8")

_env = None
_runs = {}


def env():
    global _env
    if _env is None:
        _env = pkg.envmap.synthetic_sky_rgba32f(32)
    return _env


def set_params(pt, p):
    pt.SetDenoise(p.iterations, p.sigma_color, p.sigma_plane, p.normal_log2_power)


def run(vc):
    """-> dict(image, fixed, out, var, guides, want, want_var): rendered, denoised in both modes and restated once per case."""
    if vc.name not in _runs:
        pt = fh.make_tracer(vc.case, env=env(), ray_depth=8)
        set_params(pt, vc.params)
        for _ in range(vc.frames):
            pt.Render()
        image = pt.Result.copy()
        fixed = pt.Denoise(vc.guide_frame)
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, vc.sigma_variance)
        out = pt.Denoise(vc.guide_frame)
        if vc.params.iterations == 0:
            var = None
            buf = np.empty(out.shape[:2], np.float32)
            assert pt._lib.pt_denoise_read_variance(pt._h, buf.ctypes.data_as(C.POINTER(C.c_float)), 0) == N.PT_E_BAD_ARGUMENT
        else:
            var = pt.DenoiseVariance()
        guides = pt.DenoiseGuides()
        again = pt.Result.copy()
        frames = pt.FrameIndex
        pt.Dispose()
        assert frames == vc.frames and image.tobytes() == again.tobytes()  # (the image and the counter are where they were)
        want, want_var = dv.denoise(image, guides, vc.params, vc.sigma_variance)
        r = dict(image=image, fixed=fixed, out=out, var=var, guides=guides, want=want, want_var=want_var)
        for a in r.values():
            if a is not None:
                a.setflags(write=False)
        _runs[vc.name] = r
    return _runs[vc.name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit for bit, NaN == NaN"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------------ 1. estimate and filter, bit for bit
@pytest.mark.parametrize("vc", CASES, ids=lambda v: v.name)
def test_variance_and_output_equal_the_restatement_on_every_pixel(vc):
    r = run(vc)
    out, want, g, var, want_var = r["out"], r["want"], r["guides"], r["var"], r["want_var"]
    assert out.shape == (vc.case.height, vc.case.width, 4) and g.shape == out.shape[:2]
    hit = g["id"] >= 0
    bad = ~same(out, want).all(-1)
    differs = (~same(out[..., :3], r["fixed"][..., :3]).all(-1)) & hit
    print(f"{vc.name}: image: {int(bad.sum())} of {bad.size} pixels differ from the restatement; {int(hit.sum())} pixels with id >= 0, "
          f"{int(differs.sum())} of them differ from the fixed mode's")
    if vc.params.iterations == 0:
        assert var is None and want_var is None
    else:
        assert var.shape == g.shape and var.dtype == np.float32
        vbad = ~same(var, want_var)
        print(f"{vc.name}: V0: {int(vbad.sum())} of {vbad.size} pixels differ; V0 > 0 on {int(((var > 0) & hit).sum())} of the {int(hit.sum())}")
        assert not vbad.any(), f"{vc.name}: V0 first at (y, x) = {np.argwhere(vbad)[:4].tolist()}: gpu {var[vbad][:4].tolist()} restatement {want_var[vbad][:4].tolist()}"
        assert not var[~hit].any()  # V0 = 0 on a miss
    assert not bad.any(), f"{vc.name}: first at (y, x) = {np.argwhere(bad)[:4].tolist()}: gpu {out[bad][:2].tolist()} restatement {want[bad][:2].tolist()}"
    assert (out[..., 3] == 1.0).all()
    if vc.params.iterations == 0 or vc.case.scene == "empty":
        assert same(out[..., :3], r["image"][..., :3]).all()
    assert same(out[~hit][..., :3], r["image"][~hit][..., :3]).all()  # a miss passes through
    if vc.name == "default_1x1":
        assert not var.any()  # n = 0
    if vc.name in NON_VACUOUS:
        assert ((var > 0) & hit).sum() > hit.sum() / 2
        assert differs.sum() > hit.sum() / 2


def test_the_fixed_mode_of_these_handles_is_still_the_fixed_restatement():
    for name in ("default_131x67_F1", "incuboid_64x36", "sigma3_plane_power"):
        vc = next(v for v in CASES if v.name == name)
        r = run(vc)
        assert same(r["fixed"], dr.denoise(r["image"], r["guides"], vc.params)).all(), name


# ------------------------------------------------------------------------------------------------ 2. isolation
def test_modes_do_not_leak_into_each_other():
    case = BY["default_75x43_f0"]
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    pt.Render()
    pt.Render()
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, 4.0)
    v1, var1 = pt.Denoise(1), pt.DenoiseVariance()
    pt.SetDenoiseMode(N.PT_DENOISE_FIXED, 4.0)
    f = pt.Denoise(1)
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, 4.0)
    v2, var2 = pt.Denoise(1), pt.DenoiseVariance()
    pt.Dispose()
    other = fh.make_tracer(case, env=env(), ray_depth=8)
    other.Render()
    other.Render()
    f_only = other.Denoise(1)
    other.Dispose()
    assert same(f, f_only).all()
    assert same(v1, v2).all() and same(var1, var2).all()
    assert not same(v1, f).all()


@pytest.mark.parametrize("name, batch1", [("default_8x8", False), ("default_75x43_f0", False), ("default_75x43_f0", True)])
def test_render_does_not_notice_the_variance_mode(name, batch1):
    case = BY[name]

    def go(with_denoise):
        pt = fh.make_tracer(case, env=env(), ray_depth=8)
        if batch1:
            pt.SetFrameBatch(1)  # the frame-fed path
        if with_denoise:
            pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
        for f in range(8):
            pt.Render()
            if with_denoise and f < 7:
                pt.Denoise(f)
        img, frames = pt.Result.copy(), pt.FrameIndex
        pt.Dispose()
        return img, frames
    plain, with_d = go(False), go(True)
    assert plain[1] == with_d[1] == 8
    assert (_bits(plain[0]) == _bits(with_d[0])).all()
    assert np.isfinite(plain[0]).all() and plain[0][..., :3].max() > 0


# ------------------------------------------------------------------------------------------------ 3. error codes
def test_error_codes_resize_and_refused_handles():
    case = BY["default_75x43_f0"]
    pt = fh.make_tracer(case, env=env(), ray_depth=2)
    L, h = pt._lib, pt._h
    var = np.empty((43, 75), np.float32)
    vp = var.ctypes.data_as(C.POINTER(C.c_float))
    V, F = N.PT_DENOISE_VARIANCE, N.PT_DENOISE_FIXED
    pt.Render()
    assert L.pt_denoise_read_variance(h, vp, 0) == N.PT_E_BAD_ARGUMENT  # nothing rendered yet
    # parameters: bad values are refused and the previous ones stay in force
    assert L.pt_denoise_set_mode(h, V, 3.0) == N.PT_OK
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert L.pt_denoise_set_mode(h, V, bad) == N.PT_E_BAD_ARGUMENT, bad
        assert L.pt_denoise_set_mode(h, F, bad) == N.PT_E_BAD_ARGUMENT, bad
    for bad in (0.0, -1.0):
        assert L.pt_denoise_set_mode(h, F, bad) == N.PT_E_OUT_OF_RANGE, bad
    for bad in (-1, 2, 7):
        assert L.pt_denoise_set_mode(h, bad, 6.0) == N.PT_E_BAD_ARGUMENT, bad
    image = pt.Result.copy()
    out = pt.Denoise(0)  # still VARIANCE, 3.0
    want, want_var = dv.denoise(image, pt.DenoiseGuides(), DEFAULTS, 3.0)
    assert same(out, want).all()
    assert L.pt_denoise_read_variance(h, vp, 0) == N.PT_OK and same(var, want_var).all()
    assert L.pt_denoise_read_variance(h, None, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_read_variance(h, vp, 75 * 4 - 1) == N.PT_E_BAD_ARGUMENT
    pitched = np.full((43, 80), -1.0, np.float32)
    assert L.pt_denoise_read_variance(h, pitched.ctypes.data_as(C.POINTER(C.c_float)), 80 * 4) == N.PT_OK
    assert same(pitched[:, :75], want_var).all() and (pitched[:, 75:] == -1.0).all()
    # sigma_variance is stored in FIXED mode too; a FIXED render leaves no estimate
    assert L.pt_denoise_set_mode(h, F, 5.0) == N.PT_OK
    assert same(pt.Denoise(0), dr.denoise(image, pt.DenoiseGuides(), DEFAULTS)).all()
    assert L.pt_denoise_read_variance(h, vp, 0) == N.PT_E_BAD_ARGUMENT
    # iterations = 0: a copy, no estimate
    assert L.pt_denoise_set_mode(h, V, 5.0) == N.PT_OK
    pt.SetDenoise(0)
    pt.Denoise(0)
    assert L.pt_denoise_read_variance(h, vp, 0) == N.PT_E_BAD_ARGUMENT
    pt.SetDenoise()
    pt.Denoise(0)
    assert L.pt_denoise_read_variance(h, vp, 0) == N.PT_OK
    # pt_set_size frees the buffers: a read after it fails
    pt.SetSize(75, 43)
    assert L.pt_denoise_read_variance(h, vp, 0) == N.PT_E_BAD_ARGUMENT
    pt.Render()
    assert L.pt_denoise_render(h, 0) == N.PT_OK and L.pt_denoise_read_variance(h, vp, 0) == N.PT_OK  # (the mode survives a resize)
    # tiled handles are refused by both calls
    for tile in (lambda: pt.SetTile(8, 16), lambda: pt.SetInterleavedTile(1, 3, 8)):
        tile()
        assert L.pt_denoise_set_mode(h, V, 6.0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_read_variance(h, vp, 0) == N.PT_E_BAD_ARGUMENT
    pt.SetTile(0, 43)  # all rows again: the handle owns the whole image
    pt.Render()
    assert L.pt_denoise_set_mode(h, V, 6.0) == N.PT_OK and L.pt_denoise_render(h, 0) == N.PT_OK and L.pt_denoise_read_variance(h, vp, 0) == N.PT_OK
    pt.Dispose()
    g = fh.make_tracer(case, devices=[0, 0])
    assert g._lib.pt_denoise_set_mode(g._h, V, 6.0) == N.PT_E_BAD_ARGUMENT and g._lib.pt_denoise_read_variance(g._h, vp, 0) == N.PT_E_BAD_ARGUMENT
    g.Dispose()


# ------------------------------------------------------------------------------------------------ 4. quality
def test_variance_mode_beats_the_fixed_default_and_the_noisy_image():
    """Default scene, 160x90, aperture 0, ray depth 8; truth = the 1024-frame image of the same handle; MSE of u(c) over the pixels with
    id >= 0.  At F = 1, 4, 16: MSE(variance mode, default sigma_variance) < MSE(fixed mode, defaults) and < MSE(noisy).  Ratios to the
    noisy image's MSE are printed for F = 1, 2, 4, 8, 16, 64."""
    case = fh.Case("default_160x90_ap0", "default", 160, 90, aperture=0.0)
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    got = {}
    for f in range(1, 1025):
        pt.Render()
        if f in (1, 2, 4, 8, 16, 64):
            pt.SetDenoiseMode(N.PT_DENOISE_FIXED)
            fixed = pt.Denoise(0)
            pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
            got[f] = (pt.Result.copy(), fixed, pt.Denoise(0))
    hit = pt.DenoiseGuides()["id"] >= 0
    truth = dr.u_of(pt.Result[..., :3]).astype(np.float64)
    pt.Dispose()
    assert hit.sum() > hit.size / 2

    def mse(img):
        return float(((dr.u_of(img[..., :3]).astype(np.float64) - truth)[hit] ** 2).mean())
    m = {f: tuple(mse(x) for x in imgs) for f, imgs in got.items()}
    for f, (noisy, fixed, var) in m.items():
        print(f"denoise quality F = {f}: MSE(u) noisy {noisy:.6g}; ratio fixed default {fixed / noisy:.4f}, variance mode {var / noisy:.4f}")
    for f in (1, 4, 16):
        noisy, fixed, var = m[f]
        assert var < fixed, f
        assert var < noisy, f


# ------------------------------------------------------------------------------------------------ 5. cost (measured, recorded in DESIGN.md)
def test_cost_is_recorded():
    """1920x1080, default scene, default parameters, pt_timer_*, fastest of three: pt_denoise_render in both modes on the same handle,
    stage V alone and each variance pass alone (pt_debug_denoise_stage).  Printed; no threshold."""
    case = fh.Case("default_1080p", "default", 1920, 1080)
    pt = fh.make_tracer(case, env=env(), ray_depth=13)
    pt.Render()
    pt.Denoise(0)
    pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
    pt.Denoise(0)
    pt.Synchronize()  # (everything warmed up: buffers allocated, code loaded)

    def fastest(fn):
        ms = []
        for _ in range(3):
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)

    def render():
        N.check(pt._lib.pt_denoise_render(pt._h, 0), pt._h)
    times = {"pt_denoise_render, PT_DENOISE_VARIANCE": fastest(render),
             "pt_variance_kernel (stage V)": fastest(lambda: N.debug_denoise_stage(pt._h, 0, -2))}
    for i in range(DEFAULTS.iterations):
        times[f"variance pass {i} (step {1 << i})"] = fastest(lambda: N.debug_denoise_stage(pt._h, 0, i))
    pt.SetDenoiseMode(N.PT_DENOISE_FIXED)
    render()
    times["pt_denoise_render, PT_DENOISE_FIXED"] = fastest(render)
    pt.Dispose()
    print("\n  " + "\n  ".join(f"denoise cost 1080p: {k} {v:.4f} ms" for k, v in times.items()))
    assert all(v > 0 for v in times.values())
