"""The temporal stage of the preview denoiser on the GPU (pt_denoise_set_temporal / pt_denoise_history_clear / pt_denoise_read_integrated /
pt_denoise_read_history; pt_temporal_kernel in csrc/pt_denoise.hip) against its definition: the integrated image equals the numpy float32
restatement (tests/denoise_temporal_reference.py; its own properties: tests/test_denoise_temporal_cpu.py) fed with the GPU's own image
and guides and the history the library reports, on every pixel, bit for bit, and the output equals that image run through the existing
restatement of the mode; sets are promoted by pointer across reset epochs; the history camera is the rounded float64 inverse; the two
existing modes and pt_render do not notice; the argument checks; quality against the filter alone (asserted) and cost (measured), both
recorded in DESIGN.md 3.5."""
import ctypes as C
import dataclasses
from dataclasses import dataclass

import numpy as np
import pytest

import denoise_reference as dr
import denoise_temporal_reference as dt
import denoise_variance_reference as dv
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
DEFAULTS = dr.Params()
SIGMA = dv.DEFAULT_SIGMA_VARIANCE
BY = fh.BY_NAME
SHIFT = (0.3, 0.1, 0.2)


@dataclass(frozen=True)
class TCase:
    name: str
    case: fh.Case
    frames: tuple          # frames rendered in each epoch before its denoise
    moves: tuple           # per later epoch: ("shift", (dx, dy, dz)) | ("turn", (dlook_x, dlook_y)) | ("same", None)
    params: dr.Params = DEFAULTS
    variance: bool = False
    max_history: int = dt.DEFAULT_MAX_HISTORY


def _default(w, h, **kw):
    return fh.Case(f"default_{w}x{h}", "default", w, h, **kw)


def moved(case, move):
    kind, by = move
    if kind == "shift":
        return dataclasses.replace(case, position=tuple(p + d for p, d in zip(case.position, by)))
    if kind == "turn":
        return dataclasses.replace(case, look=(case.look[0] + by[0], case.look[1] + by[1]))
    return case


CASES = [
    # several workgroups in both directions (64x4 tiles), ragged right and top edge
    TCase("shift_131x67", _default(131, 67), (3, 1), (("shift", SHIFT),)),
    TCase("turn_75x43", BY["default_75x43_f0"], (2, 1), (("turn", (5.0, 2.0)),)),
    TCase("same_75x43", BY["default_75x43_f0"], (2, 2), (("same", None),)),
    TCase("n0_75x43", BY["default_75x43_f0"], (2, 0), (("shift", SHIFT),)),             # a reset with no frame rendered yet
    TCase("turn180_64x36", _default(64, 36), (2, 1), (("turn", (180.0, 0.0)),)),        # no pixel finds history
    TCase("incuboid_64x36", BY["incuboid_64x36"], (2, 1), (("shift", (0.05, 0.02, 0.03)),)),  # camera inside cuboid 6: NaN normals
    TCase("edge_64x36", BY["edge_64x36"], (2, 1), (("shift", (0.05, 0.02, 0.03)),)),    # camera inside sphere 0
    TCase("full_64x36", BY["full_64x36"], (2, 1), (("shift", SHIFT),)),
    TCase("empty_16x9", BY["empty_16x9"], (1, 1), (("shift", SHIFT),)),                 # no objects: I == (C, n)
    TCase("default_8x8", BY["default_8x8"], (2, 1), (("shift", SHIFT),)),
    TCase("default_1x1", BY["default_1x1"], (2, 1), (("shift", SHIFT),)),
    TCase("max_history_1", BY["default_75x43_f0"], (3, 1), (("shift", SHIFT),), max_history=1),
    TCase("iterations0", BY["default_75x43_f0"], (2, 1), (("shift", SHIFT),), dr.Params(iterations=0)),
    TCase("variance_shift_131x67", _default(131, 67), (3, 1), (("shift", SHIFT),), variance=True),
    TCase("variance_turn_75x43", BY["default_75x43_f0"], (2, 1), (("turn", (5.0, 2.0)),), variance=True),
    # three epochs A -> B -> C: the history of the third render is itself a blend
    TCase("chain_75x43", BY["default_75x43_f0"], (2, 1, 1), (("shift", SHIFT), ("turn", (5.0, 2.0)))),
]
NON_VACUOUS = ("shift_131x67", "turn_75x43", "same_75x43")
BY_T = {t.name: t for t in CASES}

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


def same_guides(a, b):
    return a.tobytes() == b.tobytes()


def history_refused(pt):
    return pt._lib.pt_denoise_read_history(pt._h, None, None, None, None) == N.PT_E_BAD_ARGUMENT


def new_view(pt, case):
    """A camera move as the host makes it (MainWindow.cs:58-63, 131-132): upload the view, reset the renderer."""
    pt.UploadBasicData(fh.inputs(case)[3])
    pt.ResetRenderer()


def run(tc):
    """-> one dict per epoch: image, n, out, I, guides, history (image, guides, B, O) or None, basic blob, and the restatement's want_I /
    want_out.  Rendered, denoised and restated once per case."""
    if tc.name not in _runs:
        pt = fh.make_tracer(tc.case, env=env(), ray_depth=8)
        p = tc.params
        pt.SetDenoise(p.iterations, p.sigma_color, p.sigma_plane, p.normal_log2_power)
        if tc.variance:
            pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
        pt.SetDenoiseTemporal(True, tc.max_history)
        steps, view = [], tc.case
        for k, frames in enumerate(tc.frames):
            if k > 0:
                view = moved(view, tc.moves[k - 1])
                new_view(pt, view)
            for _ in range(frames):
                pt.Render()
            image = pt.Result.copy()
            out = pt.Denoise(0)
            s = dict(image=image, n=frames, out=out, I=pt.DenoiseIntegrated(), guides=pt.DenoiseGuides(), basic=fh.inputs(view)[3],
                     history=None if k == 0 else pt.DenoiseHistory())
            if k == 0:
                assert history_refused(pt)
            assert pt.FrameIndex == frames and image.tobytes() == pt.Result.tobytes()  # (the image and the counter are where they were)
            steps.append(s)
        pt.Dispose()
        for s in steps:
            hi, hg, B, O = s["history"] if s["history"] else (None, None, None, None)
            s["want_I"] = dt.integrate(s["image"], s["n"], s["guides"], hi, hg, B, O, p, tc.max_history)
            s["want_out"] = dt.filter(s["want_I"], s["guides"], p, SIGMA if tc.variance else None)
        _runs[tc.name] = steps
    return _runs[tc.name]


# ------------------------------------------------------------------------------------------------ 1. I and the output, bit for bit
@pytest.mark.parametrize("tc", CASES, ids=lambda t: t.name)
def test_integrated_image_and_output_equal_the_restatement_on_every_pixel(tc):
    steps = run(tc)
    for k, s in enumerate(steps):
        I, want_I, out, want_out, g = s["I"], s["want_I"], s["out"], s["want_out"], s["guides"]
        assert I.shape == (tc.case.height, tc.case.width, 4) and out.shape == I.shape and g.shape == I.shape[:2]
        hit = g["id"] >= 0
        n = np.float32(s["n"])
        found = (want_I[..., 3] > n) & hit
        bad_I, bad_out = ~same(I, want_I).all(-1), ~same(out, want_out).all(-1)
        print(f"{tc.name} epoch {k}: I: {int(bad_I.sum())} of {bad_I.size} pixels differ from the restatement, output: {int(bad_out.sum())}; "
              f"{int(hit.sum())} pixels with id >= 0, {int(found.sum())} of them with count > n = {s['n']}; max count {float(want_I[..., 3].max())}")
        assert not bad_I.any(), f"{tc.name}/{k}: I first at (y, x) = {np.argwhere(bad_I)[:4].tolist()}: gpu {I[bad_I][:2].tolist()} restatement {want_I[bad_I][:2].tolist()}"
        assert not bad_out.any(), f"{tc.name}/{k}: output first at (y, x) = {np.argwhere(bad_out)[:4].tolist()}: gpu {out[bad_out][:2].tolist()} restatement {want_out[bad_out][:2].tolist()}"
        assert (out[..., 3] == 1.0).all()
        assert (I[..., 3] >= n).all() and (I[..., 3] <= n + np.float32(tc.max_history)).all()
        miss = ~hit
        assert (I[miss][..., 3] == n).all() and same(I[miss][..., :3], s["image"][miss][..., :3]).all()  # a miss passes through
        if k == 0 or tc.case.scene == "empty":
            assert same(I[..., :3], s["image"][..., :3]).all() and (I[..., 3] == n).all()  # no history / nothing to find: I == (C, n)
        if k > 0:
            # promotion: the history is the previous epoch's I and guides, byte for byte
            hi, hg, _, _ = s["history"]
            assert hi.tobytes() == steps[k - 1]["I"].tobytes() and same_guides(hg, steps[k - 1]["guides"])
            if tc.name in NON_VACUOUS or tc.name == "chain_75x43":
                assert found.sum() > hit.sum() / 2, (tc.name, k, int(found.sum()), int(hit.sum()))
            if tc.name == "turn180_64x36":
                assert hit.sum() > 0 and not found.any()
    if tc.name == "chain_75x43":
        assert (steps[1]["I"][..., 3] > 1).any() and (steps[2]["I"][..., 3] > 2).any()  # the third render's history is itself a blend
    if tc.name == "max_history_1":
        assert steps[1]["I"][..., 3].max() == 2.0


# ------------------------------------------------------------------------------------------------ 2. promotion
def test_same_epoch_reuses_the_history_and_clear_forgets_it():
    tc = BY_T["turn_75x43"]
    pt = fh.make_tracer(tc.case, env=env(), ray_depth=8)
    pt.SetDenoiseTemporal(True)
    pt.Render()
    pt.Render()
    pt.Denoise(0)
    first_I, first_g = pt.DenoiseIntegrated(), pt.DenoiseGuides()
    assert history_refused(pt)
    new_view(pt, moved(tc.case, tc.moves[0]))
    pt.Render()
    pt.Denoise(0)
    I1, (h1, g1, B1, O1) = pt.DenoiseIntegrated(), pt.DenoiseHistory()
    assert h1.tobytes() == first_I.tobytes() and same_guides(g1, first_g)
    pt.Denoise(0)  # the same epoch: the same history, integrated afresh — nothing is counted twice
    I2, (h2, g2, B2, O2) = pt.DenoiseIntegrated(), pt.DenoiseHistory()
    assert h2.tobytes() == h1.tobytes() and same_guides(g2, g1) and B2.tobytes() == B1.tobytes() and O2.tobytes() == O1.tobytes()
    assert I2.tobytes() == I1.tobytes() and (I1[..., 3] > 1).any()
    pt.Render()    # ... also with one more frame in the image: n = 2 now, on top of the same history
    image = pt.Result.copy()
    pt.Denoise(0)
    I3, (h3, g3, _, _) = pt.DenoiseIntegrated(), pt.DenoiseHistory()
    assert h3.tobytes() == h1.tobytes() and same_guides(g3, g1)
    assert same(I3, dt.integrate(image, 2, pt.DenoiseGuides(), h3, g3, B1, O1)).all()
    pt.ClearDenoiseHistory()
    assert history_refused(pt)
    new_view(pt, tc.case)
    pt.Render()
    image = pt.Result.copy()
    pt.Denoise(0)
    I4 = pt.DenoiseIntegrated()
    assert history_refused(pt)
    assert same(I4[..., :3], image[..., :3]).all() and (I4[..., 3] == 1.0).all()
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ 3. B and O
@pytest.mark.parametrize("name", ["shift_131x67", "turn_75x43", "incuboid_64x36", "edge_64x36", "chain_75x43"])
def test_history_camera_is_the_rounded_float64_inverse(name):
    steps = run(BY_T[name])
    for k in range(1, len(steps)):
        _, _, B, O = steps[k]["history"]
        blob = steps[k - 1]["basic"]  # the camera the history was made under
        A, _, _ = dt.camera(blob)
        assert O.tobytes() == np.frombuffer(blob, np.float32, 3, 64 + 48).tobytes()
        B64 = np.linalg.inv(A)
        err = np.abs(B.astype(np.float64) - B64).max()
        bound = 2.0 ** -23 * np.abs(B64).max()
        print(f"{name} epoch {k}: max |B - inv(A)| = {err:.3g}, bound {bound:.3g}")
        assert err <= bound


# ------------------------------------------------------------------------------------------------ 4. nothing else notices
@pytest.mark.parametrize("name", ["default_75x43_f0", "incuboid_64x36"])
def test_the_two_modes_with_the_stage_off_are_what_they_were(name):
    case = BY[name]
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    pt.Render()
    pt.Render()

    def both():
        pt.SetDenoiseMode(N.PT_DENOISE_FIXED)
        f, gf = pt.Denoise(1), pt.DenoiseGuides()
        pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE)
        return f, gf, pt.Denoise(1), pt.DenoiseVariance(), pt.DenoiseGuides()
    before = both()  # (pt_denoise_set_temporal was never called on this handle)
    image = pt.Result.copy()
    assert same(before[0], dr.denoise(image, before[1])).all()
    pt.SetDenoiseTemporal(True)
    pt.Denoise(1)
    pt.ResetRenderer()  # a new epoch; the image keeps its contents until the next frame
    pt.Denoise(1)       # n = 0: the history alone
    assert (pt.DenoiseIntegrated()[..., 3] > 0).any() and not history_refused(pt)
    assert pt.Result.tobytes() == image.tobytes()
    pt.SetDenoiseTemporal(False)
    after = both()
    buf = np.empty(image.shape, np.float32)
    assert pt._lib.pt_denoise_read_integrated(pt._h, buf.ctypes.data_as(C.POINTER(C.c_float)), 0) == N.PT_E_BAD_ARGUMENT
    pt.Dispose()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name, batch1", [("default_8x8", False), ("default_75x43_f0", False), ("default_75x43_f0", True)])
def test_render_does_not_notice_the_temporal_stage(name, batch1):
    case = BY[name]

    def go(with_denoise):
        pt = fh.make_tracer(case, env=env(), ray_depth=8)
        if batch1:
            pt.SetFrameBatch(1)  # the frame-fed path
        if with_denoise:
            pt.SetDenoiseTemporal(True)
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


# ------------------------------------------------------------------------------------------------ 5. arguments and scope
def test_error_codes_resize_and_refused_handles():
    case = BY["default_75x43_f0"]
    pt = fh.make_tracer(case, env=env(), ray_depth=2)
    L, h = pt._lib, pt._h
    img = np.empty((43, 75, 4), np.float32)
    ip = img.ctypes.data_as(C.POINTER(C.c_float))
    pt.Render()
    assert L.pt_denoise_read_integrated(h, ip, 0) == N.PT_E_BAD_ARGUMENT and history_refused(pt)  # nothing rendered yet
    # parameters: bad values are refused and the previous ones stay in force
    assert L.pt_denoise_set_temporal(h, 1, 7) == N.PT_OK
    for bad in (-1, 2, 7):
        assert L.pt_denoise_set_temporal(h, bad, 32) == N.PT_E_BAD_ARGUMENT, bad
    for bad in (0, -5, 65536):
        assert L.pt_denoise_set_temporal(h, 1, bad) == N.PT_E_OUT_OF_RANGE, bad
        assert L.pt_denoise_set_temporal(h, 0, bad) == N.PT_E_OUT_OF_RANGE, bad
    assert L.pt_denoise_set_temporal(h, 1, 65535) == N.PT_OK and L.pt_denoise_set_temporal(h, 1, 7) == N.PT_OK
    for _ in range(9):
        pt.Render()
    pt.Denoise(0)
    assert L.pt_denoise_read_integrated(h, ip, 0) == N.PT_OK and (img[..., 3] == 10.0).all()
    assert L.pt_denoise_read_integrated(h, None, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_read_integrated(h, ip, 75 * 16 - 1) == N.PT_E_BAD_ARGUMENT
    new_view(pt, case)
    pt.Render()
    image = pt.Result.copy()
    pt.Denoise(0)
    hi, hg, B, O = pt.DenoiseHistory()
    I = pt.DenoiseIntegrated()
    assert same(I, dt.integrate(image, 1, pt.DenoiseGuides(), hi, hg, B, O, DEFAULTS, 7)).all()  # still on, max_history 7
    assert I[..., 3].max() == 8.0
    pitched = np.full((43, 80, 4), -1.0, np.float32)
    assert L.pt_denoise_read_integrated(h, pitched.ctypes.data_as(C.POINTER(C.c_float)), 80 * 16) == N.PT_OK
    assert same(pitched[:, :75], I).all() and (pitched[:, 75:] == -1.0).all()
    # a render with the stage off leaves no integrated image to read
    pt.SetDenoiseTemporal(False, 7)
    pt.Denoise(0)
    assert L.pt_denoise_read_integrated(h, ip, 0) == N.PT_E_BAD_ARGUMENT
    pt.SetDenoiseTemporal(True, 7)
    pt.Denoise(0)
    assert L.pt_denoise_read_integrated(h, ip, 0) == N.PT_OK and not history_refused(pt)
    # pt_set_size drops both sets
    pt.SetSize(75, 43)
    assert L.pt_denoise_read_integrated(h, ip, 0) == N.PT_E_BAD_ARGUMENT and history_refused(pt)
    pt.Render()
    image = pt.Result.copy()
    pt.Denoise(0)  # (the switch survives a resize)
    assert L.pt_denoise_read_integrated(h, ip, 0) == N.PT_OK and history_refused(pt)
    assert same(img[..., :3], image[..., :3]).all() and (img[..., 3] == 1.0).all()
    # tiled handles are refused by all four calls
    for tile in (lambda: pt.SetTile(8, 16), lambda: pt.SetInterleavedTile(1, 3, 8)):
        tile()
        assert L.pt_denoise_set_temporal(h, 1, 32) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_history_clear(h) == N.PT_E_BAD_ARGUMENT
        assert L.pt_denoise_read_integrated(h, ip, 0) == N.PT_E_BAD_ARGUMENT and history_refused(pt)
    pt.SetTile(0, 43)  # all rows again: the handle owns the whole image
    pt.Render()
    assert L.pt_denoise_set_temporal(h, 1, 32) == N.PT_OK and L.pt_denoise_history_clear(h) == N.PT_OK
    assert L.pt_denoise_render(h, 0) == N.PT_OK and L.pt_denoise_read_integrated(h, ip, 0) == N.PT_OK
    pt.Dispose()
    g = fh.make_tracer(case, devices=[0, 0])
    assert g._lib.pt_denoise_set_temporal(g._h, 1, 32) == N.PT_E_BAD_ARGUMENT and g._lib.pt_denoise_history_clear(g._h) == N.PT_E_BAD_ARGUMENT
    assert g._lib.pt_denoise_read_integrated(g._h, ip, 0) == N.PT_E_BAD_ARGUMENT and history_refused(g)
    g.Dispose()


# ------------------------------------------------------------------------------------------------ 6. quality
def test_temporal_stage_beats_the_filter_alone_after_a_camera_move():
    """Default scene, 160x90, aperture 0, ray depth 8: 16 frames at camera A and a denoise; a shift of (0.3, 0.1, 0.2) to B; reset; 1 frame.
    Truth = the 256-frame image at B on the same handle; MSE of u(c) over the pixels with id >= 0.  MSE(temporal + filter) <
    MSE(filter alone) in both modes; the ratios are printed."""
    case = fh.Case("default_160x90_ap0", "default", 160, 90, aperture=0.0)
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    pt.SetDenoiseTemporal(True)
    for _ in range(16):
        pt.Render()
    pt.Denoise(0)
    new_view(pt, moved(case, ("shift", SHIFT)))
    pt.Render()
    noisy = pt.Result.copy()
    got = {}
    for mode, label in ((N.PT_DENOISE_FIXED, "fixed"), (N.PT_DENOISE_VARIANCE, "variance")):
        pt.SetDenoiseMode(mode)
        pt.SetDenoiseTemporal(True)
        with_t = pt.Denoise(0)  # (the same epoch: both modes integrate the same history afresh)
        integrated = pt.DenoiseIntegrated()
        pt.SetDenoiseTemporal(False)
        got[label] = (with_t, pt.Denoise(0), integrated)
    hit = pt.DenoiseGuides()["id"] >= 0
    for _ in range(255):
        pt.Render()
    assert pt.FrameIndex == 256
    truth = dr.u_of(pt.Result[..., :3]).astype(np.float64)
    pt.Dispose()
    assert hit.sum() > hit.size / 2

    def mse(img):
        return float(((dr.u_of(img[..., :3]).astype(np.float64) - truth)[hit] ** 2).mean())
    m_noisy = mse(noisy)
    found = (got["fixed"][2][..., 3] > 1) & hit
    print(f"temporal quality: {int(found.sum())} of {int(hit.sum())} pixels with id >= 0 found history; MSE(u) noisy {m_noisy:.6g}")
    for label, (with_t, alone, integrated) in got.items():
        mt, ma, mi = mse(with_t), mse(alone), mse(integrated)
        print(f"temporal quality, {label} mode: ratio to the noisy image: filter alone {ma / m_noisy:.4f}, temporal + filter {mt / m_noisy:.4f}, "
              f"integrated image unfiltered {mi / m_noisy:.4f}; temporal + filter / filter alone {mt / ma:.4f}")
        assert mt < ma, label


# ------------------------------------------------------------------------------------------------ 7. cost (measured, recorded in DESIGN.md)
def test_cost_is_recorded():
    """1920x1080, default scene, default parameters, pt_timer_*, fastest of three: the temporal kernel alone and each a-trous pass alone
    (pt_debug_denoise_stage) with a valid history of the same camera, pt_denoise_render with the stage on and off.  Printed; no threshold."""
    case = fh.Case("default_1080p", "default", 1920, 1080)
    pt = fh.make_tracer(case, env=env(), ray_depth=13)
    pt.SetDenoiseTemporal(True)
    pt.Render()
    pt.Denoise(0)
    pt.ResetRenderer()
    pt.Render()
    pt.Denoise(0)
    assert not history_refused(pt)
    pt.Synchronize()  # (everything warmed up: buffers allocated, code loaded, a history in place)

    def fastest(fn):
        ms = []
        for _ in range(3):
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)

    def render():
        N.check(pt._lib.pt_denoise_render(pt._h, 0), pt._h)
    times = {"pt_denoise_render, temporal on": fastest(render),
             "pt_temporal_kernel": fastest(lambda: N.debug_denoise_stage(pt._h, 0, -4)),
             "pt_guides_kernel": fastest(lambda: N.debug_denoise_stage(pt._h, 0, -1))}
    for i in range(DEFAULTS.iterations):
        times[f"pass {i} (step {1 << i})"] = fastest(lambda: N.debug_denoise_stage(pt._h, 0, i))
    pt.SetDenoiseTemporal(False)
    render()
    times["pt_denoise_render, temporal off"] = fastest(render)
    pt.Dispose()
    print("\n  " + "\n  ".join(f"temporal cost 1080p: {k} {v:.4f} ms" for k, v in times.items()))
    assert all(v > 0 for v in times.values())
