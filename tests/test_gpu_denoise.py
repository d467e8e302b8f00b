"""The preview denoiser on the GPU (pt_denoise_render & co., csrc/pt_denoise.hip) against its definition: the a-trous passes equal the
numpy float32 restatement (tests/denoise_reference.py; its own properties: tests/test_denoise_cpu.py) on the GPU's own image and guides
on every pixel, bit for bit; the guides are the first-hit record's ray; pt_render does not notice; the present is the tone map of the
result; quality and cost are measured (recorded in DESIGN.md 3.5, not gated)."""
import ctypes as C
import struct
from dataclasses import dataclass

import numpy as np
import pytest

import denoise_reference as dr
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
DEFAULTS = dr.Params()


@dataclass(frozen=True)
class DCase:
    name: str
    case: fh.Case
    frames: int = 1
    params: dr.Params = DEFAULTS
    guide_frame: int = 0


def _default(w, h, **kw):
    return fh.Case(f"default_{w}x{h}", "default", w, h, **kw)


BY = fh.BY_NAME
CASES = [
    # several workgroups in both directions (16x16 and 64x4 tiles), ragged right and top edge, in-image taps at step 16
    DCase("default_131x67_F1", _default(131, 67), 1),
    DCase("default_131x67_F3", _default(131, 67), 3, guide_frame=2),
    DCase("default_75x43", BY["default_75x43_f0"], 1),
    DCase("default_8x8", BY["default_8x8"], 1),     # every far tap falls off the image
    DCase("default_1x1", BY["default_1x1"], 1),
    DCase("full_64x36", BY["full_64x36"], 2),
    DCase("insphere_64x36", BY["edge_64x36"], 2),   # camera inside sphere 0
    DCase("incuboid_64x36", BY["incuboid_64x36"], 2),  # camera inside cuboid 6: normals seen from inside, sqrt(1/2) components on its edges
    DCase("empty_16x9", BY["empty_16x9"], 1),       # no objects: output == input
    DCase("iterations0", BY["default_75x43_f0"], 1, dr.Params(iterations=0)),
    DCase("iterations1", BY["default_75x43_f0"], 1, dr.Params(iterations=1)),
    DCase("iterations6", _default(131, 67), 1, dr.Params(iterations=6)),
    DCase("sigmas_power", BY["default_75x43_f0"], 2, dr.Params(iterations=4, sigma_color=0.3, sigma_plane=0.05, normal_log2_power=2)),
    DCase("power0_aperture0", BY["default_75x43_ap0"], 1, dr.Params(iterations=3, sigma_color=1.75, sigma_plane=0.004, normal_log2_power=0)),
    DCase("power7", BY["default_75x43_f0"], 1, dr.Params(iterations=2, normal_log2_power=7)),
]
# Non-vacuity: in the default-scene cases with F = 1 the restatement's output differs from its input on more than half of the pixels
# with id >= 0.  The one-pixel image is exempt because no camera can make it hold there: its only tap is the centre, every pass
# returns (w * C) / w, and a correctly rounded product divided by the same w gives C back (measured: 16 cameras and lens settings, all
# 15 round trips of each returned C bit for bit) — the filter of a single sample is the identity.  That case still pins the
# all-taps-off-the-image path bit for bit.
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


def run(dc):
    """-> dict(image, out, guides, first_hit, want): rendered, denoised and restated once per case, then left unchanged."""
    if dc.name not in _runs:
        pt = fh.make_tracer(dc.case, env=env(), ray_depth=8)
        set_params(pt, dc.params)
        for _ in range(dc.frames):
            pt.Render()
        image = pt.Result.copy()
        out = pt.Denoise(dc.guide_frame)
        guides = pt.DenoiseGuides()
        first = pt.FirstHit(dc.guide_frame)
        again = pt.Result.copy()
        frames = pt.FrameIndex
        pt.Dispose()
        assert frames == dc.frames and image.tobytes() == again.tobytes()  # (the image and the counter are where they were)
        r = dict(image=image, out=out, guides=guides, first_hit=first, want=dr.denoise(image, guides, dc.params))
        for a in r.values():
            a.setflags(write=False)
        _runs[dc.name] = r
    return _runs[dc.name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit for bit, NaN == NaN"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------------ 1. the filter, bit for bit
@pytest.mark.parametrize("dc", CASES, ids=lambda d: d.name)
def test_output_equals_the_restatement_on_every_pixel(dc):
    r = run(dc)
    out, want, g = r["out"], r["want"], r["guides"]
    assert out.shape == (dc.case.height, dc.case.width, 4) and g.shape == out.shape[:2]
    ok = same(out, want)
    bad = ~ok.all(-1)
    hit = g["id"] >= 0
    changed = (~same(want[..., :3], r["image"][..., :3]).all(-1)) & hit
    print(f"{dc.name}: {int(bad.sum())} of {bad.size} pixels differ; {int(hit.sum())} pixels with id >= 0, the filter changes {int(changed.sum())} of them")
    assert not bad.any(), f"{dc.name}: first at (y, x) = {np.argwhere(bad)[:4].tolist()}: gpu {out[bad][:2].tolist()} restatement {want[bad][:2].tolist()}"
    assert (out[..., 3] == 1.0).all()
    if dc.params.iterations == 0 or dc.case.scene == "empty":
        assert same(out[..., :3], r["image"][..., :3]).all()
    assert same(out[~hit][..., :3], r["image"][~hit][..., :3]).all()  # a miss passes through
    if dc.name in NON_VACUOUS:
        assert changed.sum() > hit.sum() / 2, f"{dc.name}: the filter changes {int(changed.sum())} of {int(hit.sum())} pixels with id >= 0"


def test_nan_normals_pass_through_on_the_gpu():
    """GetNormal(Cuboid) (compute.glsl:322-332) keeps a component only where |p - centre| is within EPSILON = 0.001 of the half extent,
    and normalises a zero vector to NaN otherwise.  Here a cuboid spans 99990 .. 100010 + 2^-7 in x and z: max + min is an odd multiple
    of 2^-7 above 2^17, where binary32 is spaced 2^-6, so the centre the shader computes is 0.0039 off and no hit on an x or z face lies
    in its band; the y faces (99990 .. 100010) are ordinary.  A NaN centre gets W = 0 and passes through; as a tap it weighs 0."""
    s = pkg.scene
    sc = s.Scene()
    sc.cuboids.append(s.Cuboid(s.vec3(1.0e5), s.vec3(20.0), 0, s.Material(albedo=s.vec3(0.7), emissiv=s.vec3(0.4))))
    blob = bytearray(sc.ubo_bytes())
    lo, hi = np.float32(99990.0), np.float32(100010.0078125)
    assert struct.unpack_from("<3f", blob, 20480) == (lo,) * 3 and struct.unpack_from("<3f", blob, 20496) == (np.float32(100010.0),) * 3
    struct.pack_into("<3f", blob, 20496, hi, 100010.0, hi)  # Cuboids[0].Max (min at byte 20480, max at 20496)
    assert abs(float(hi - (hi + lo) * np.float32(0.5)) - float((hi - lo) * np.float32(0.5))) > 0.003  # the premise, in binary32
    cam = pkg.camera.Camera(position=(1.0e5 + 3.0, 1.0e5 - 2.0, 1.0e5 + 1.0), look_x=30.0, look_y=10.0)
    pt = pkg.PathTracer(env(), W_NAN, H_NAN, 4, 1, 20.0, 0.0)
    objs = np.frombuffer(bytes(blob), dtype=np.uint8)
    pt.GameObjectsUBO.SubData(0, objs.nbytes, objs)
    pt._numSpheres, pt._numCuboids = 0, 1
    pt._push_params()
    pt.UploadBasicData(pkg.camera.basic_data_ubo(cam, W_NAN, H_NAN))
    pt.Render()
    pt.Render()
    image = pt.Result.copy()
    out = pt.Denoise(1)
    g = pt.DenoiseGuides()
    pt.Dispose()
    nan = np.isnan(g["normal"]).any(-1)
    print(f"far cuboid: {int(nan.sum())} NaN normals of {nan.size}, {int((g['id'] == fh.PT_MAX_SPHERES).sum())} hits")
    assert (g["id"] == fh.PT_MAX_SPHERES).all() and nan.any()
    assert same(out, dr.denoise(image, g)).all()
    assert same(out[nan][..., :3], image[nan][..., :3]).all()


W_NAN, H_NAN = 40, 23


# ------------------------------------------------------------------------------------------------ 2. the guides
@pytest.mark.parametrize("dc", CASES[:9], ids=lambda d: d.name)
def test_guides_are_the_first_hit_records_ray(dc):
    r = run(dc)
    g, f = r["guides"], r["first_hit"]
    assert (g["id"] == f["id"]).all() and (_bits(g["t"]) == _bits(f["t"])).all()
    hit = g["id"] >= 0
    with np.errstate(all="ignore"):
        pos = f["dir"] * f["t"][..., None] + f["origin"]  # two float32 operations per component
    assert pos.dtype == np.float32 and (_bits(g["pos"][hit]) == _bits(pos[hit])).all()
    miss = ~hit
    assert (_bits(g["pos"][miss]) == 0).all() and (_bits(g["normal"][miss]) == 0).all() and np.isposinf(g["t"][miss]).all() and (g["id"][miss] == -1).all()
    if dc.case.scene == "empty":
        assert miss.all()


@pytest.mark.parametrize("dc", CASES[:9], ids=lambda d: d.name)
def test_normals(dc):
    """Spheres: within 1e-5 of (pos - centre) / radius in float64 (a few binary32 roundings of a unit-length quantity).  Cuboids:
    GetNormal (compute.glsl:322-332) normalises a vector of -1 / 0 / +1 components, so every component is 0, +-1, +-sqrt(1/2) or
    +-sqrt(1/3) — to 2^-21: the contract's inverse square root is within 1.7 ulp (csrc/pt_math.hpp), the product adds a rounding — or
    the vector was zero and all three are NaN."""
    r = run(dc)
    g = r["guides"]
    blob, ns, nc, _ = fh.inputs(dc.case)
    f = np.frombuffer(blob, np.float32).astype(np.float64)
    sph = (g["id"] >= 0) & (g["id"] < fh.PT_MAX_SPHERES)
    if sph.any():
        geo = f[:20 * ns].reshape(ns, 20)[:, :4][g["id"][sph]]
        want = (g["pos"][sph].astype(np.float64) - geo[:, :3]) / geo[:, 3:4]
        err = np.abs(g["normal"][sph].astype(np.float64) - want).max()
        print(f"{dc.name}: sphere normals within {err:.3g} of (pos - centre) / radius over {int(sph.sum())} pixels")
        assert err <= 1e-5
    cub = g["id"] >= fh.PT_MAX_SPHERES
    if cub.any():
        n = g["normal"][cub].astype(np.float64)
        nan = np.isnan(n)
        assert (nan.all(-1) | ~nan.any(-1)).all()
        allowed = np.array([0.0, 1.0, np.sqrt(0.5), np.sqrt(1.0 / 3.0)])
        dist = np.abs(np.abs(n[~nan])[:, None] - allowed[None, :]).min(-1)
        print(f"{dc.name}: cuboid normal components within {dist.max() if dist.size else 0.0:.3g} of the allowed set; {int(nan.all(-1).sum())} NaN normals of {len(n)}")
        assert dist.size == 0 or dist.max() <= 2.0 ** -21
    if dc.name == "incuboid_64x36":
        assert cub.all()  # the case holds what it is meant to: every ray starts inside the cuboid it hits


# ------------------------------------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("name, batch1", [("default_8x8", False), ("default_75x43_f0", False), ("default_75x43_f0", True)])
def test_render_does_not_notice_the_denoiser(name, batch1):
    case = BY[name]

    def go(with_denoise):
        pt = fh.make_tracer(case, env=env(), ray_depth=8)
        if batch1:
            pt.SetFrameBatch(1)  # the frame-fed path
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


def test_error_codes_resize_and_refused_handles():
    case = BY["default_75x43_f0"]
    pt = fh.make_tracer(case, env=env(), ray_depth=2)
    L, h = pt._lib, pt._h
    img = np.empty((43, 75, 4), np.float32)
    gd = np.empty((43, 75), pkg.path_tracer.GUIDE_DTYPE)
    px = np.empty((43, 75, 4), np.uint8)
    fp, gp, up = img.ctypes.data_as(C.POINTER(C.c_float)), gd.ctypes.data_as(C.c_void_p), px.ctypes.data_as(C.POINTER(C.c_uint8))
    ptr, nbytes = C.c_void_p(), C.c_size_t()

    def four():
        return [L.pt_denoise_read(h, fp, 0), L.pt_denoise_read_guides(h, gp, 0), L.pt_denoise_device_ptr(h, C.byref(ptr), C.byref(nbytes)),
                L.pt_denoise_present_rgba8(h, up, 0)]
    pt.Render()
    assert four() == [N.PT_E_BAD_ARGUMENT] * 4  # nothing rendered yet
    assert L.pt_denoise_render(h, -1) == N.PT_E_BAD_ARGUMENT
    # parameters: bad values are refused and the previous ones stay in force
    assert L.pt_denoise_set_params(h, 2, 0.25, 0.05, 3) == N.PT_OK
    for bad in [(-1, 0.5, 0.02, 5), (7, 0.5, 0.02, 5), (5, 0.0, 0.02, 5), (5, -1.0, 0.02, 5), (5, 0.5, 0.0, 5), (5, 0.5, 0.02, -1), (5, 0.5, 0.02, 8)]:
        assert L.pt_denoise_set_params(h, *bad) == N.PT_E_OUT_OF_RANGE, bad
    for bad in [(5, float("nan"), 0.02, 5), (5, float("inf"), 0.02, 5), (5, 0.5, float("nan"), 5), (5, 0.5, float("-inf"), 5)]:
        assert L.pt_denoise_set_params(h, *bad) == N.PT_E_BAD_ARGUMENT, bad
    image = pt.Result.copy()
    out = pt.Denoise(0)
    assert same(out, dr.denoise(image, pt.DenoiseGuides(), dr.Params(2, 0.25, 0.05, 3))).all()
    assert four() == [N.PT_OK] * 4 and ptr.value and nbytes.value == 43 * 75 * 16
    assert L.pt_denoise_read(h, None, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_read(h, fp, 75 * 16 - 1) == N.PT_E_BAD_ARGUMENT
    assert L.pt_denoise_read_guides(h, None, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_read_guides(h, gp, 75 * 32 - 1) == N.PT_E_BAD_ARGUMENT
    assert L.pt_denoise_present_rgba8(h, None, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_present_rgba8(h, up, 75 * 4 - 1) == N.PT_E_BAD_ARGUMENT
    # pt_set_size frees the buffers: a read after it fails
    pt.SetSize(75, 43)
    assert four() == [N.PT_E_BAD_ARGUMENT] * 4
    pt.Render()
    assert L.pt_denoise_render(h, 0) == N.PT_OK and four() == [N.PT_OK] * 4
    # tiled handles are refused (the filter needs up to 62 halo rows), and the tiling dropped the buffers
    for tile in (lambda: pt.SetTile(8, 16), lambda: pt.SetInterleavedTile(1, 3, 8)):
        tile()
        assert L.pt_denoise_render(h, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_set_params(h, 5, 0.5, 0.02, 5) == N.PT_E_BAD_ARGUMENT
        assert four() == [N.PT_E_BAD_ARGUMENT] * 4
    pt.SetTile(0, 43)  # all rows again: the handle owns the whole image
    pt.Render()
    assert L.pt_denoise_render(h, 0) == N.PT_OK and four() == [N.PT_OK] * 4
    pt.Dispose()
    g = fh.make_tracer(case, devices=[0, 0])
    assert g._lib.pt_denoise_render(g._h, 0) == N.PT_E_BAD_ARGUMENT and g._lib.pt_denoise_set_params(g._h, 5, 0.5, 0.02, 5) == N.PT_E_BAD_ARGUMENT
    assert g._lib.pt_denoise_read(g._h, fp, 0) == N.PT_E_BAD_ARGUMENT and g._lib.pt_denoise_device_ptr(g._h, C.byref(ptr), C.byref(nbytes)) == N.PT_E_BAD_ARGUMENT
    g.Dispose()


@pytest.mark.parametrize("mode", [N.PT_ARITH_CONTRACT, N.PT_ARITH_REFERENCE], ids=["contract", "reference"])
def test_present_is_the_tone_map_of_the_denoised_image(mode):
    case = BY["default_75x43_f0"]
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    for _ in range(2):
        pt.Render()
    pt.SetPresentArithmetic(mode)
    out = pt.Denoise(0)
    shown = pt.PresentDenoised()
    raw = pt.Present()
    other = fh.make_tracer(case)
    other.SetPresentArithmetic(mode)
    other.WriteResult(out, 2)
    want = other.Present()
    other.Dispose()
    pt.Dispose()
    assert shown.tobytes() == want.tobytes()
    assert shown.tobytes() != raw.tobytes()  # (and it is not the raw image's present)


# ------------------------------------------------------------------------------------------------ 4. quality (measured, recorded in DESIGN.md)
def test_denoised_early_frames_are_closer_to_the_converged_image():
    """Default scene, 160x90, aperture 0; ground truth = the 256-frame image of the same handle; MSE on u(c) over the pixels with id >= 0."""
    case = fh.Case("default_160x90_ap0", "default", 160, 90, aperture=0.0)
    pt = fh.make_tracer(case, env=env(), ray_depth=8)
    got = {}
    for f in range(1, 257):
        pt.Render()
        if f in (1, 4):
            got[f] = (pt.Result.copy(), pt.Denoise(0))
    hit = pt.DenoiseGuides()["id"] >= 0
    truth = dr.u_of(pt.Result[..., :3]).astype(np.float64)
    pt.Dispose()
    assert hit.sum() > hit.size / 2
    for f, (noisy, den) in got.items():
        mse_n = float(((dr.u_of(noisy[..., :3]).astype(np.float64) - truth)[hit] ** 2).mean())
        mse_d = float(((dr.u_of(den[..., :3]).astype(np.float64) - truth)[hit] ** 2).mean())
        print(f"denoise quality F = {f}: MSE(u) noisy {mse_n:.6g}, denoised {mse_d:.6g}, ratio {mse_d / mse_n:.4f}")
        assert mse_d < mse_n, f


# ------------------------------------------------------------------------------------------------ 5. cost (measured, recorded in DESIGN.md)
def test_cost_is_recorded():
    """1920x1080, default scene, default parameters, pt_timer_*, fastest of three: pt_denoise_render in total, the guide kernel alone and
    each pass (pt_debug_denoise_stage), one pt_render frame and pt_postprocess_device on the same handle.  Printed; no threshold."""
    case = fh.Case("default_1080p", "default", 1920, 1080)
    pt = fh.make_tracer(case, env=env(), ray_depth=13)
    pt.Render()
    pt.Denoise(0)
    pt.PostProcessDevice()
    pt.Synchronize()  # (everything warmed up: buffers allocated, code loaded)

    def fastest(fn):
        ms = []
        for _ in range(3):
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)
    times = {"pt_denoise_render": fastest(lambda: N.check(pt._lib.pt_denoise_render(pt._h, 0), pt._h)),
             "pt_guides_kernel": fastest(lambda: N.debug_denoise_stage(pt._h, 0, -1))}
    for i in range(DEFAULTS.iterations):
        times[f"pass {i} (step {1 << i})"] = fastest(lambda: N.debug_denoise_stage(pt._h, 0, i))
    times["pt_render, one frame"] = fastest(pt.Render)
    times["pt_postprocess_device"] = fastest(pt.PostProcessDevice)
    pt.Dispose()
    print("\n  " + "\n  ".join(f"denoise cost 1080p: {k} {v:.4f} ms" for k, v in times.items()))
    assert all(v > 0 for v in times.values())
