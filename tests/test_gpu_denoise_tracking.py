"""Object tracking of the temporal stage on the GPU (pt_denoise_set_object_tracking / pt_denoise_read_object_map;
pt_temporal_tracked_kernel in csrc/pt_denoise.hip, denoise_object_map in csrc/mi355pt_queries.cpp) against its definition: after an edit
made as the host makes it (patch the object, pt_upload_game_objects, pt_reset) the integrated image equals the numpy float32 restatement
(tests/denoise_tracking_reference.py; its own properties: tests/test_denoise_tracking_cpu.py) fed with the GPU's own image and guides and
the map and history the library reports, on every pixel, bit for bit, and the output equals that image run through the existing
restatement of the mode; the map equals the restated classification; with the switch off, or the scene unchanged, nothing differs from
the untracked stage; pt_render does not notice; the argument checks; quality against a cleared history and against the switch off
(asserted) and cost (measured), both recorded in DESIGN.md 3.5."""
import ctypes as C
import dataclasses
from dataclasses import dataclass

import numpy as np
import pytest

import denoise_reference as dr
import denoise_temporal_reference as dt
import denoise_tracking_reference as dk
import denoise_variance_reference as dv
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
DEFAULTS = dr.Params()
SIGMA = dv.DEFAULT_SIGMA_VARIANCE
BY = fh.BY_NAME
SHIFT = (0.3, 0.1, 0.2)
F = np.float32
# the object the edits are made to: sphere 3 of the default scene — specular chance 0 (diffuse), centre (-12, 1.3, -5), radius 1.3, the
# large sphere at the lower right of the default view (148 pixels at 75x43, 707 at 160x90) — and cuboid 2, the room's back wall behind it
SPHERE, CUBOID = 3, 2
QUALITY_STEP = (0.0, 0.5, 0.0)  # about 7 pixels upwards at 160x90
QUALITY_ALBEDO = (0.9, 0.2, 0.2)


@dataclass(frozen=True)
class TCase:
    name: str
    case: fh.Case
    frames: tuple                # frames rendered in each epoch before its denoise
    edits: tuple                 # per later epoch: a tuple of operations, see apply()
    variance: bool = False
    max_history: int = dt.DEFAULT_MAX_HISTORY
    edit_max_history: int = 0
    moved: tuple = ()            # guide ids whose move must be seen to matter (non-vacuity)
    dropped: tuple = ()          # guide ids whose material changed


def _default(w, h, **kw):
    return fh.Case(f"default_{w}x{h}", "default", w, h, **kw)


C75, C131 = BY["default_75x43_f0"], _default(131, 67)
CASES = [
    TCase("move_sphere_75x43", C75, (3, 1), ((("move_sphere", SPHERE, (0.0, 0.3, 0.0)),),), moved=(SPHERE,)),
    # several workgroups in both directions (64x4 tiles), ragged right and top edge
    TCase("move_sphere_131x67", C131, (3, 1), ((("move_sphere", SPHERE, (0.1, 0.3, -0.2)),),), moved=(SPHERE,)),
    TCase("move_cuboid_131x67", C131, (3, 1), ((("move_cuboid", CUBOID, (0.5, 0.25, 0.1)),),), moved=(256 + CUBOID,)),
    TCase("radius_75x43", C75, (3, 1), ((("radius", SPHERE, 1.5),),), moved=(SPHERE,)),
    TCase("albedo_75x43", C75, (3, 1), ((("albedo", SPHERE, QUALITY_ALBEDO),),), dropped=(SPHERE,)),
    TCase("move_and_camera_75x43", C75, (3, 1), ((("move_sphere", SPHERE, (0.0, 0.3, 0.0)), ("camera", ("shift", SHIFT))),), moved=(SPHERE,)),
    # three epochs: the history of the third render is itself a tracked blend
    TCase("drag_75x43", C75, (2, 1, 1), ((("move_sphere", SPHERE, (0.0, 0.2, 0.0)),), (("move_sphere", SPHERE, (0.0, 0.2, 0.0)),)), moved=(SPHERE,)),
    TCase("one_sphere_less_75x43", C75, (3, 1), ((("spheres", -1),),)),
    TCase("edit_max_history_1_75x43", C75, (3, 1), ((("move_sphere", SPHERE, (0.0, 0.3, 0.0)),),), edit_max_history=1, moved=(SPHERE,)),
    TCase("variance_131x67", C131, (3, 1), ((("move_sphere", SPHERE, (0.1, 0.3, -0.2)),),), variance=True, moved=(SPHERE,)),
    # all 320 slots in use: sphere 194 (the stress scene's largest on screen) and cuboid 49 (one of the small boxes in front of the room)
    TCase("full_64x36", BY["full_64x36"], (2, 1), ((("move_sphere", 194, (0.1, 0.1, 0.0)), ("move_cuboid", 49, (0.1, 0.0, 0.05)), ("albedo", 176, (0.1, 0.9, 0.1))),)),
    TCase("default_8x8", BY["default_8x8"], (2, 1), ((("move_cuboid", 0, (0.25, 0.0, 0.25)), ("move_sphere", 9, (0.05, 0.0, 0.0))),)),
    TCase("default_1x1", BY["default_1x1"], (2, 1), ((("move_cuboid", 0, (0.25, 0.0, 0.25)),),)),
]
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


def map_refused(pt):
    return pt._lib.pt_denoise_read_object_map(pt._h, None, None) == N.PT_E_BAD_ARGUMENT


def moved_view(case, move):
    kind, by = move
    if kind == "shift":
        return dataclasses.replace(case, position=tuple(p + d for p, d in zip(case.position, by)))
    return dataclasses.replace(case, look=(case.look[0] + by[0], case.look[1] + by[1]))


class World:
    """A tracer and the host's own scene objects (Sphere.cs / Cuboid.cs as scene.py mirrors them): an edit changes an object and uploads
    its bytes at its BufferOffset, as Gui.cs:212-216 does; reset() is the ResetRenderer that follows."""

    def __init__(self, case, ray_depth=8):
        self.scene = fh.make_scene(case.scene)
        self.view = case
        self.pt = fh.make_tracer(case, env=env(), ray_depth=ray_depth)
        self.ns, self.nc = self.scene.num_spheres, self.scene.num_cuboids

    def upload(self, obj):
        data = obj.gpu_data()
        self.pt.GameObjectsUBO.SubData(obj.buffer_offset, data.nbytes, data)

    def apply(self, op):
        kind = op[0]
        if kind == "move_sphere":
            s = self.scene.spheres[op[1]]
            s.position = (s.position + np.asarray(op[2], F)).astype(F)
            self.upload(s)
        elif kind == "move_cuboid":  # (Min / Max = Position -+ Dimensions / 2, rounded again: Cuboid.cs:23-24)
            c = self.scene.cuboids[op[1]]
            c.position = (c.position + np.asarray(op[2], F)).astype(F)
            self.upload(c)
        elif kind == "radius":
            self.scene.spheres[op[1]].radius = F(op[2])
            self.upload(self.scene.spheres[op[1]])
        elif kind == "albedo":
            s = self.scene.spheres[op[1]]
            s.material = dataclasses.replace(s.material, albedo=np.asarray(op[2], F))  # (a material of its own: the stress scene shares them)
            self.upload(s)
        elif kind == "spheres":
            self.ns += op[1]
            self.pt._numSpheres = self.ns
            self.pt._push_params()
        elif kind == "camera":
            self.view = moved_view(self.view, op[1])
            self.pt.UploadBasicData(fh.inputs(self.view)[3])
        else:
            raise ValueError(kind)

    def reset(self):
        self.pt.ResetRenderer()

    def snapshot(self):
        return self.scene.ubo_bytes(), self.ns, self.nc


def run(tc):
    """-> one dict per epoch: image, n, out, I, guides, history, the map and flag read back, the scene snapshot, and the restatement's
    map, want_I / want_out and the untracked definition's I on the same inputs.  Rendered, denoised and restated once per case."""
    if tc.name not in _runs:
        w = World(tc.case)
        pt = w.pt
        if tc.variance:
            pt.SetDenoiseMode(N.PT_DENOISE_VARIANCE, SIGMA)
        pt.SetDenoiseTemporal(True, tc.max_history)
        pt.SetDenoiseTracking(True, tc.edit_max_history)
        steps = []
        for k, frames in enumerate(tc.frames):
            if k > 0:
                for op in tc.edits[k - 1]:
                    w.apply(op)
                w.reset()
            for _ in range(frames):
                pt.Render()
            image = pt.Result.copy()
            out = pt.Denoise(0)
            s = dict(image=image, n=frames, out=out, I=pt.DenoiseIntegrated(), guides=pt.DenoiseGuides(), scene=w.snapshot(),
                     history=None if k == 0 else pt.DenoiseHistory(), map=None if k == 0 else pt.DenoiseObjectMap())
            if k == 0:
                assert map_refused(pt)  # no history: no map
            assert pt.FrameIndex == frames and image.tobytes() == pt.Result.tobytes()  # (the image and the counter are where they were)
            steps.append(s)
        pt.Dispose()
        cap = dk.cap_of(tc.max_history, tc.edit_max_history)
        for k, s in enumerate(steps):
            args = (s["image"], s["n"], s["guides"]) + (s["history"] if s["history"] else (None, None, None, None))
            s["untracked_I"] = dt.integrate(*args, DEFAULTS, tc.max_history)
            if k == 0:
                s["want_map"], s["want_I"] = None, s["untracked_I"]
            else:
                prev, cur = steps[k - 1]["scene"], s["scene"]
                s["want_map"] = dk.object_map(prev[0], prev[1], prev[2], cur[0], cur[1], cur[2])
                s["want_I"] = dk.integrate_tracked(*args, s["map"][0], DEFAULTS, cap) if s["want_map"].tracked else s["untracked_I"]
            s["want_out"] = dt.filter(s["want_I"], s["guides"], DEFAULTS, SIGMA if tc.variance else None)
        _runs[tc.name] = steps
    return _runs[tc.name]


# ------------------------------------------------------------------------------------------------ 1. I and the output, bit for bit
@pytest.mark.parametrize("tc", CASES, ids=lambda t: t.name)
def test_integrated_image_and_output_equal_the_restatement_on_every_pixel(tc):
    steps = run(tc)
    cap = dk.cap_of(tc.max_history, tc.edit_max_history)
    for k, s in enumerate(steps):
        I, want_I, out, want_out, g = s["I"], s["want_I"], s["out"], s["want_out"], s["guides"]
        assert I.shape == (tc.case.height, tc.case.width, 4) and out.shape == I.shape and g.shape == I.shape[:2]
        n = F(s["n"])
        bad_I, bad_out = ~same(I, want_I).all(-1), ~same(out, want_out).all(-1)
        differs = ~same(want_I, s["untracked_I"]).all(-1)
        print(f"{tc.name} epoch {k}: I: {int(bad_I.sum())} of {bad_I.size} pixels differ from the restatement, output: {int(bad_out.sum())}; "
              f"{int((g['id'] >= 0).sum())} pixels with id >= 0, {int((want_I[..., 3] > n).sum())} with count > n = {s['n']}, "
              f"{int(differs.sum())} where the untracked definition gives another I; max count {float(want_I[..., 3].max())}")
        assert not bad_I.any(), f"{tc.name}/{k}: I first at (y, x) = {np.argwhere(bad_I)[:4].tolist()}: gpu {I[bad_I][:2].tolist()} restatement {want_I[bad_I][:2].tolist()}"
        assert not bad_out.any(), f"{tc.name}/{k}: output first at (y, x) = {np.argwhere(bad_out)[:4].tolist()}: gpu {out[bad_out][:2].tolist()} restatement {want_out[bad_out][:2].tolist()}"
        assert (out[..., 3] == 1.0).all()
        assert (I[..., 3] >= n).all() and (I[..., 3] <= n + F(cap if k > 0 else tc.max_history)).all()
        miss = g["id"] < 0
        assert (I[miss][..., 3] == n).all() and same(I[miss][..., :3], s["image"][miss][..., :3]).all()  # a miss passes through
        if k == 0:
            continue
        hi, hg, _, _ = s["history"]  # promotion as before: the history is the previous epoch's I and guides, byte for byte
        assert hi.tobytes() == steps[k - 1]["I"].tobytes() and hg.tobytes() == steps[k - 1]["guides"].tobytes()
        assert s["map"][1] is True  # every case edits the scene: the tracked kernel ran
        # non-vacuity: the move is seen, and the map matters
        for obj in tc.moved:
            on = g["id"] == obj
            assert on.any() and (I[on][..., 3] > n).any(), (tc.name, k, obj, int(on.sum()))
            assert differs[on].any(), (tc.name, k, obj)
        for obj in tc.dropped:
            on = g["id"] == obj
            assert on.any() and (I[on][..., 3] == n).all() and (s["untracked_I"][on][..., 3] > n).any(), (tc.name, k, obj)
        # the objects nobody touched keep their history: most of the other hit pixels still find it
        rest = (g["id"] >= 0) & ~np.isin(g["id"], tc.moved + tc.dropped)
        if tc.case.width >= 64 and tc.name != "move_and_camera_75x43":
            assert (I[rest][..., 3] > n).mean() > 0.5, (tc.name, k)
    if tc.name == "drag_75x43":
        on = steps[2]["guides"]["id"] == SPHERE
        assert (steps[1]["I"][..., 3] > 1).any() and (steps[2]["I"][on][..., 3] > 2).any()  # the third render's history is itself a tracked blend
    if tc.name == "edit_max_history_1_75x43":
        assert steps[1]["I"][..., 3].max() == 2.0


# ------------------------------------------------------------------------------------------------ 2. the map
@pytest.mark.parametrize("tc", CASES, ids=lambda t: t.name)
def test_object_map_read_back_equals_the_restated_classification(tc):
    steps = run(tc)
    for k in range(1, len(steps)):
        got, tracked = steps[k]["map"]
        want = steps[k]["want_map"]
        _, ns, nc = steps[k]["scene"]
        assert got.shape == (dk.ENTRIES,) and got.dtype.itemsize == 32
        assert tracked == want.tracked and (got["state"] == want.states).all(), np.argwhere(got["state"] != want.states)[:8].tolist()
        assert (got["zero"] == 0).all()
        bound = 2.0 ** -23 * max(np.abs(want.a64).max(), np.abs(want.b64).max())
        err = max(np.abs(got["a"].astype(np.float64) - want.a64).max(), np.abs(got["b"].astype(np.float64) - want.b64).max())
        count = {name: int((got["state"] == v).sum()) for name, v in (("KEEP", dk.KEEP), ("MOVED", dk.MOVED), ("DROP", dk.DROP))}
        print(f"{tc.name} epoch {k}: {count}; max |a, b - float64| = {err:.3g}, bound {bound:.3g}")
        assert err <= bound
        assert (got["state"][ns:256] == dk.DROP).all() and (got["state"][256 + nc:] == dk.DROP).all()  # beyond the counts
        keep = got["state"] == dk.KEEP
        assert (got["a"][keep] == 1).all() and (got["b"][keep] == 0).all()
        for obj in tc.moved:
            assert got["state"][obj] == dk.MOVED
        for obj in tc.dropped:
            assert got["state"][obj] == dk.DROP


# ------------------------------------------------------------------------------------------------ 3. switch off / scene unchanged
def test_switch_off_is_the_untracked_stage_and_an_unchanged_scene_is_untracked():
    w = World(C75)
    pt = w.pt
    pt.SetDenoiseTemporal(True)
    pt.SetDenoiseTracking(True)
    for _ in range(3):
        pt.Render()
    pt.Denoise(0)
    # (a) switch on, camera move only: the untracked kernel, bit for bit the switch-off result
    w.apply(("camera", ("shift", SHIFT)))
    w.reset()
    pt.Render()
    image = pt.Result.copy()
    on = pt.Denoise(0), pt.DenoiseIntegrated()
    table, tracked = pt.DenoiseObjectMap()
    assert tracked is False
    assert (table["state"][:w.ns] == dk.KEEP).all() and (table["state"][256:256 + w.nc] == dk.KEEP).all() and (table["state"] == dk.DROP).sum() == 320 - w.ns - w.nc
    hist = pt.DenoiseHistory()
    pt.SetDenoiseTracking(False)
    off = pt.Denoise(0), pt.DenoiseIntegrated()  # (the same epoch: the same history, integrated afresh)
    assert map_refused(pt)
    assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
    want = dt.integrate(image, 1, pt.DenoiseGuides(), *hist)
    assert same(on[1], want).all() and (on[1][..., 3] > 1).any()
    # (b) switch off, scene edited: the untracked definition, as before this switch existed
    w.apply(("move_sphere", SPHERE, (0.0, 0.3, 0.0)))
    w.apply(("albedo", 4, QUALITY_ALBEDO))
    w.reset()
    pt.Render()
    image = pt.Result.copy()
    out, I, g, hist = pt.Denoise(0), pt.DenoiseIntegrated(), pt.DenoiseGuides(), pt.DenoiseHistory()
    assert map_refused(pt)
    want = dt.integrate(image, 1, g, *hist)
    assert same(I, want).all() and same(out, dt.filter(want, g)).all()
    assert (I[g["id"] == 4][..., 3] > 1).any()  # the recoloured sphere still drags its old colour along
    # ... and the snapshot was kept all the while: switched on again in the same epoch, the edit is seen
    pt.SetDenoiseTracking(True)
    pt.Denoise(0)
    table, tracked = pt.DenoiseObjectMap()
    assert tracked is True and table["state"][SPHERE] == dk.MOVED and table["state"][4] == dk.DROP
    I2 = pt.DenoiseIntegrated()
    assert same(I2, dk.integrate_tracked(image, 1, g, *hist, table)).all() and (I2[g["id"] == 4][..., 3] == 1).all()
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ 4. pt_render does not notice
@pytest.mark.parametrize("name, batch1", [("default_8x8", False), ("default_75x43_f0", False), ("default_75x43_f0", True)])
def test_render_does_not_notice_a_tracked_denoise(name, batch1):
    def go(with_denoise):
        w = World(BY[name])
        pt = w.pt
        if batch1:
            pt.SetFrameBatch(1)  # the frame-fed path
        if with_denoise:
            pt.SetDenoiseTemporal(True)
            pt.SetDenoiseTracking(True)
        pt.Render()
        if with_denoise:
            pt.Denoise(0)
        w.apply(("move_sphere", 9, (0.05, 0.1, 0.0)))
        w.reset()
        for f in range(8):
            pt.Render()
            if f < 7:
                if with_denoise:
                    pt.Denoise(f)
                    assert pt.DenoiseObjectMap()[1] is True
                w.upload(w.scene.spheres[9])  # an edit-free upload (Gui.cs:212-216 re-uploads the picked object, changed or not)
        img, frames = pt.Result.copy(), pt.FrameIndex
        pt.Dispose()
        return img, frames
    plain, with_d = go(False), go(True)
    assert plain[1] == with_d[1] == 8
    assert (_bits(plain[0]) == _bits(with_d[0])).all()
    assert np.isfinite(plain[0]).all() and plain[0][..., :3].max() > 0


# ------------------------------------------------------------------------------------------------ 5. arguments and scope
def test_error_codes_resize_and_refused_handles():
    w = World(C75, ray_depth=2)
    pt = w.pt
    L, h = pt._lib, pt._h
    buf = np.zeros(dk.ENTRIES, dk.MAP_DTYPE)
    bp, flag = buf.ctypes.data_as(C.c_void_p), C.c_int(-7)
    pt.Render()
    assert map_refused(pt)  # nothing rendered yet
    # parameters: bad values are refused and the previous ones (on, 2) stay in force — the render below shows it
    assert L.pt_denoise_set_temporal(h, 1, 32) == N.PT_OK
    assert L.pt_denoise_set_object_tracking(h, 1, 65535) == N.PT_OK and L.pt_denoise_set_object_tracking(h, 0, 0) == N.PT_OK
    assert L.pt_denoise_set_object_tracking(h, 1, 2) == N.PT_OK
    for bad in (-1, 2, 7):
        assert L.pt_denoise_set_object_tracking(h, bad, 0) == N.PT_E_BAD_ARGUMENT, bad
    for bad in (-1, -5, 65536):
        assert L.pt_denoise_set_object_tracking(h, 1, bad) == N.PT_E_OUT_OF_RANGE, bad
        assert L.pt_denoise_set_object_tracking(h, 0, bad) == N.PT_E_OUT_OF_RANGE, bad
    pt.Render()
    pt.Render()
    pt.Denoise(0)  # (3 frames: the history brings more than edit_max_history along)
    assert map_refused(pt)  # a render without a history builds no map
    w.apply(("move_sphere", SPHERE, (0.0, 0.3, 0.0)))
    w.reset()
    pt.Render()
    image = pt.Result.copy()
    pt.Denoise(0)
    assert L.pt_denoise_read_object_map(h, bp, C.byref(flag)) == N.PT_OK and flag.value == 1 and buf["state"][SPHERE] == dk.MOVED
    assert L.pt_denoise_read_object_map(h, None, C.byref(flag)) == N.PT_OK and L.pt_denoise_read_object_map(h, bp, None) == N.PT_OK
    I = pt.DenoiseIntegrated()
    assert same(I, dk.integrate_tracked(image, 1, pt.DenoiseGuides(), *pt.DenoiseHistory(), buf, DEFAULTS, 2)).all()  # still on, edit_max_history 2
    assert I[..., 3].max() == 3.0
    # the switch or the stage off: no map
    pt.SetDenoiseTracking(False, 2)
    pt.Denoise(0)
    assert map_refused(pt)
    pt.SetDenoiseTracking(True, 2)
    pt.Denoise(0)
    assert not map_refused(pt)
    pt.SetDenoiseTemporal(False)
    pt.Denoise(0)
    assert map_refused(pt)
    pt.SetDenoiseTemporal(True)
    pt.Denoise(0)
    assert not map_refused(pt)
    pt.ClearDenoiseHistory()
    assert map_refused(pt)
    pt.Denoise(0)
    assert map_refused(pt)  # (both sets were forgotten: this render had no history)
    # pt_set_size frees the buffers, the map's among them; the switch survives; the map is refused until a render has a history again
    w.reset()
    pt.Render()
    pt.Denoise(0)
    assert not map_refused(pt)
    pt.SetSize(75, 43)
    assert map_refused(pt)
    for _ in range(3):
        pt.Render()
    pt.Denoise(0)
    assert map_refused(pt)
    w.apply(("move_sphere", SPHERE, (0.0, -0.3, 0.0)))
    w.reset()
    pt.Render()
    pt.Denoise(0)
    assert L.pt_denoise_read_object_map(h, bp, C.byref(flag)) == N.PT_OK and flag.value == 1 and buf["state"][SPHERE] == dk.MOVED
    assert pt.DenoiseIntegrated()[..., 3].max() == 3.0
    # tiled handles are refused by both calls
    for tile in (lambda: pt.SetTile(8, 16), lambda: pt.SetInterleavedTile(1, 3, 8)):
        tile()
        assert L.pt_denoise_set_object_tracking(h, 1, 0) == N.PT_E_BAD_ARGUMENT and L.pt_denoise_read_object_map(h, bp, C.byref(flag)) == N.PT_E_BAD_ARGUMENT
    pt.SetTile(0, 43)  # all rows again: the handle owns the whole image
    pt.Render()
    assert L.pt_denoise_set_object_tracking(h, 1, 0) == N.PT_OK and L.pt_denoise_render(h, 0) == N.PT_OK and map_refused(pt)
    pt.Dispose()
    g = fh.make_tracer(C75, devices=[0, 0])
    assert g._lib.pt_denoise_set_object_tracking(g._h, 1, 0) == N.PT_E_BAD_ARGUMENT
    assert g._lib.pt_denoise_read_object_map(g._h, bp, C.byref(flag)) == N.PT_E_BAD_ARGUMENT
    g.Dispose()


# ------------------------------------------------------------------------------------------------ 6. quality
def quality(op):
    """Default scene, 160x90, aperture 0, ray depth 8: 16 frames and a denoise; the edit; reset; 1 frame; then, in the same epoch, the
    denoise with tracking on, with it off, and with the history cleared.  Truth = the 256-frame image of the edited scene on the same
    handle.  -> MSE of u(c) per variant over the pixels of sphere SPHERE and over all pixels with id >= 0, and the noisy image's."""
    w = World(fh.Case("default_160x90_ap0", "default", 160, 90, aperture=0.0))
    pt = w.pt
    pt.SetDenoiseTemporal(True)
    pt.SetDenoiseTracking(True)
    for _ in range(16):
        pt.Render()
    pt.Denoise(0)
    w.apply(op)
    w.reset()
    pt.Render()
    got = {"noisy": pt.Result.copy(), "tracked": pt.Denoise(0)}
    assert pt.DenoiseObjectMap()[1] is True
    ids = pt.DenoiseGuides()["id"]
    pt.SetDenoiseTracking(False)
    got["switch off"] = pt.Denoise(0)
    pt.ClearDenoiseHistory()
    got["history cleared"] = pt.Denoise(0)
    assert (pt.DenoiseIntegrated()[..., 3] == 1.0).all()
    for _ in range(255):
        pt.Render()
    assert pt.FrameIndex == 256
    truth = dr.u_of(pt.Result[..., :3]).astype(np.float64)
    pt.Dispose()
    on, hit = ids == SPHERE, ids >= 0
    assert on.sum() > 300 and hit.sum() > hit.size / 2

    def mse(img, where):
        return float(((dr.u_of(img[..., :3]).astype(np.float64) - truth)[where] ** 2).mean())
    return {k: (mse(v, on), mse(v, hit)) for k, v in got.items()}


def report(label, m):
    for k in ("tracked", "switch off", "history cleared"):
        print(f"tracking quality, {label}: {k}: MSE(u) over the sphere {m[k][0]:.6g} ({m[k][0] / m['noisy'][0]:.4f} of the 1-frame image's), "
              f"over all hit pixels {m[k][1]:.6g} ({m[k][1] / m['noisy'][1]:.4f})")
    print(f"tracking quality, {label}: over the sphere tracked / history cleared {m['tracked'][0] / m['history cleared'][0]:.4f}, tracked / switch off "
          f"{m['tracked'][0] / m['switch off'][0]:.4f}; over all hit pixels tracked / history cleared {m['tracked'][1] / m['history cleared'][1]:.4f}")


def test_tracking_beats_a_cleared_history_and_the_switch_off_after_a_move():
    """(a) sphere 3 moved by (0, 0.5, 0): over its pixels tracked < history cleared and tracked < switch off; over all hit pixels
    tracked < history cleared.  The ratios are printed."""
    m = quality(("move_sphere", SPHERE, QUALITY_STEP))
    report("sphere 3 moved by (0, 0.5, 0)", m)
    assert m["tracked"][0] < m["history cleared"][0]
    assert m["tracked"][0] < m["switch off"][0]
    assert m["tracked"][1] < m["history cleared"][1]


def test_tracking_beats_the_switch_off_after_an_albedo_edit():
    """(b) sphere 3's albedo changed to (0.9, 0.2, 0.2): over its pixels tracked < switch off.  The ratios are printed."""
    m = quality(("albedo", SPHERE, QUALITY_ALBEDO))
    report("sphere 3 albedo (0.9, 0.2, 0.2)", m)
    assert m["tracked"][0] < m["switch off"][0]


# ------------------------------------------------------------------------------------------------ 7. cost (measured, recorded in DESIGN.md)
def test_cost_is_recorded():
    """1920x1080, default scene, one sphere moved, pt_timer_*, fastest of three: the tracked temporal kernel and pt_temporal_kernel<2> alone
    (pt_debug_denoise_stage -4) on the same handle, between the same buffers.  Printed, as the other cost tests print theirs; no threshold."""
    w = World(fh.Case("default_1080p", "default", 1920, 1080), ray_depth=13)
    pt = w.pt
    pt.SetDenoiseTemporal(True)
    pt.SetDenoiseTracking(True)
    pt.Render()
    pt.Denoise(0)
    w.apply(("move_sphere", SPHERE, QUALITY_STEP))
    w.reset()
    pt.Render()
    pt.Denoise(0)
    assert pt.DenoiseObjectMap()[1] is True
    pt.Synchronize()  # (everything warmed up: buffers allocated, code loaded, a history and a map in place)

    def fastest(fn):
        ms = []
        for _ in range(3):
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)
    times = {"pt_temporal_tracked_kernel<2>": fastest(lambda: N.debug_denoise_stage(pt._h, 0, -4))}
    pt.SetDenoiseTracking(False)  # (stage -4 runs the kernel the switch selects: the untracked one over the same sets)
    N.debug_denoise_stage(pt._h, 0, -4)
    times["pt_temporal_kernel<2>"] = fastest(lambda: N.debug_denoise_stage(pt._h, 0, -4))
    pt.Dispose()
    lines = [f"tracking cost 1080p: {k} {v:.4f} ms" for k, v in times.items()]
    print("\n  " + "\n  ".join(lines))
    assert all(v > 0 for v in times.values())
