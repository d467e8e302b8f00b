"""The first-hit query under pt_first_hit_set_ray(PT_RAY_PINHOLE) (csrc/pt_first_hit.hip: pt_first_hit_pinhole_kernel) on the cases of
tests/first_hit_cases.py: the origin is InvView's translation column, the direction goes through the pixel's centre, neither the frame
nor the lens enters, id and t are the oracle's RayTrace on the record's own ray, picking / tiling / group handles agree, switching back
returns the records of sample 0, and pt_render does not notice."""
import ctypes as C
import dataclasses
from importlib import import_module

import numpy as np
import pytest

import first_hit_cases as fh
import test_gpu_first_hit as base

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
_bits = base._bits

_records = {}


def pinhole_records(case, frame=None):
    """The GPU's (H, W) pinhole records of a case (at the case's own frame unless one is given), computed once and left unchanged."""
    frame = case.frame if frame is None else frame
    key = (case, frame)
    if key not in _records:
        pt = fh.make_tracer(case)
        pt.SetFirstHitRay(N.PT_RAY_PINHOLE)
        rec = pt.FirstHit(frame)
        pt.Dispose()
        rec.setflags(write=False)
        _records[key] = rec
    return _records[key]


# ------------------------------------------------------------------------------------------------ 1. the ray
@pytest.mark.parametrize("case", fh.CASES, ids=lambda c: c.name)
def test_origin_is_the_inverse_views_translation_column(case):
    rec = pinhole_records(case)
    column = np.frombuffer(fh.inputs(case)[3], np.float32)[28:31]
    assert rec.shape == (case.height, case.width)
    assert (_bits(rec["origin"]) == _bits(column)).all()
    if case.aperture == 0.0:  # ... which is the origin sample 0 has without a lens
        assert (_bits(base.gpu_records(case)["origin"]) == _bits(rec["origin"])).all()


@pytest.mark.parametrize("case", [c for c in fh.CASES if c.name in ("default_75x43_f0", "default_75x43_ap0", "default_75x43_ap2", "default_1x1",
                                                                   "incuboid_64x36", "default_64x36_ap0_cam2")], ids=lambda c: c.name)
def test_direction_goes_through_the_pixel_centre(case):
    """The float64 camera model of test_pinhole_origin_and_frustum_cell (tests/test_gpu_first_hit.py): every direction is within 1e-5
    rad — that test's slack for the fp32 matrix products — of the model's ray through (x + 0.5, y + 0.5), has unit length, and the
    sub-pixel offsets recovered from it are 0.5.  A pixel of these images spans at least 0.012 rad (45 degrees over at most 43 rows,
    times cos^2 of the off-axis angle at a corner, >= 0.67), so 1e-5 rad is less than 1e-3 of a pixel: the offsets span less than
    0.01, where sample 0's span more than 0.5."""
    rec = pinhole_records(case)
    inv_proj, inv_view, _ = base._camera(fh.inputs(case)[3])
    H, W = rec.shape
    d = rec["dir"].astype(np.float64)
    length = np.abs(np.sqrt((d * d).sum(-1)) - 1.0)
    assert length.max() <= 4 * base.ULP1
    A, bvec = inv_proj[:2, :2], -inv_proj[:2, 2]
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    ndc_c = np.stack([(px + 0.5) / W * 2.0 - 1.0, (py + 0.5) / H * 2.0 - 1.0], -1)
    eye_c = ndc_c @ A.T + bvec
    wd = np.concatenate([eye_c, -np.ones((H, W, 1))], -1) @ inv_view[:3, :3].T
    wd /= np.linalg.norm(wd, axis=-1, keepdims=True)
    cross = np.linalg.norm(np.cross(wd, d), axis=-1) / np.linalg.norm(d, axis=-1)
    angle = np.arcsin(np.clip(cross, 0.0, 1.0))  # (arccos of a dot product loses half the digits near 0)
    cam = np.linalg.solve(inv_view[:3, :3], d.reshape(-1, 3).T).T.reshape(H, W, 3)
    eye = cam[..., :2] / -cam[..., 2:3]
    ndc = np.linalg.solve(A, (eye - bvec).reshape(-1, 2).T).T.reshape(H, W, 2)
    ox, oy = (ndc[..., 0] + 1.0) * 0.5 * W - px, (ndc[..., 1] + 1.0) * 0.5 * H - py
    print(f"{case.name}: directions within {angle.max():.3g} rad of the pixel centre's; sub-pixel offsets x [{ox.min():.5f}, {ox.max():.5f}] y [{oy.min():.5f}, {oy.max():.5f}]")
    assert angle.max() <= 1e-5
    assert (d * wd).sum(-1).min() > 0
    if case.width > 1:
        for o in (ox, oy):
            assert np.abs(o - 0.5).max() < 0.005 and o.max() - o.min() < 0.01


def test_neither_the_frame_nor_the_lens_enters():
    case = fh.BY_NAME["default_75x43_f0"]
    rec = pinhole_records(case, 0)
    assert pinhole_records(case, 7).tobytes() == rec.tobytes()
    for focal, aperture in ((5.0, 2.0), (0.0, 0.0), (20.0, 0.0)):  # (focal length 0: the ray is defined there too)
        other = dataclasses.replace(case, name=f"{case.name}_F{focal}_A{aperture}", focal_length=focal, aperture=aperture)
        assert pinhole_records(other, 3).tobytes() == rec.tobytes(), (focal, aperture)
    sample0 = base.gpu_records(case)
    assert sample0.tobytes() != rec.tobytes()  # (and it is not sample 0's record)
    assert (rec["id"] != sample0["id"]).any() or (_bits(rec["dir"]) != _bits(sample0["dir"])).any()


# ------------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("case", [c for c in fh.CASES if c.scene != "empty"], ids=lambda c: c.name)
def test_id_and_t_are_the_oracles_ray_trace_of_the_records_own_ray(oracle, case):
    """As test_t_is_the_oracles_root_bit_for_bit: the record's (origin, dir) and the winner's geometry through the oracle's ray_sphere /
    ray_cuboid give t as uint32 on every hit pixel; on REPLAY_CASES the whole of RayTrace is re-run in visiting order: winner and T
    come out the same, misses included."""
    blob, ns, nc, _ = fh.inputs(case)
    rp = fh.Replayer(oracle, blob, ns, nc)
    rec = pinhole_records(case)
    miss = rec["id"] < 0
    assert np.isposinf(rec["t"][miss]).all() and np.isfinite(rec["t"][~miss]).all() and (rec["t"][~miss] > 0).all()
    assert (~miss).any()
    bad = []
    for y, x in np.argwhere(~miss):
        r = rec[y, x]
        rp.set_ray(r["origin"], r["dir"])
        hit, t1, t2 = rp.leaf(int(r["id"]))
        root = t2 if t1 < 0.0 else t1
        if not (hit and t2 > 0.0 and _bits(np.float32(root)) == _bits(r["t"])):
            bad.append((int(y), int(x), int(r["id"]), float(root), float(r["t"])))
    assert not bad, f"{case.name}: {len(bad)} roots differ, e.g. (y, x, id, oracle, gpu) = {bad[:3]}"
    if case.name in fh.REPLAY_CASES:
        for y in range(case.height):
            for x in range(case.width):
                r = rec[y, x]
                rp.set_ray(r["origin"], r["dir"])
                winner, T = rp.trace()
                assert winner == int(r["id"]), (case.name, y, x, winner, int(r["id"]))
                if winner >= 0:
                    assert _bits(np.float32(T)) == _bits(r["t"]), (case.name, y, x)


def test_an_empty_scene_misses_everywhere():
    rec = pinhole_records(fh.BY_NAME["empty_16x9"])
    assert (rec["id"] == -1).all() and np.isposinf(rec["t"]).all()


# ------------------------------------------------------------------------------------------------ 3. picking, tiling, groups, switching back
def test_pick_tiles_and_switching_back():
    case = fh.BY_NAME["default_75x43_f1"]  # aperture 0.14
    whole, sample0 = pinhole_records(case), base.gpu_records(case)
    pt = fh.make_tracer(case)
    before = pt.FirstHit(case.frame)
    assert before.tobytes() == sample0.tobytes()
    pt.SetFirstHitRay(N.PT_RAY_PINHOLE)
    rec = pt.FirstHit(case.frame)
    assert rec.tobytes() == whole.tobytes()
    base._picks_equal_records(pt, rec, {y: y for y in range(43)}, case, 1, list(range(43)))
    pt.SetTile(8, 16)
    rec = pt.FirstHit(case.frame)
    assert rec.shape == (16, 75) and rec.tobytes() == whole[8:24].tobytes()
    base._picks_equal_records(pt, rec, {y: y - 8 for y in range(8, 24)}, case, 2, list(range(8, 24)))
    pt.SetInterleavedTile(1, 3, 8)
    rows = import_module(pkg.__name__ + ".distributed").interleaved_rows(43, 1, 3, 8)
    rec = pt.FirstHit(case.frame)
    assert rec.shape == (len(rows), 75) and rec.tobytes() == whole[rows].tobytes()
    base._picks_equal_records(pt, rec, {y: k for k, y in enumerate(rows)}, case, 3, rows)
    # the mode survives the re-tilings; back to sample 0: the earlier records, bit for bit
    pt.SetFirstHitRay(N.PT_RAY_SAMPLE0)
    assert pt.FirstHit(case.frame).tobytes() == sample0[rows].tobytes()
    pt.SetTile(0, 43)
    rec = pt.FirstHit(case.frame)
    assert rec.tobytes() == sample0.tobytes()
    base._picks_equal_records(pt, rec, {y: y for y in range(43)}, case, 4, list(range(43)))
    pt.Dispose()


def test_group_handle_returns_the_single_handle_buffer():
    case = fh.BY_NAME["default_75x43_f1"]
    whole = pinhole_records(case)
    for band in (8, 0):
        pt = fh.make_tracer(case, devices=[0, 0])
        if band == 0:
            pt.SetPartition(0)
        pt.SetFirstHitRay(N.PT_RAY_PINHOLE)  # fans out to both parts
        rec = pt.FirstHit(case.frame)
        assert rec.tobytes() == whole.tobytes(), f"band_rows {band}"
        base._picks_equal_records(pt, rec, {y: y for y in range(43)}, case, 5 + band, list(range(43)))
        pt.SetFirstHitRay(N.PT_RAY_SAMPLE0)
        assert pt.FirstHit(case.frame).tobytes() == base.gpu_records(case).tobytes()
        pt.Dispose()


def test_render_does_not_notice_the_pinhole_query():
    case = fh.BY_NAME["default_75x43_f0"]
    env = pkg.envmap.synthetic_sky_rgba32f(32)

    def run(with_query):
        pt = fh.make_tracer(case, env=env, ray_depth=8)
        pt.SetFirstHitRay(N.PT_RAY_PINHOLE)
        for f in range(8):
            pt.Render()
            if with_query and f < 7:
                N.check(pt._lib.pt_first_hit_render(pt._h, f), pt._h)
                pt.Pick(10 + f, 20, f)
        img, frames = pt.Result.copy(), pt.FrameIndex
        pt.Dispose()
        return img, frames
    plain, with_q = run(False), run(True)
    assert plain[1] == with_q[1] == 8
    assert (_bits(plain[0]) == _bits(with_q[0])).all()
    assert np.isfinite(plain[0]).all() and plain[0][..., :3].max() > 0


# ------------------------------------------------------------------------------------------------ 4. error codes
def test_error_codes():
    case = fh.BY_NAME["default_75x43_f0"]
    whole, sample0 = pinhole_records(case), base.gpu_records(case)
    pt = fh.make_tracer(case)
    L, h = pt._lib, pt._h
    i = C.c_int()
    assert L.pt_first_hit_set_ray(None, N.PT_RAY_PINHOLE) == N.PT_E_BAD_HANDLE
    for bad in (-1, 2, 1 << 20):
        assert L.pt_first_hit_set_ray(h, bad) == N.PT_E_BAD_ARGUMENT, bad
    assert pt.FirstHit(0).tobytes() == sample0.tobytes()       # the default is still in force
    assert L.pt_first_hit_set_ray(h, N.PT_RAY_PINHOLE) == N.PT_OK
    for bad in (-1, 2):
        assert L.pt_first_hit_set_ray(h, bad) == N.PT_E_BAD_ARGUMENT, bad
    assert pt.FirstHit(0).tobytes() == whole.tobytes()         # ... and now the pinhole ray is
    assert L.pt_first_hit_render(h, -1) == N.PT_E_BAD_ARGUMENT  # frame_index is still validated
    assert L.pt_pick(h, 0, 0, -1, C.byref(i), None, None, None) == N.PT_E_BAD_ARGUMENT
    assert L.pt_pick(h, 75, 0, 0, C.byref(i), None, None, None) == N.PT_E_OUT_OF_RANGE
    assert L.pt_pick(h, 74, 42, 5, C.byref(i), None, None, None) == N.PT_OK and i.value == int(whole[42, 74]["id"])
    pt.Dispose()
    g = fh.make_tracer(case, devices=[0, 0])
    assert g._lib.pt_first_hit_set_ray(g._h, 2) == N.PT_E_BAD_ARGUMENT
    assert g.FirstHit(0).tobytes() == sample0.tobytes()
    g.Dispose()
