"""The first-hit query on the GPU (pt_first_hit_render / pt_first_hit_read / pt_pick, csrc/pt_first_hit.hip) against the frozen oracle:
ids equal the oracle's own first-hit decode on every pixel (tests/first_hit_cases.py; soundness: tests/test_first_hit_abi.py), t is
the oracle's root bit for bit, the ray is the integrator's, tiling / picking / group handles agree, and pt_render does not notice."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
ULP1 = 2.0 ** -23  # spacing of binary32 at 1.0

_records = {}


def gpu_records(case):
    """The GPU's (H, W) records of a case, computed once and left unchanged."""
    if case.name not in _records:
        pt = fh.make_tracer(case)
        rec = pt.FirstHit(case.frame)
        pt.Dispose()
        rec.setflags(write=False)
        _records[case.name] = rec
    return _records[case.name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. ids
@pytest.mark.parametrize("case", fh.CASES, ids=lambda c: c.name)
def test_id_equals_the_oracle_decode_on_every_pixel(oracle, case):
    want, _ = fh.oracle_first_hit(oracle, case)
    rec = gpu_records(case)
    assert rec.shape == (case.height, case.width)
    diff = rec["id"] != want
    assert not diff.any(), f"{case.name}: {int(diff.sum())} of {diff.size} ids differ, first at (y, x) = {np.argwhere(diff)[:4].tolist()}"
    miss = rec["id"] < 0
    assert np.isposinf(rec["t"][miss]).all() and np.isfinite(rec["t"][~miss]).all() and (rec["t"][~miss] > 0).all()
    if case.scene == "empty":
        assert miss.all()


# ------------------------------------------------------------------------------------------------ 2. t
@pytest.mark.parametrize("case", [c for c in fh.CASES if c.scene != "empty"], ids=lambda c: c.name)
def test_t_is_the_oracles_root_bit_for_bit(oracle, case):
    """The GPU's own (origin, dir) and the winner's geometry through the oracle's ray_sphere / ray_cuboid: the root RayTrace keeps
    (t1 < 0 ? t2 : t1, compute.glsl:347-350) equals t as uint32.  On REPLAY_CASES the whole of RayTrace is re-run in visiting order with
    that ray: no other object is accepted instead, i.e. winner and T come out the same."""
    blob, ns, nc, _ = fh.inputs(case)
    rp = fh.Replayer(oracle, blob, ns, nc)
    rec = gpu_records(case)
    replay = case.name in fh.REPLAY_CASES
    bad = []
    for y, x in np.argwhere(rec["id"] >= 0):
        r = rec[y, x]
        rp.set_ray(r["origin"], r["dir"])
        hit, t1, t2 = rp.leaf(int(r["id"]))
        root = t2 if t1 < 0.0 else t1
        if not (hit and t2 > 0.0 and _bits(np.float32(root)) == _bits(r["t"])):
            bad.append((int(y), int(x), int(r["id"]), float(root), float(r["t"])))
    assert not bad, f"{case.name}: {len(bad)} roots differ, e.g. (y, x, id, oracle, gpu) = {bad[:3]}"
    if replay:
        for y in range(case.height):
            for x in range(case.width):
                r = rec[y, x]
                rp.set_ray(r["origin"], r["dir"])
                winner, T = rp.trace()
                assert winner == int(r["id"]), (case.name, y, x, winner, int(r["id"]))
                if winner >= 0:
                    assert _bits(np.float32(T)) == _bits(r["t"]), (case.name, y, x)


# ------------------------------------------------------------------------------------------------ 3. the ray
@pytest.mark.parametrize("case", fh.CASES, ids=lambda c: c.name)
def test_directions_have_unit_length(case):
    d = gpu_records(case)["dir"].astype(np.float64)
    err = np.abs(np.sqrt((d * d).sum(-1)) - 1.0)
    print(f"{case.name}: | |dir| - 1 | up to {err.max() / ULP1:.2f} ulp")
    assert err.max() <= 4 * ULP1


def _camera(basic):
    b = np.frombuffer(basic, np.float32).astype(np.float64)
    inv_proj, inv_view = b[0:16].reshape(4, 4).T, b[16:32].reshape(4, 4).T  # GLSL column-major view: M[r][c] = m[4 c + r]
    return inv_proj, inv_view, np.frombuffer(basic, np.float32)[32:35]


@pytest.mark.parametrize("name", ["default_75x43_ap0", "default_64x36_ap0_cam2"])
def test_pinhole_origin_and_frustum_cell(name):
    """Aperture 0: the origin is InvView * (0, 0, 0, 1) (compute.glsl:120), i.e. InvView's translation column, bit for bit — which is
    ViewPos bit for bit for the camera whose blob holds the same bits in both places (cam2; the default camera's inverse is one ulp off
    in z, as the host computes it) — and every direction lies in its pixel's frustum cell: float64 camera model, sub-pixel offset in
    [0, 1), 1e-5 rad of slack for the fp32 matrix products (per-component error of a few 2^-24 of unit-scale terms)."""
    case = fh.BY_NAME[name]
    rec = gpu_records(case)
    basic = fh.inputs(case)[3]
    inv_proj, inv_view, view_pos = _camera(basic)
    column = np.frombuffer(basic, np.float32)[28:31]
    assert (_bits(rec["origin"]) == _bits(column)).all()
    if name.endswith("cam2"):
        assert (_bits(column) == _bits(view_pos)).all()  # (the premise; also pinned on the CPU)
        assert (_bits(rec["origin"]) == _bits(view_pos)).all()
    H, W = rec.shape
    d = rec["dir"].astype(np.float64)
    cam = np.linalg.solve(inv_view[:3, :3], d.reshape(-1, 3).T).T.reshape(H, W, 3)
    eye = cam[..., :2] / -cam[..., 2:3]      # scaled so that z = -1, as GetWorldSpaceRay builds it (compute.glsl:352-357)
    A, bvec = inv_proj[:2, :2], -inv_proj[:2, 2]  # eye.xy = A ndc + b for the clip-space point (ndc, -1, 0)
    ndc = np.linalg.solve(A, (eye - bvec).reshape(-1, 2).T).T.reshape(H, W, 2)
    fx, fy = (ndc[..., 0] + 1.0) * 0.5 * W, (ndc[..., 1] + 1.0) * 0.5 * H
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    cx, cy = np.clip(fx, px, px + 1.0), np.clip(fy, py, py + 1.0)  # the nearest point of the pixel's cell
    ndc_c = np.stack([cx / W * 2.0 - 1.0, cy / H * 2.0 - 1.0], -1)
    eye_c = ndc_c @ A.T + bvec
    wd = np.concatenate([eye_c, -np.ones((H, W, 1))], -1) @ inv_view[:3, :3].T
    wd /= np.linalg.norm(wd, axis=-1, keepdims=True)
    angle = np.arccos(np.clip((wd * d).sum(-1) / np.linalg.norm(d, axis=-1), -1.0, 1.0))
    print(f"{name}: directions leave their cell by at most {angle.max():.3g} rad; sub-pixel offsets span [{(fx - px).min():.3f}, {(fx - px).max():.3f}]")
    assert angle.max() <= 1e-5
    assert (fx - px).max() - (fx - px).min() > 0.5  # the sub-pixel draws are in: offsets spread over the cell


# ------------------------------------------------------------------------------------------------ 4. tiling, picking, groups
def _picks_equal_records(pt, rec, row_of, case, seed, rows):
    rng = np.random.default_rng(seed)
    for _ in range(32):
        x, y = int(rng.integers(case.width)), int(rows[int(rng.integers(len(rows)))])
        i, t, o, d = pt.Pick(x, y, case.frame)
        r = rec[row_of[y], x]
        assert i == int(r["id"]) and _bits(np.float32(t)) == _bits(r["t"]), (x, y)
        assert (_bits(o) == _bits(r["origin"])).all() and (_bits(d) == _bits(r["dir"])).all(), (x, y)


def test_pick_equals_the_record_untiled_tiled_and_interleaved():
    case = fh.BY_NAME["default_75x43_f1"]
    whole = gpu_records(case)
    pt = fh.make_tracer(case)
    rec = pt.FirstHit(case.frame)
    assert rec.tobytes() == whole.tobytes()
    _picks_equal_records(pt, rec, {y: y for y in range(43)}, case, 1, list(range(43)))
    pt.SetTile(8, 16)  # rows 8-23 of 43
    rec = pt.FirstHit(case.frame)
    assert rec.shape == (16, 75) and rec.tobytes() == whole[8:24].tobytes()
    _picks_equal_records(pt, rec, {y: y - 8 for y in range(8, 24)}, case, 2, list(range(8, 24)))
    pt.SetInterleavedTile(1, 3, 8)
    rows = import_module(pkg.__name__ + ".distributed").interleaved_rows(43, 1, 3, 8)
    assert rows == list(range(8, 16)) + list(range(32, 40))
    rec = pt.FirstHit(case.frame)
    assert rec.shape == (len(rows), 75) and rec.tobytes() == whole[rows].tobytes()
    _picks_equal_records(pt, rec, {y: k for k, y in enumerate(rows)}, case, 3, rows)
    pt.Dispose()


def test_group_handle_returns_the_single_handle_buffer():
    case = fh.BY_NAME["default_75x43_f1"]
    whole = gpu_records(case)
    for band in (8, 0):  # block-cyclic bands (gathered through the band assembly) and contiguous row blocks
        pt = fh.make_tracer(case, devices=[0, 0])
        if band == 0:
            pt.SetPartition(0)
        rec = pt.FirstHit(case.frame)
        assert rec.tobytes() == whole.tobytes(), f"band_rows {band}"
        _picks_equal_records(pt, rec, {y: y for y in range(43)}, case, 4 + band, list(range(43)))
        pt.Dispose()


# ------------------------------------------------------------------------------------------------ 5. non-interference
@pytest.mark.parametrize("name, batch1", [("default_8x8", False), ("default_75x43_f0", False), ("default_75x43_f0", True)])
def test_render_does_not_notice_the_query(name, batch1):
    case = fh.BY_NAME[name]
    env = pkg.envmap.synthetic_sky_rgba32f(32)

    def run(with_query):
        pt = fh.make_tracer(case, env=env, ray_depth=8)
        if batch1:
            pt.SetFrameBatch(1)
        for f in range(8):
            pt.Render()
            if with_query and f < 7:
                N.check(pt._lib.pt_first_hit_render(pt._h, f), pt._h)
        img, frames = pt.Result.copy(), pt.FrameIndex
        pt.Dispose()
        return img, frames
    plain, with_q = run(False), run(True)
    assert plain[1] == with_q[1] == 8
    assert (_bits(plain[0]) == _bits(with_q[0])).all()
    assert np.isfinite(plain[0]).all() and plain[0][..., :3].max() > 0


# ------------------------------------------------------------------------------------------------ 6. error codes
def test_error_codes():
    case = fh.BY_NAME["default_75x43_f0"]
    pt = fh.make_tracer(case)  # (no environment: the query needs none)
    L, h = pt._lib, pt._h
    buf = np.empty((43, 75), pkg.path_tracer.FIRST_HIT_DTYPE)
    p = buf.ctypes.data_as(C.c_void_p)
    i, t = C.c_int(), C.c_float()
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert L.pt_first_hit_read(h, p, 0) == N.PT_E_BAD_ARGUMENT          # nothing rendered yet
    assert L.pt_first_hit_device_ptr(h, C.byref(ptr), C.byref(nbytes)) == N.PT_E_BAD_ARGUMENT
    assert L.pt_first_hit_render(h, -1) == N.PT_E_BAD_ARGUMENT
    assert L.pt_first_hit_render(h, 0) == N.PT_OK
    assert L.pt_first_hit_read(h, None, 0) == N.PT_E_BAD_ARGUMENT
    assert L.pt_first_hit_read(h, p, 75 * 32 - 1) == N.PT_E_BAD_ARGUMENT  # pitch smaller than a row
    assert L.pt_first_hit_read(h, p, 0) == N.PT_OK
    assert L.pt_first_hit_device_ptr(h, C.byref(ptr), C.byref(nbytes)) == N.PT_OK and ptr.value and nbytes.value == 43 * 75 * 32
    assert L.pt_pick(h, 0, 0, 0, None, C.byref(t), None, None) == N.PT_E_BAD_ARGUMENT
    assert L.pt_pick(h, 0, 0, -1, C.byref(i), None, None, None) == N.PT_E_BAD_ARGUMENT
    for x, y in [(-1, 0), (75, 0), (0, -1), (0, 43)]:
        assert L.pt_pick(h, x, y, 0, C.byref(i), None, None, None) == N.PT_E_OUT_OF_RANGE
    assert L.pt_pick(h, 74, 42, 0, C.byref(i), None, None, None) == N.PT_OK  # every out-pointer but out_id may be NULL
    for resize in (lambda: pt.SetTile(8, 16), lambda: pt.SetInterleavedTile(1, 3, 8), lambda: pt.SetSize(75, 43)):
        assert L.pt_first_hit_render(h, 0) == N.PT_OK and L.pt_first_hit_read(h, p, 0) == N.PT_OK
        resize()
        assert L.pt_first_hit_read(h, p, 0) == N.PT_E_BAD_ARGUMENT      # the records went with the old size / tiling
    pt.SetTile(8, 16)
    assert L.pt_pick(h, 0, 7, 0, C.byref(i), None, None, None) == N.PT_E_OUT_OF_RANGE   # rows the handle does not own
    assert L.pt_pick(h, 0, 24, 0, C.byref(i), None, None, None) == N.PT_E_OUT_OF_RANGE
    assert L.pt_pick(h, 0, 8, 0, C.byref(i), None, None, None) == N.PT_OK
    pt.SetInterleavedTile(1, 3, 8)
    assert L.pt_pick(h, 0, 16, 0, C.byref(i), None, None, None) == N.PT_E_OUT_OF_RANGE
    assert L.pt_pick(h, 0, 32, 0, C.byref(i), None, None, None) == N.PT_OK
    pt.Dispose()
    g = fh.make_tracer(case, devices=[0, 0])
    assert g._lib.pt_first_hit_device_ptr(g._h, C.byref(ptr), C.byref(nbytes)) == N.PT_E_BAD_ARGUMENT  # single-GPU handles only
    assert g._lib.pt_first_hit_read(g._h, p, 0) == N.PT_E_BAD_ARGUMENT
    assert g._lib.pt_pick(g._h, 0, 43, 0, C.byref(i), None, None, None) == N.PT_E_OUT_OF_RANGE
    g.Dispose()


# ------------------------------------------------------------------------------------------------ 7. cost (recorded, not gated)
def test_cost_is_recorded(oracle, parity_report):
    """One 1080p pt_first_hit_render against one depth-1 frame of variant 1 (the same shape of kernel: one wavefront per tile), same scene,
    same handle, pt_timer_*, fastest of three.  The query runs a strict subset of that frame's work.  The times are recorded, not gated:
    they go into the terminal summary as the labels of two parity rows (tests/conftest.py's table), whose figures are the share of the
    1080p image's ids that equal the oracle's decode (all of them: 32,400 tiles, every XCD band)."""
    case = fh.Case("default_1080p", "default", 1920, 1080)
    pt = fh.make_tracer(case, env=pkg.envmap.synthetic_sky_rgba32f(32), ray_depth=1)
    pt.SetVariant(1)
    pt.Render()
    N.check(pt._lib.pt_first_hit_render(pt._h, 0), pt._h)  # (both warmed up: buffers allocated, code loaded)
    pt.Synchronize()
    query, frame = [], []
    for k in range(3):
        pt.TimerBegin()
        N.check(pt._lib.pt_first_hit_render(pt._h, k), pt._h)
        query.append(pt.TimerEnd())
        pt.TimerBegin()
        pt.Render()
        frame.append(pt.TimerEnd())
    rec = pt.FirstHit(case.frame)
    pt.Dispose()
    same = float((rec["id"] == fh.oracle_first_hit(oracle, case)[0]).mean())
    lines = [f"first hit 1080p: pt_first_hit_render {min(query):.4f} ms",
             f"first hit 1080p: pt_render variant 1 depth 1 {min(frame):.4f} ms"]
    print("\n  " + "\n  ".join(lines) + f"\n  (runs: query {query}, frame {frame})")
    for line in lines:
        parity_report(line, {"within": same, "bit_identical": same, "mean_rel_err": 0.0, "mean_abs_err": 0.0}, 1.0)
    assert same == 1.0
    assert min(query) > 0 and min(frame) > 0
