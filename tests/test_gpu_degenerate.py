"""The HIP path on the degenerate and extreme scenes of tests/degenerate_cases.py against the frozen oracle: hit acceptance, the
tile-pass culling and its cached masks, the sphere runs, the grid walk, cuboid normals, Fresnel / refraction / Beer's law with
unclamped materials, and non-finite values in every field.  What each case is aimed at is proved on the CPU first
(tests/test_degenerate_cpu.py).  Images are compared with dc.same_colour: RGB words equal as uint32 or both NaN, alpha equal as
uint32.  The sign and payload of a NaN are not part of the contract: which payload an operation on two NaNs keeps, and what an
accumulation carries over many frames, may differ between the two machines.  (Measured: generated NaNs were 0xFFC00000 on the MI355X
as on x86, propagated ones 0x7FC00000; one pixel of one 40-frame case differed in its NaN word.)  How many pixels of a case match only
as NaN == NaN is printed, not asserted (docs/parity.md has the figures).  Run with `pytest -m gpu` on an MI355X; the
ids carry the tier (`-k tierF`, `-k tierN`).

Termination (read before the first run; nothing here is meant to fault or hang a card).  The bounce loop is bounded by rayDepth, the
Newton sequences of the primitives have a fixed length, and the hand-over protocol reads alpha tags, never colours — alpha is exactly
1 in every case (test_degenerate_cpu.py).  The one loop whose trip count depends on scene data is the grid walk of ray_trace_t<GRID>
(csrc/pt_device.hpp) together with its caller: a walk cut short after PT_WALK_ROUNDS = 6 cells returns walkFrom = the exit parameter
`texit` of the last cell it processed, and the caller traces the same ray again from there.  Why that always makes progress, for every
grid ptgrid::build can return on the F6 and tier-N blobs (zero radii, every centre in one plane; radii of 1e19 and non-finite spheres
are refused, `Rg < 1e15` and the isfinite test — asserted in tests/test_sphere_grid_host.py on exactly these blobs):
  1. Within one call the walk is a loop over `round` that either breaks or steps one cell along one axis and decrements that axis's
     count of cells left (rx, ry, rz >= 0; `more` is false at 0 and ends the walk).  So a call ends after at most 6 rounds, and a walk
     as a whole crosses at most nx + ny + nz <= 96 cell faces.
  2. A lane only walks when its direction has unit length to 1e-5 and its origin is within gridReach of the box, so the clamped
     reciprocals are at least 0.99999 in magnitude and finite (|d| <= 1e-18 is replaced by 1e18), and the per-cell increments
     dx = |cell * rcp(d.x)| etc. are positive and finite; m + dm > m holds because m / dm is at most the number of cells between the
     origin and the far face, a few hundred, far below 2^24.  The exit parameter of successive rounds therefore never decreases, and
     it can stay equal for at most three rounds in a row (a ray through a cell corner steps x, y and z at the same parameter).  Hence
     the texit of round 5 exceeds the texit of round 0 by at least one whole increment, >= 0.99999 times the smallest cell extent.
  3. The resumed call enters at p = fma(d, max(tn, walkFrom), o) and recomputes its cell from p.  p lies within delta of the face the
     last call stopped at, delta <= 4 * 2^-23 * D + 2^-24 * (M + D) (the error of texit — two roundings and a 1-ulp reciprocal — times
     a length of at most D = reach + the box's diagonal, plus the rounding of the fused multiply-add at coordinate magnitude M + D).
     test_sphere_grid_host.py asserts that every cell of every grid of the table is at least 16 delta wide (measured: 9,000 to
     110,000 delta, the thinnest being 64 zero-radius spheres in one plane, whose box is the sqrt(2 err) margin plus the walk slack
     on either side).  So along the axis of the last step p falls into the cell the last call stopped in or into the next one, never
     further back; in the first case round 0 repeats that cell with texit equal to walkFrom up to a few ulps, and by 2. round 5 ends
     a whole cell increment later: the new walkFrom exceeds the old one by at least 15 delta > 0.  The same holds for the two lateral
     axes: where the ray crossed one of their faces within delta of texit (an exit near a cell edge or corner), p may lie one cell
     back on that axis as well — at most one cell on each of the three axes, so at most 3 of the resumed call's rounds repeat cells
     and each ends at a texit within a few ulps of walkFrom, while the call takes 6: at least 3 rounds go forward, and the bound of
     2. on texit (a whole increment over any 4 consecutive rounds) still gives a new walkFrom above the old one.
  4. walkFrom strictly increases from call to call by at least 15/16 of the smallest cell increment while tn <= tf, and tf is finite
     (the box is finite): after finitely many calls `more` is false or tn > tf, and the walk ends.  A lane whose walk sets `viol`
     (an inside sphere after the first cell) or that is not covered (NaN anywhere in o or d: both comparisons of needBrute fail) takes
     the in-order loop, which is bounded by numSpheres.
A flat grid (every centre in one plane) has one layer of cells on the thin axis; rz is 0 there, so a step along z ends the walk at once.
"""
import numpy as np
import pytest

import degenerate_cases as dc
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = dc.pkg
N = pkg.native

ids = lambda c: f"tier{c.tier}-{c.name}"  # noqa: E731
CASES = dc.CASES
FIRST_HIT = [c for c in CASES if c.first_hit]
SMALL = dc.BY_NAME["f1_huge_inside_1e20"]      # the 8 x 8 case of tier F
SMALL_N = dc.BY_NAME["n_mat_b"]                # ... and of tier N (22 % NaN pixels)
MORE_VARIANTS = [SMALL, SMALL_N, dc.BY_NAME["f6_f3_200"]]
SPP3 = [dc.BY_NAME["f3_spheres"], dc.BY_NAME["f4_room_1e4"], dc.BY_NAME["f5_ior"], dc.BY_NAME["n_mat_a"]]
LONG = [SMALL, dc.BY_NAME["f5_absorbance"], SMALL_N]
GROUP = [dc.BY_NAME["f3_spheres"], dc.BY_NAME["n_mat_a"]]
assert SMALL.width == SMALL.height == 8 and SMALL_N.width == SMALL_N.height == 8


def tracer(case, blob, ns, nc, spp=None, aperture=None, **extra):
    """A PathTracer with the given blob as the case's scene (uploaded as bytes: nothing clamps or converts them)."""
    pt = pkg.PathTracer(dc.env(case), case.width, case.height, case.depth, case.spp if spp is None else spp, case.focal_length,
                        case.aperture if aperture is None else aperture, **extra)
    objs = np.frombuffer(blob, dtype=np.uint8)
    pt.GameObjectsUBO.SubData(0, objs.nbytes, objs)
    pt._numSpheres, pt._numCuboids = ns, nc
    pt._push_params()
    pt.UploadBasicData(dc.basic(case))
    return pt


_images = {}


def gpu_image(case, variant=0):
    """dc.FRAMES frames of the case through pt_render, computed once per (case, variant) and left unchanged"""
    key = (case.name, variant)
    if key not in _images:
        b = dc.built(case)
        pt = tracer(case, b.blob, b.ns, b.nc)
        try:
            pt.SetVariant(variant)
            for _ in range(dc.FRAMES):
                pt.Render()
            img = pt.Result.copy()
        finally:
            pt.Dispose()
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def nan_words(img):
    rgb = np.asarray(img)[..., :3]
    return sorted({hex(int(v)) for v in dc.words(rgb)[np.isnan(rgb)]})[:6]


def assert_same_colour(got, want, what):
    ok = dc.same_colour(got, want)
    only_nan = int(dc.nan_only(got, want).sum())
    print(f"{what}: {only_nan} of {ok.size} pixels match only as NaN == NaN; NaN words GPU {nan_words(got)}, oracle {nan_words(want)}")
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} pixels differ from the oracle, first at (y, x) = {np.argwhere(~ok)[:4].tolist()}"


# ------------------------------------------------------------------------------------------------ accumulation
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_accumulation_equals_the_oracle(oracle, case, variant):
    assert_same_colour(gpu_image(case, variant), dc.oracle_image(oracle, case), f"{case.name}, variant {variant}")


@pytest.mark.parametrize("variant", [2, 6, 12])
@pytest.mark.parametrize("case", MORE_VARIANTS, ids=ids)
def test_other_kernel_variants(oracle, case, variant):
    assert_same_colour(gpu_image(case, variant), dc.oracle_image(oracle, case), f"{case.name}, variant {variant}")


@pytest.mark.parametrize("batch_pass", [False, True], ids=["in_lane", "batch_pass"])
@pytest.mark.parametrize("case", SPP3, ids=ids)
def test_three_samples_per_pixel(oracle, case, batch_pass):
    """spp 3: the persistent kernel's in-lane sample chain, and — small images only reach it with the knob batch_pass_min_tiles = 0 — the
    multisample kernel"""
    b = dc.built(case)
    want = dc.oracle_image(oracle, case, spp=3)
    if batch_pass:
        N.debug_set("batch_pass_min_tiles", 0)
    try:
        pt = tracer(case, b.blob, b.ns, b.nc, spp=3)
        try:
            for _ in range(dc.FRAMES):
                pt.Render()
            got = pt.Result.copy()
        finally:
            pt.Dispose()
    finally:
        if batch_pass:
            N.debug_set("batch_pass_min_tiles", 16384)
    assert_same_colour(got, want, f"{case.name}, spp 3{', batch pass' if batch_pass else ''}")


@pytest.mark.parametrize("case", LONG, ids=ids)
def test_forty_frames_in_chained_launches(oracle, case):
    """40 frames with pt_set_frame_batch(16): tagged launches of several frames each, chained on the alpha tags — which no NaN colour may
    disturb"""
    b = dc.built(case)
    pt = tracer(case, b.blob, b.ns, b.nc)
    try:
        pt.SetFrameBatch(16)
        for _ in range(40):
            pt.Render()
        got, frames = pt.Result.copy(), pt.FrameIndex
    finally:
        pt.Dispose()
    assert frames == 40
    assert_same_colour(got, dc.oracle_image(oracle, case, frames=40), f"{case.name}, 40 frames")


# ------------------------------------------------------------------------------------------------ never-hit objects, unused slots
@pytest.mark.parametrize("case", [c for c in CASES if c.still], ids=ids)
def test_still_cases_equal_the_base_scene_strictly(oracle, case):
    """Slots past the counts filled with NaN or -inf words, and objects no ray can hit: word for word the image of the scene with zeros
    in those slots / without those objects — on the oracle (no NaN rule needed: these images hold no NaN) and rendered by the GPU itself"""
    base = dc.built(case).base
    want = dc.oracle_image(oracle, case, "base")
    for variant in (0, 1):
        got = gpu_image(case, variant)
        assert (dc.words(got) == dc.words(want)).all(), f"{case.name}, variant {variant}: differs from the oracle's image of the base scene"
    pt = tracer(case, *base)
    try:
        for _ in range(dc.FRAMES):
            pt.Render()
        plain = pt.Result.copy()
    finally:
        pt.Dispose()
    assert (dc.words(gpu_image(case)) == dc.words(plain)).all(), f"{case.name}: differs from the GPU's own image of the base scene"


# ------------------------------------------------------------------------------------------------ tile masks
def changed_slots(old: bytes, new: bytes):
    """(offset, size) of every object slot of the GameObjectsUBO, used or not, whose bytes differ"""
    a, b = np.frombuffer(old, np.uint8), np.frombuffer(new, np.uint8)
    slots = [(dc.SPHERE_STRIDE * i, dc.SPHERE_STRIDE) for i in range(dc.PT_MAX_SPHERES)]
    slots += [(dc.CUBOID_BASE + dc.CUBOID_STRIDE * j, dc.CUBOID_STRIDE) for j in range(dc.PT_MAX_CUBOIDS)]
    return [(off, n) for off, n in slots if (a[off:off + n] != b[off:off + n]).any()]


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_cached_tile_masks_on_and_after_a_degenerate_edit(oracle, case):
    """Every case with aperture 0.14 on a static camera: five launches of three frames, the later ones with the cached tile masks
    (tile_cone, cone_sphere_masks, cone_cuboid_mask — the only place cuboids are culled at all) — first on the REPAIRED scene (same
    counts: the degenerate objects benign, moved out of the way, or zeros in the unused slots), then, without moving the camera, after
    partial uploads that put the degenerate bytes into their own slots: the masks must be dropped by the edit, rebuilt, and follow it.
    That the masks are in force is read from pt_debug_launch_stats, not assumed."""
    b = dc.built(case)
    blob0, ns, nc = b.repaired or b.base
    assert (ns, nc) == (b.ns, b.nc)
    edits = changed_slots(blob0, b.blob)
    assert edits
    kw = dict(dc.oracle_kwargs(case, ns, nc), aperture=0.14)
    render = lambda blob, frames: oracle.render(case.width, case.height, dc.basic(case), blob, dc.env(case), num_frames=frames, **kw)  # noqa: E731
    stats = lambda: N.debug_launch_stats(pt._h)  # noqa: E731
    pt = tracer(case, blob0, ns, nc, aperture=0.14)
    try:
        for _ in range(5):
            for _ in range(3):
                pt.Render()
            pt.Synchronize()
        s0 = stats()
        assert s0["tile_masks_valid"] and s0["mask_builds"] >= 1, f"{case.name}: no cached masks after 15 frames on a static camera: {s0}"
        assert_same_colour(pt.Result, render(blob0, 15), f"{case.name}, repaired scene, cached masks")
        new = np.frombuffer(b.blob, np.uint8)
        for off, size in edits:
            pt.GameObjectsUBO.SubData(off, size, new[off:off + size].copy())
        assert not stats()["tile_masks_valid"], f"{case.name}: the edit left the cached masks in force"
        pt.ResetRenderer()
        for _ in range(4):
            for _ in range(3):
                pt.Render()
            pt.Synchronize()
        s1 = stats()
        assert s1["tile_masks_valid"] and s1["mask_builds"] > s0["mask_builds"], f"{case.name}: the masks were not rebuilt after the edit: {s1}"
        after = render(b.blob, 12)
        if not case.still:
            assert (~dc.same_colour(after, render(blob0, 12))).mean() >= 0.05, "the edit must be visible"
        assert_same_colour(pt.Result, after, f"{case.name}, after the edit, cached masks")
        # and the static degenerate scene once more, the rebuilt masks in force for every one of these frames
        for _ in range(2):
            for _ in range(3):
                pt.Render()
            pt.Synchronize()
        s2 = stats()
        assert s2["tile_masks_valid"] and s2["mask_builds"] == s1["mask_builds"]
        assert_same_colour(pt.Result, render(b.blob, 18), f"{case.name}, degenerate scene, cached masks")
    finally:
        pt.Dispose()


# ------------------------------------------------------------------------------------------------ first hit
def expected_records(oracle, case, rec):
    """the Replayer's winner and T for every record's own ray; a winner left at T = FLOAT_MAX is the reference's miss (compute.glsl:257)"""
    b = dc.built(case)
    rp = fh.Replayer(oracle, b.blob, b.ns, b.nc)
    want_id, want_t = np.full(rec.shape, -1, np.int32), np.full(rec.shape, np.inf, np.float32)
    for y in range(rec.shape[0]):
        for x in range(rec.shape[1]):
            rp.set_ray(rec[y, x]["origin"], rec[y, x]["dir"])
            winner, T = rp.trace()
            if winner >= 0 and T != fh.FLOAT_MAX:
                want_id[y, x], want_t[y, x] = winner, T
    return want_id, want_t


@pytest.mark.parametrize("ray", ["sample0", "pinhole"])
@pytest.mark.parametrize("case", FIRST_HIT, ids=ids)
def test_first_hit_equals_the_replayer(oracle, case, ray):
    """pt_first_hit records — id, and t as words — equal the reference's RayTrace re-run on the record's own ray with the oracle's leaf
    functions, on the whole image and for one picked tile; F2: the pinhole origin is ViewPos bit for bit"""
    b = dc.built(case)
    pt = tracer(case, b.blob, b.ns, b.nc)
    try:
        if ray == "pinhole":
            pt.SetFirstHitRay(N.PT_RAY_PINHOLE)
        rec = pt.FirstHit(1)
        y0, rows = (8, 16) if case.height >= 24 else (0, case.height)
        pt.SetTile(y0, rows)
        tile = pt.FirstHit(1)
    finally:
        pt.Dispose()
    assert rec.shape == (case.height, case.width) and tile.tobytes() == rec[y0:y0 + rows].tobytes()
    if case.klass == "F2":
        assert (dc.words(rec["origin"]) == dc.words(np.array(dc.CAM2_POS, np.float32))).all()
    want_id, want_t = expected_records(oracle, case, rec)
    bad = rec["id"] != want_id
    assert not bad.any(), f"{case.name}, {ray}: {int(bad.sum())} ids differ, first (y, x, gpu, replay) = {[(int(y), int(x), int(rec['id'][y, x]), int(want_id[y, x])) for y, x in np.argwhere(bad)[:4]]}"
    bad = dc.words(rec["t"]) != dc.words(want_t)
    assert not bad.any(), f"{case.name}, {ray}: {int(bad.sum())} distances differ as words, first at {np.argwhere(bad)[:4].tolist()}"
    share = float(np.isin(rec["id"], dc.built(case).bad).mean())
    print(f"{case.name}, {ray}: {100 * share:.1f} % of the records name a degenerate object, {int((rec['id'] < 0).sum())} misses")


# ------------------------------------------------------------------------------------------------ group handle
@pytest.mark.parametrize("case", GROUP, ids=ids)
def test_group_handle_equals_the_single_handle(case):
    b = dc.built(case)
    pt = tracer(case, b.blob, b.ns, b.nc, devices=[0, 0])  # (8-row bands)
    try:
        for _ in range(dc.FRAMES):
            pt.Render()
        got = pt.Result.copy()
    finally:
        pt.Dispose()
    assert (dc.words(got) == dc.words(gpu_image(case))).all(), f"{case.name}: the group handle's image differs from the single handle's"


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("case", [c for c in CASES if c.grid is not None], ids=ids)
def test_grid_is_what_the_case_records(native_lib, case):
    import ctypes as C
    b = dc.built(case)
    pt = tracer(case, b.blob, b.ns, b.nc)
    try:
        out = (C.c_int * 5)()
        native_lib.pt_debug_sphere_grid.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        assert native_lib.pt_debug_sphere_grid(pt._h, out) == 0
    finally:
        pt.Dispose()
    print(f"{case.name}: grid {list(out)}")
    assert bool(out[4]) == case.grid
