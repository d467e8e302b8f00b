"""What every case of tests/degenerate_cases.py is aimed at, proved on the frozen oracle alone (no GPU): a table whose degenerate
objects no ray meets, or whose images no degenerate object changes, cannot pass.  Only what the oracle already exports is used —
render, ray_sphere / ray_cuboid (through first_hit_cases.Replayer), cuboid_normal and pto_bounce_counts.

Conditions, per case unless said otherwise:
  first-hit share   at least 10 % of the pixels (pixel-centre pinhole rays) have a degenerate object as first hit; for objects that can
                    never be hit, their repaired twins in the repaired scene; classes that act at the second bounce need more than 2
                    bounces in at least 10 % of the pixels instead
  image moves       the oracle's image differs from the base scene's (degenerate objects repaired or removed) in at least 5 % of
                    the pixels — or, for the cases listed in STILL, equals it word for word
  NaN share         at most 25 % of the pixels hold a NaN colour, alpha is exactly 1 everywhere; all cases together hold at least
                    100 NaN pixels (else same_colour's NaN == NaN rule would never be exercised)
  cuboid normals    the scaled rooms hold at least 50 first hits whose cuboid_normal is NaN; the EPSILON-thick box seen edge-on holds
                    at least 50 hits with two non-zero components
  ties              F3: at least 50 pixels with an exact tie t1 == T between two objects, and the lower index wins every one — checked
                    on two paths that do not share the bookkeeping that found the ties: Replayer.trace(), and the oracle's own
                    RayTrace through the id-emissive render of first_hit_cases.py
  determinism       two renders give the same words, also with 1 versus 16 threads
"""
import numpy as np
import pytest

import degenerate_cases as dc

CASES = dc.CASES
ids = lambda c: c.name  # noqa: E731


def test_the_table_covers_what_it_must():
    classes = {c.klass for c in CASES}
    assert classes == {"F1", "F2", "F3", "F4", "F5", "F6", "N"}
    sizes = {(c.width, c.height) for c in CASES}
    assert (75, 43) in sizes and (8, 8) in sizes and all(w <= 75 and h <= 43 for w, h in sizes)
    assert all(c.depth == 8 and c.spp == 1 for c in CASES) and dc.FRAMES == 2
    assert {c.env for c in CASES} == {"sky_f32_32", "sky_srgb_32"}
    assert any(c.grid is True for c in CASES if c.klass == "F6") and any(c.grid is False for c in CASES if c.klass == "F6")
    assert any(c.grid is False for c in dc.TIER_N)  # the non-finite sphere among >= 64
    for c in CASES:  # `grid` is recorded exactly for the cases with at least 64 spheres
        assert (c.grid is not None) == (dc.built(c).ns >= 64), c.name
    assert any(c.aperture > 0 for c in CASES) and any(c.aperture == 0 for c in CASES)
    f2 = [c for c in CASES if c.klass == "F2"]
    assert len(f2) >= 3 and all(c.position == dc.CAM2_POS and c.aperture == 0.0 for c in f2)
    b = np.frombuffer(dc.basic(f2[0]), np.float32)
    assert (b[28:31].view(np.uint32) == b[32:35].view(np.uint32)).all()  # the ray origin IS ViewPos for that camera
    assert sum(c.ties for c in CASES) >= 3 and sum(c.nan_normals for c in CASES) == 2 and any(c.q2 for c in CASES)
    for c in CASES:  # every `repaired` scene has the counts of the case's own: an edit can swap one for the other in place
        b = dc.built(c)
        assert (b.repaired or b.base)[1:] == (b.ns, b.nc), c.name
    for name in ("f5_ior", "n_mat_a"):  # the material values sit on cuboids too: five glass boxes in view, distinct values
        b = dc.built(dc.BY_NAME[name])
        mats = {np.frombuffer(b.blob, np.uint32)[5120 + 24 * j + 8:5120 + 24 * j + 24].tobytes() for j in range(2, 7)}
        assert len(mats) == 5 and all(256 + j in b.bad for j in range(2, 7)), name
    past = [c for c in CASES if c.aim == "none" and not dc.built(c).bad]
    assert len(past) >= 2 and all(c.name in dc.STILL for c in past)


def test_f2_cameras_sit_on_the_geometry_exactly():
    f = lambda name: np.frombuffer(dc.built(dc.BY_NAME[name]).blob, np.float32)  # noqa: E731
    pos = np.array(dc.CAM2_POS, np.float32)
    assert (f("f2_centre")[0:3] == pos).all()
    s = f("f2_surface")[20 * 12:20 * 12 + 4].astype(np.float64)
    assert ((s[:3] - pos) ** 2).sum() - s[3] ** 2 == 0.0
    c = f("f2_face")
    assert c[5120 + 24 * 1 + 5] == pos[1] and c[5120 + 24 * 2 + 0] == pos[0]


def test_f3_groups_lie_in_and_across_sphere_runs():
    """the run rule (bit i clear: sphere i's x and z words equal sphere i - 1's): the coincident spheres hold shared and unshared steps"""
    w = np.frombuffer(dc.built(dc.BY_NAME["f3_spheres"]).blob, np.uint32)
    shares = [bool(w[20 * i] == w[20 * (i - 1)] and w[20 * i + 2] == w[20 * (i - 1) + 2]) for i in range(1, 12)]
    assert shares == [True, True, False, True, True, False, True, True, False, True, True]
    assert (w[20 * 1:20 * 1 + 4] == w[0:4]).all() and (w[20 * 4:20 * 4 + 4] == w[20 * 3:20 * 3 + 4]).all() and (w[20 * 5:20 * 5 + 4] == w[20 * 3:20 * 3 + 4]).all()
    assert (w[20 * 7:20 * 7 + 3] == w[20 * 6:20 * 6 + 3]).all() and w[20 * 7 + 3] != w[20 * 6 + 3]


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_first_hit_share(oracle, case):
    if case.aim == "none":  # slots past the count, objects behind the camera that can never be hit: no primary ray meets them
        assert case.name in dc.STILL
        b = dc.built(case)
        if b.bad:  # ... but bounce rays must: the repaired twins, seen by bounce rays only, change pixels
            assert not np.isin(dc.case_replay(oracle, case, "repaired")[0], b.bad).any()
            blob, ns, nc = b.repaired
            twin = oracle.render(case.width, case.height, dc.basic(case), blob, dc.env(case), num_frames=dc.FRAMES, **dc.oracle_kwargs(case, ns, nc))
            reached = float((~dc.same_colour(twin, dc.oracle_image(oracle, case, "base"))).mean())
            print(f"{case.name}: the repaired twins change {100 * reached:.1f} % of the pixels through bounce rays")
            assert reached >= 0.05, f"{case.name}: bounce rays reach the objects' place in only {100 * reached:.1f} % of the pixels"
        return
    if case.aim == "bounce":
        share = float((dc.bounce_counts(oracle, case, 0) > 2).mean())
        what = "pixels with more than 2 bounces"
    else:
        share = dc.first_hit_share(oracle, case)
        what = "pixels whose first hit is a degenerate object" + (" (its repaired twin)" if case.aim == "candidate" else "")
        if case.aim == "candidate":  # ... and the object itself is never hit
            assert not np.isin(dc.case_replay(oracle, case)[0], dc.built(case).bad).any(), case.name
    print(f"{case.name}: {100 * share:.1f} % {what}")
    assert share >= 0.10, f"{case.name}: only {100 * share:.1f} % {what}"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_image_moves_or_stays(oracle, case):
    got, base = dc.oracle_image(oracle, case), dc.oracle_image(oracle, case, "base")
    if case.name in dc.STILL:
        assert (dc.words(got) == dc.words(base)).all(), f"{case.name}: the image must equal the base scene's word for word"
        assert not dc.nan_pixels(got).any()  # (the strict comparison of the GPU tests needs no NaN rule)
    else:
        moved = dc.moved_share(oracle, case)
        print(f"{case.name}: {100 * moved:.1f} % of the pixels differ from the base scene's")
        assert moved >= 0.05, f"{case.name}: only {100 * moved:.1f} % of the pixels move"


def test_nan_share(oracle):
    total, seen = 0, set()
    for case in CASES:
        img = dc.oracle_image(oracle, case)
        nan = dc.nan_pixels(img)
        assert (dc.words(img[..., 3]) == 0x3F800000).all(), f"{case.name}: alpha"
        assert nan.mean() <= 0.25, f"{case.name}: {100 * nan.mean():.1f} % NaN pixels"
        if nan.any():
            rgb = img[..., :3]
            seen |= {int(v) & 0xFFC00000 for v in dc.words(rgb)[np.isnan(rgb)]}
            print(f"{case.name}: {int(nan.sum())} NaN pixels")
        total += int(nan.sum())
    print(f"{total} NaN pixels in all; sign and quiet bit of the NaN words seen: {sorted(hex(v) for v in seen)}")
    assert total >= 100


def hit_points(oracle, case):
    """first hits on cuboids (pixel-centre rays): (cuboid index, hit point fma(d, T, o) as the oracle forms it) per such pixel"""
    winner, T, _ = dc.case_replay(oracle, case)
    o, d = dc.pinhole_rays(dc.basic(case), case.width, case.height)
    for y, x in np.argwhere(winner >= dc.PT_MAX_SPHERES):
        p = (d[y, x].astype(np.float64) * np.float64(T[y, x]) + o.astype(np.float64)).astype(np.float32)  # (the product of two binary32 is exact in binary64)
        yield int(winner[y, x]) - dc.PT_MAX_SPHERES, p


def normal_classes(oracle, case):
    """-> counts of first hits by the oracle's cuboid_normal: [NaN, 0, 1, 2, 3 non-zero components]"""
    f = np.frombuffer(dc.built(case).blob, np.float32)
    counts = np.zeros(5, int)
    for j, p in hit_points(oracle, case):
        n = oracle.cuboid_normal(f[5120 + 24 * j:5120 + 24 * j + 3], f[5120 + 24 * j + 4:5120 + 24 * j + 7], p)
        counts[int((n != 0).sum()) + 1 if np.isfinite(n).all() else 0] += 1
    return counts


@pytest.mark.parametrize("case", [c for c in CASES if c.nan_normals or c.q2], ids=ids)
def test_cuboid_normals(oracle, case):
    counts = normal_classes(oracle, case)
    print(f"{case.name}: first hits with a NaN normal / 0 / 1 / 2 / 3 non-zero components: {counts.tolist()}")
    if case.nan_normals:
        assert counts[0] >= 50
    if case.q2:
        assert counts[3] >= 50


@pytest.mark.parametrize("case", [c for c in CASES if c.ties], ids=ids)
def test_ties_go_to_the_lower_index(oracle, case):
    winner, _, tie = dc.case_replay(oracle, case)
    tied = tie >= 0
    print(f"{case.name}: {int(tied.sum())} pixels with an exact tie t1 == T, pairs {sorted({(int(a), int(b)) for a, b in zip(winner[tied], tie[tied])})}")
    assert tied.sum() >= 50
    assert (winner[tied] < tie[tied]).all()  # (holds by the construction of dc.replay; the two checks below are the independent ones)
    # 1. Replayer.trace(), which keeps no tie bookkeeping, names the same winner and T on every pixel
    import first_hit_cases as fh
    b = dc.built(case)
    rp = fh.Replayer(oracle, b.blob, b.ns, b.nc)
    o, d = dc.pinhole_rays(dc.basic(case), case.width, case.height)
    T = dc.case_replay(oracle, case)[1]
    for y, x in np.argwhere(tied):
        rp.set_ray(o, d[y, x])
        w, t = rp.trace()
        assert w == winner[y, x] and np.float32(t) == T[y, x], (case.name, int(y), int(x), w, int(winner[y, x]))
    # 2. the oracle's own RayTrace: object k emits (k + 1, 0, 0), one frame at depth 1 against a black environment leaves k + 1 in the
    # red channel (first_hit_cases.py).  Its ray is the frame's jittered sample, not the pixel centre — for objects with IDENTICAL
    # geometry words every ray that meets one meets the other at the same t1, so on the tied pixels of such pairs the higher index may
    # never appear, and the lower one appears wherever the jitter did not carry the ray past the silhouette.
    img = oracle.render(case.width, case.height, dc.basic(case), fh.id_emissive_blob(b.blob, b.ns, b.nc), np.zeros((6, 2, 2, 4), np.float32),
                        num_frames=1, **dict(dc.oracle_kwargs(case, b.ns, b.nc), ray_depth=1))
    ids = (np.rint(img[..., 0].astype(np.float64)) - 1).astype(np.int32)
    f = np.frombuffer(b.blob, np.uint32)
    geometry = lambda k: f[20 * k:20 * k + 4].tobytes() if k < 256 else f[5120 + 24 * (k - 256):5120 + 24 * (k - 256) + 8].tobytes()  # noqa: E731
    twins = tied & np.array([[tie[y, x] >= 0 and geometry(int(winner[y, x])) == geometry(int(tie[y, x])) for x in range(case.width)] for y in range(case.height)])
    losers = {int(k) for k in tie[twins]} - {int(k) for k in winner[twins]}
    agree = float((ids[twins] == winner[twins]).mean())
    print(f"{case.name}: {int(twins.sum())} tied pixels between identical objects; the oracle's first hit there is the lower index in {100 * agree:.1f} %, "
          f"objects that lose every tie: {sorted(losers)}")
    assert twins.sum() >= 50 and agree >= 0.9
    assert not np.isin(ids, sorted(losers)).any(), f"{case.name}: an object that loses every tie is somewhere the oracle's first hit"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_oracle_is_deterministic(oracle, case):
    b = dc.built(case)
    kw = dict(num_frames=dc.FRAMES, **dc.oracle_kwargs(case, b.ns, b.nc))
    first = dc.oracle_image(oracle, case)
    for threads in (1, 16):
        again = oracle.render(case.width, case.height, dc.basic(case), b.blob, dc.env(case), threads=threads, **kw)
        assert (dc.words(again) == dc.words(first)).all(), f"{case.name}, {threads} threads"


def test_same_colour_rule():
    a = np.zeros((1, 4, 4), np.float32)
    a[..., 3] = 1.0
    b = a.copy()
    a.view(np.uint32)[0, 0, 0], b.view(np.uint32)[0, 0, 0] = 0xFFC00000, 0x7FC00000  # both NaN: equal, and counted as NaN-only
    a[0, 1, 1], b[0, 1, 1] = 0.0, -0.0                                               # +0 against -0: different words
    a.view(np.uint32)[0, 2, 2] = 0x7FC00000                                          # NaN against a number
    b.view(np.uint32)[0, 3, 3] = 0x7FC00000                                          # alpha is compared strictly
    a.view(np.uint32)[0, 3, 3] = 0xFFC00000
    assert dc.same_colour(a, b).tolist() == [[True, False, False, False]]
    assert dc.nan_only(a, b).tolist() == [[True, False, False, False]]
