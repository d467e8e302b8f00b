"""The denoiser's restatements on adversarial images (tests/denoise_inputs.py), without a GPU: the generator places what it says; the
arithmetic under the restatements is IEEE; the restatements accept every case that tests/test_gpu_denoise_inputs.py feeds the kernels;
what the definition ("Non-finite and out-of-range colour") does with a non-finite pixel, as footprints; and the
inputs bite: edited copies of the passes that break one arithmetic rule each equal the restatement on plain noise and differ on the
recipes."""
import warnings

import numpy as np
import pytest

import denoise_input_cases as dc
import denoise_inputs as di
import denoise_reference as dr
import denoise_temporal_reference as dt
import denoise_variance_reference as dv
import first_hit_cases as fh

F = np.float32
R = di.Recipe
TINY = dc.TINY


# ------------------------------------------------------------------------------------------------ synthetic guides
def synthetic_ids(H, W, isolated=True):
    """Two ids side by side along the longer axis (0, and 256 from 0.6 of the way), a miss region in the corner of the far end (a
    quarter of the rows, a sixth of the columns), and — where there is room — one pixel of a third id amid id 0 (no first difference
    of u is valid around it: n = 0 in stage V)."""
    ids = np.zeros((H, W), np.int32)
    if W >= H:
        ids[:, int(0.6 * W):] = 256
    else:
        ids[int(0.6 * H):, :] = 256
    ids[H - max(1, H // 4):, W - max(1, W // 6):] = -1
    if isolated and H >= 8 and W >= 8:
        ids[H // 4, W // 4] = 7
    return ids


def plane_guides(ids, shift=(0.0, 0.0)):
    """A plane z = 0 seen head-on from z = 10 (as plane_guides of tests/test_denoise_cpu.py), at any size: pos = (x, y, 0) / 10 + shift,
    t = 10; a miss as the guide kernel writes it."""
    H, W = ids.shape
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    yy, xx = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    g["pos"][..., 0], g["pos"][..., 1] = xx * F(0.1) + F(shift[0]), yy * F(0.1) + F(shift[1])
    g["normal"][:] = np.asarray((0.0, 0.0, 1.0), F)
    g["t"] = F(10.0)
    g["id"] = ids
    miss = ids == -1
    g["pos"][miss], g["normal"][miss], g["t"][miss] = 0.0, 0.0, np.inf
    return g


def plane_camera(H, W):
    """The camera that sees plane_guides(shift = 0) (plane_camera of tests/test_denoise_temporal_cpu.py, at any size)."""
    return np.diag([20.0 / W, 20.0 / H, -0.1]).astype(F), np.array([(W - 1) / 20.0, (H - 1) / 20.0, 10.0], F)


def guides_for(shape):
    W, H = shape
    return plane_guides(synthetic_ids(H, W))


# ------------------------------------------------------------------------------------------------ the arithmetic under the reference
def test_the_arithmetic_under_the_restatements_is_ieee():
    assert F(1e-39) * F(0.5) == F(5e-40)
    dc.assert_ieee_arithmetic()  # ... and a restatement pass over subnormal_block returns subnormal, non-zero colours


# ------------------------------------------------------------------------------------------------ the generator
def test_the_generator_is_deterministic_and_places_what_it_says():
    ids = synthetic_ids(67, 131)
    for rec in (di.NOISE, R("finite_specials"), R("finite_specials", True), R("subnormal_block"), R("subnormal_block", True),
                R("nonfinite_seed"), R("nonfinite_seed", True, "+inf", 0), R("nonfinite_seed", where="small"), R("flat"), R("zero")):
        a, b = di.plan(ids, rec, 5), di.plan(ids, rec, 5)
        assert a.image.tobytes() == b.image.tobytes() and di.build(ids, rec, 5).tobytes() == a.image.tobytes(), rec.name
        assert a.image.dtype == np.float32 and a.image.shape == (67, 131, 4) and (a.image[..., 3] == 1).all()
        base = di.build(ids, di.NOISE, 5)
        assert dc.same(a.image[~a.special], base[~a.special]).all()  # everything else is the seeded noise
        if rec.kind != "noise":
            assert (a.special & (ids >= 0)).any()
        if rec.boundary:
            assert (a.special & (ids == -1)).any()
            xs, ys = di.boundary_xy(67, 131)
            assert sorted(xs) == [0, 15, 16, 63, 64, 130] and sorted(ys) == [0, 3, 4, 15, 16, 66]
            if rec.kind != "nonfinite_seed":
                assert all(a.special[y, x] for y in ys for x in xs if ids[y, x] >= 0)
    base = di.build(ids, di.NOISE, 5)[..., :3]
    assert base.min() >= 0.2 and base.max() <= 0.8
    # finite_specials: several hundred pixels, every value of the list, both whole colours
    fs = di.plan(ids, R("finite_specials"), 5)
    assert fs.special.sum() == 300 and np.isfinite(fs.image).all()
    got = fs.image[fs.special][:, :3]
    for v in di.FINITE_VALUES:
        assert (dc.bits(got) == dc.bits(np.array(v, F))).any(), v
    for colour in (di.GREY_MINUS_ONE, di.L_LARGEST):
        assert (got == np.array(colour, F)).all(-1).any()
    one, three = (((got < 0.2) | (got > 0.8)).sum(-1) == k for k in (1, 3))
    assert one.any() and three.any()  # some with one channel set, some with all three
    # the grey: l within an ulp of -1, so 1 + l is 0 or tiny and u is infinite or huge; the largest colour
    with np.errstate(all="ignore"):
        grey = np.array(di.GREY_MINUS_ONE, F)
        l = (F(0.2126) * grey[0] + F(0.7152) * grey[1]) + F(0.0722) * grey[2]
        assert abs(float(l) + 1.0) <= 2.0 ** -23 and abs(float(F(1.0) + l)) <= 2.0 ** -23
        u = dr.u_of(grey)
        print(f"grey -1: l = {float(l)!r}, 1 + l = {float(F(1.0) + l)!r}, u = {float(u)!r}")
        assert np.isinf(u) or abs(float(u)) >= 2.0 ** 22
        # the largest l of finite channels is FLT_MAX, not +inf (l does not decrease in r, g, b); u = FLT_MAX / FLT_MAX = 1
        big = np.array(di.L_LARGEST, F)
        l = (F(0.2126) * big[0] + F(0.7152) * big[1]) + F(0.0722) * big[2]
        assert l == di.FLT_MAX and F(1.0) + l == di.FLT_MAX and dr.u_of(big) == 1
        assert float(F(0.2126)) + float(F(0.7152)) + float(F(0.0722)) == 1.0
    # subnormal_block: at least 10x10 inside one id, every channel subnormal and non-zero
    for rec in (R("subnormal_block"), R("subnormal_block", True)):
        sb = di.plan(ids, rec, 5)
        y0, y1, x0, x1, target = sb.block
        inblock = np.zeros_like(sb.special)
        inblock[y0:y1, x0:x1] = ids[y0:y1, x0:x1] == target
        assert y1 - y0 >= 10 and x1 - x0 >= 10 and inblock.sum() >= 100 and (sb.special & inblock).sum() == inblock.sum()
        c = sb.image[sb.special][:, :3]
        assert (c >= F(1e-39)).all() and (c <= F(8e-39)).all() and (c < TINY).all()
    assert di.plan(ids, R("subnormal_block", True), 5).block[:4] == (10, 22, 10, 22)  # across x = 15 | 16 and y = 15 | 16
    # nonfinite_seed: one pixel, one channel, where it says
    d = di.edge_distance(ids)
    for val, ch in (("nan", 1), ("+inf", 0), ("-inf", 2)):
        nf = di.plan(ids, R("nonfinite_seed", value=val, channel=ch), 5)
        (y, x), = nf.seeds
        assert nf.special.sum() == 1 and nf.distance == d[y, x] == d.max() and ids[y, x] >= 0
        bad = ~np.isfinite(nf.image)
        assert bad.sum() == 1 and bad[y, x, ch] and dc.same(nf.image[y, x, ch], di.NONFINITE[val])
    small = di.plan(ids, R("nonfinite_seed", where="small"), 5)
    assert di.smallest_id(ids) == 256 and ids[small.seeds[0]] == 256
    nb = di.plan(ids, R("nonfinite_seed", True), 5)
    assert nb.seeds[0] == (4, 16) and ids[nb.seeds[1]] == -1 and len(nb.seeds) == 2 and nb.distance == d[4, 16]


def test_edge_distance():
    ids = np.zeros((9, 11), np.int32)
    ids[:, 8:] = 3
    ids[0, 0] = -1
    d = di.edge_distance(ids)
    assert d[4, 4] == 3 and d[4, 0] == 0 and d[4, 7] == 0 and d[4, 6] == 1 and d[0, 0] == -1 and d[1, 1] == 0 and d[4, 9] == 1
    assert di.deepest(ids) == (4, 4, 3) and di.deepest(ids, 3) == (4, 9, 1)


def test_every_shape_sees_two_ids_and_hits_on_half_of_its_pixels(oracle):
    for W, H in dc.SHAPES:
        ids, _ = fh.oracle_first_hit(oracle, dc.scene_case((W, H)))
        seen = np.unique(ids[ids >= 0])
        print(f"{W}x{H}: {len(seen)} ids, hits on {float((ids >= 0).mean()):.2f} of the pixels")
        assert len(seen) >= 2 and (ids >= 0).sum() * 2 >= ids.size


# ------------------------------------------------------------------------------------------------ the restatements accept every case
def run_case(case, guides):
    pl = di.plan(guides["id"], case.recipe, case.seed)
    want, v0 = dc.restate(case, pl.image, guides)
    return pl, want, v0


@pytest.mark.parametrize("table", ["CASES", "EXTREMES"])
def test_the_restatements_accept_every_case_without_raising_or_warning(table):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for case in getattr(dc, table):
            g = guides_for(case.shape)
            pl, want, v0 = run_case(case, g)
            nonfinite, changed, _ = dc.shares(pl.image, want, g["id"])  # (CASES: asserted on the scene's id maps below, and on the GPU's guides)
            print(f"{case.name}: non-finite expected {nonfinite:.3f}, changed {changed:.3f}")
            if table == "EXTREMES":  # plain noise: nothing non-finite to spread, so the conditions hold on the synthetic plane too
                dc.assert_case_can_fail(case, pl.image, want, g["id"], pl.special)
            assert want.shape == pl.image.shape and (want[..., 3] == 1).all()
            assert dc.same(want[g["id"] == -1], pl.image[g["id"] == -1]).all()  # a miss passes through, whatever it holds
            if case.variance:
                assert v0.shape == g.shape and not v0[g["id"] == -1].any()
            if case.sigma_color == 1e-40:
                assert np.isinf(dr.inv_sigma(case.sigma_color, 0)) and dc.same(want, pl.image).all()  # every pixel passes through
            if case.sigma_color == 3e38:
                assert 0 < dr.inv_sigma(case.sigma_color, 0) < TINY
            if case.recipe.kind in ("flat", "zero"):
                assert dc.same(want, pl.image).all() and (v0 is None or not v0.any())
    assert dv.k2_of(1e-25) == 0 and 0 < dv.k2_of(1e-19) < TINY and np.isfinite(dv.k2_of(1e19)) and np.isinf(dv.k2_of(3e38))


def test_the_cases_can_fail_on_the_id_maps_of_the_scene(oracle):
    """The hiding conditions again, on the id maps the kernels will see (the oracle's first hit) with the plane's geometry: in the fixed
    mode the spread of a non-finite value depends on the ids alone (0 * NaN is NaN whatever the weight was)."""
    for case in dc.CASES:
        ids, _ = fh.oracle_first_hit(oracle, dc.scene_case(case.shape))
        g = plane_guides(ids)
        pl, want, _ = run_case(case, g)
        nonfinite, changed = dc.assert_case_can_fail(case, pl.image, want, ids, pl.special)
        print(f"{case.name}: non-finite expected {nonfinite:.3f}, changed {changed:.3f}; seeds {pl.seeds} distance {pl.distance}")


def test_the_temporal_restatement_accepts_every_case_without_raising_or_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for tc in dc.TEMPORAL_CASES:
            W, H = tc.shape
            ids = synthetic_ids(H, W)
            ga, gb = plane_guides(ids), plane_guides(ids, shift=(0.03, 0.02))
            B, O = plane_camera(H, W)
            pa, pb = di.plan(ids, tc.history, tc.seed), di.plan(ids, tc.current, tc.seed + 1)
            a, b = pa.image, pb.image
            p = dr.Params(iterations=tc.iterations)
            sv = 6.0 if tc.variance else None
            hist = dt.integrate(a, tc.n_history, ga, None, None, None, None, p, tc.max_history)
            I = dt.integrate(b, tc.n, gb, hist, ga, B, O, p, tc.max_history)
            out = dt.filter(I, gb, p, sv)
            found = (I[..., 3] > F(tc.n)) & (ids >= 0)
            assert dc.same(hist[..., :3], a[..., :3]).all() and (hist[..., 3] == tc.n_history).all()
            assert found.sum() * 2 > (ids >= 0).sum()
            assert (out[..., 3] == 1).all() and dc.same(I[ids == -1][:, :3], b[ids == -1][:, :3]).all()
            for epoch, rec, pl, wI, wout in (("A", tc.history, pa, hist, dt.filter(hist, ga, p, sv)), ("B", tc.current, pb, I, out)):
                got = dc.assert_temporal_case_can_fail(tc, rec, pl.image, wI, wout, ids, pl.special)
                print(f"{tc.name} epoch {epoch}: {int(found.sum()) if epoch == 'B' else 0} of {int((ids >= 0).sum())} hit pixels found history; "
                      f"{got[0]:.3f} expect a non-finite I, {got[1]:.3f} a non-finite output, the stage and the filter change {got[2]:.3f}")


def test_temporal_footprint_of_one_nonfinite_pixel():
    """The plane seen again after a shift of (0.3, 0.2) pixels: the 2x2 footprint of a pixel p is p, p + (1, 0), p + (0, 1), p + (1, 1).  A
    NaN history pixel s enters Sh of every pixel whose footprint holds it, whatever its weight: I is non-finite at s, s - (1, 0),
    s - (0, 1), s - (1, 1) and nowhere else.  A NaN pixel of the current image makes I non-finite at itself alone, for any n."""
    H, W = 67, 131
    ids = np.zeros((H, W), np.int32)
    ga, gb = plane_guides(ids), plane_guides(ids, shift=(0.03, 0.02))
    B, O = plane_camera(H, W)
    seed, noise = di.plan(ids, R("nonfinite_seed"), 11), di.build(ids, di.NOISE, 12)
    (y, x), = seed.seeds
    for n in (0, 1, 1000):
        for mh in (1, 32, 65535):
            hist = dt.integrate(seed.image, 3, ga, None, None, None, None, dr.Params(), mh)
            bad = nonfinite(dt.integrate(noise, n, gb, hist, ga, B, O, dr.Params(), mh))
            assert sorted(map(tuple, np.argwhere(bad).tolist())) == [(y - 1, x - 1), (y - 1, x), (y, x - 1), (y, x)], (n, mh)
            hist = dt.integrate(noise, 3, ga, None, None, None, None, dr.Params(), mh)
            bad = nonfinite(dt.integrate(seed.image, n, gb, hist, ga, B, O, dr.Params(), mh))
            assert np.argwhere(bad).tolist() == [[y, x]], (n, mh)  # (also at n = 0: 0 * NaN is NaN)


# ------------------------------------------------------------------------------------------------ footprints of a non-finite pixel
def nonfinite(img):
    return ~np.isfinite(img[..., :3]).all(-1)


def block(shape, y, x, half):
    m = np.zeros(shape, bool)
    m[max(0, y - half):y + half + 1, max(0, x - half):x + half + 1] = True
    return m


@pytest.mark.parametrize("value, channel", [("nan", 1), ("+inf", 0), ("-inf", 2)])
def test_fixed_mode_footprint_of_one_nonfinite_pixel(value, channel):
    """A tap of weight 0 still multiplies its colour, and 0 * NaN = 0 * inf = NaN: after n passes every pixel of the seed's id within
    2 (2^n - 1) of it — the (4 (2^n - 1) + 1)^2 block — is non-finite in the seed's channel, and nothing else is.  (+-inf: l = +-inf,
    u = inf / inf = NaN.)  The seed itself passes through: its own u is NaN, so its W is 0."""
    g = plane_guides(np.zeros((131, 131), np.int32))
    pl = di.plan(g["id"], R("nonfinite_seed", value=value, channel=channel), 1)
    (y, x), = pl.seeds
    assert (y, x) == (65, 65) and pl.distance >= 62
    out = pl.image
    widths = []
    for n in range(1, 5):
        out = dr.atrous_pass(out, g, n - 1, dr.Params())
        side = 4 * (2 ** n - 1) + 1
        bad = nonfinite(out)
        widths.append(int(bad[y].sum()))
        assert (bad == block(bad.shape, y, x, side // 2)).all() and bad.sum() == side * side
        assert not np.isfinite(out[bad][:, channel]).any() and np.isfinite(np.delete(out[..., :3], channel, -1)).all()
        assert dc.same(out[y, x], pl.image[y, x]).all()
    print(f"fixed mode, seed {value}: non-finite block per pass count 1..4: {widths} wide")
    assert widths == [5, 13, 29, 61]


def test_fixed_mode_footprint_at_the_default_depth_and_at_id_edges():
    # five passes on a one-id 131x67 plane: 125 wide, clipped by the image
    g = plane_guides(np.zeros((67, 131), np.int32))
    pl = di.plan(g["id"], R("nonfinite_seed"), 1)
    bad = nonfinite(dr.denoise(pl.image, g))
    print(f"fixed mode, 5 passes, 131x67, one id, seed at {pl.seeds[0]}: {int(bad.sum())} of {bad.size} pixels non-finite")
    assert pl.seeds == [(33, 65)] and bad.sum() == 125 * 67 == 8375 and (bad == block(bad.shape, 33, 65, 62)).all()
    # whatever the distance: no non-finite pixel has another id, and miss pixels are unchanged
    ids = synthetic_ids(67, 131)
    g = plane_guides(ids)
    for rec in (R("nonfinite_seed"), R("nonfinite_seed", True), R("nonfinite_seed", where="small"), R("nonfinite_seed", True, "-inf", 2)):
        pl = di.plan(ids, rec, 1)
        for it in (1, 3, 5, 6):
            p = dr.Params(iterations=it)
            reach = 2 * (2 ** it - 1)
            for out in (dr.denoise(pl.image, g, p), dv.denoise(pl.image, g, p)[0]):
                bad = nonfinite(out) & (ids >= 0)
                y, x = pl.seeds[0]
                assert bad[y, x] and (ids[bad] == ids[y, x]).all() and (bad <= block(bad.shape, y, x, reach)).all()
                assert dc.same(out[ids == -1], pl.image[ids == -1]).all()
        bad = nonfinite(dr.denoise(pl.image, g, dr.Params(iterations=3))) & (ids >= 0)
        assert (bad == (block(bad.shape, *pl.seeds[0], 14) & (ids == ids[pl.seeds[0]]))).all()  # ... and it is every pixel of that id in reach


@pytest.mark.parametrize("value, channel", [("nan", 1), ("+inf", 0), ("-inf", 2)])
def test_variance_mode_footprint_of_one_nonfinite_pixel(value, channel):
    """Stage V: the seed's u is NaN, so Dx is NaN at the seed and left of it, Dy at the seed and below it, and V0 is NaN for every centre
    whose 7x7 window visits one of those: the 8x8 block from (-4, -4) to (+3, +3) without its (-4, -4) corner, 63 pixels.  A NaN variance
    makes inv_p, every weight's c and so W fail `> 0`: those pixels pass through, with their NaN variance.  Around them Q = sum w^2 var
    turns the variance of every pixel that taps one of them NaN — 2 * step further out per pass, always ahead of the taps that could
    reach the seed itself (2 * step) — so no pixel with a finite variance ever multiplies the seed's colour: after any number of passes
    the seed is the only non-finite pixel, and the 63 are bit-equal to the input."""
    g = plane_guides(np.zeros((131, 131), np.int32))
    pl = di.plan(g["id"], R("nonfinite_seed", value=value, channel=channel), 1)
    (y, x), = pl.seeds
    v0 = dv.estimate(pl.image, g)
    want = block(v0.shape, y, x, 4)
    want[y + 4, :], want[:, x + 4] = False, False
    want[y - 4, x - 4] = False
    assert (np.isnan(v0) == want).all() and want.sum() == 63 and np.isfinite(v0[~want]).all()
    for it in range(1, 7):
        out, _ = dv.denoise(pl.image, g, dr.Params(iterations=it))
        bad = nonfinite(out)
        equal = dc.same(out[..., :3], pl.image[..., :3]).all(-1)
        print(f"variance mode, seed {value}, {it} passes: {int(bad.sum())} non-finite pixel(s), {int(np.isnan(v0).sum())} NaN estimates, "
              f"{int(equal.sum())} pixels bit-equal to the input")
        assert bad.sum() == 1 and bad[y, x] and equal[want].all() and equal.sum() == 63


# ------------------------------------------------------------------------------------------------ the inputs bite
EDITS = ("skip_zero_taps", "nan_propagating_max", "W_ge_0", "flush_subnormals", "n_ge_0")


def flush(a):
    return np.where((a != 0) & (np.abs(a) < TINY), F(0.0), a)


def edited_estimate(rgb, guides, edit):
    """dv.estimate; edit n_ge_0: `n >= 0` for `n > 0` (0 / 0 where no first difference is valid)."""
    if edit != "n_ge_0":
        return dv.estimate(rgb, guides)
    H, W = guides.shape
    ids = guides["id"]
    u = dr.u_of(np.ascontiguousarray(rgb[..., :3], dtype=F))
    with np.errstate(all="ignore"):
        Dx, Dy = np.zeros((H, W), F), np.zeros((H, W), F)
        vx, vy = np.zeros((H, W), bool), np.zeros((H, W), bool)
        ex = u[:, 1:] - u[:, :-1]
        Dx[:, :-1] = ex * ex
        vx[:, :-1] = ids[:, 1:] == ids[:, :-1]
        ey = u[1:, :] - u[:-1, :]
        Dy[:-1, :] = ey * ey
        vy[:-1, :] = ids[1:, :] == ids[:-1, :]
        n, s = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                sh = dv._shift(H, W, dy, dx)
                if sh is None:
                    continue
                P, Q = sh
                visit = ids[Q] == ids[P]
                for ok, D in ((visit & vx[Q], Dx), (visit & vy[Q], Dy)):
                    n[P] = np.where(ok, n[P] + F(1.0), n[P])
                    s[P] = np.where(ok, s[P] + D[Q], s[P])
        return np.where((n >= 0) & (ids != -1), F(0.5) * (s / n), F(0.0)).astype(F)


def edited_pass(colour, var, guides, i, p, sigma_variance, edit):
    """dr.atrous_pass (var None) / dv.variance_pass, operation for operation, with one rule broken:
    skip_zero_taps: a tap of weight 0 is skipped (the natural `if (w > 0)`); nan_propagating_max: np.maximum(x, 0) for every
    np.where(x > 0, x, 0) (fmax semantics aside: NaN stays NaN); W_ge_0: the output test is `W >= 0`; flush_subnormals: subnormal w * c
    and S / W become 0."""
    variance = var is not None
    H, W = guides.shape
    st = 1 << i
    rgb = np.ascontiguousarray(colour[..., :3], dtype=F)
    ids, pos, nrm, t = guides["id"], guides["pos"], guides["normal"], guides["t"]
    u = dr.u_of(rgb)
    den = F(p.sigma_plane) * t
    clamp = (lambda x: np.maximum(x, F(0.0))) if edit == "nan_propagating_max" else (lambda x: np.where(x > 0, x, F(0.0)))
    Wsum, S, Qsum = np.zeros((H, W), F), np.zeros((H, W, 3), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        if variance:
            var = np.ascontiguousarray(var, dtype=F)
            inv = F(1.0) / (dv.k2_of(sigma_variance) * var + dv.EPS)
        else:
            isig = dr.inv_sigma(p.sigma_color, i)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sh = dv._shift(H, W, st * dy, st * dx)
                if sh is None:
                    continue
                P, Q = sh
                h = dr.KERNEL[abs(dx)] * dr.KERNEL[abs(dy)]
                wn = clamp(dr._dot(nrm[P], nrm[Q]))
                for _ in range(p.normal_log2_power):
                    wn = wn * wn
                r = dr._dot(nrm[P], pos[Q] - pos[P]) / den[P]
                wz = clamp(F(1.0) - r * r)
                if variance:
                    du = u[Q] - u[P]
                    c = F(1.0) - (du * du) * inv[P]
                else:
                    a = (u[Q] - u[P]) * isig
                    c = F(1.0) - a * a
                c = clamp(c)
                w = ((h * wn) * wz) * (c * c)
                match = ids[Q] == ids[P]
                if edit == "skip_zero_taps":
                    match = match & (w > 0)
                prod = w[..., None] * rgb[Q]
                if edit == "flush_subnormals":
                    prod = flush(prod)
                Wsum[P] = np.where(match, Wsum[P] + w, Wsum[P])
                S[P] = np.where(match[..., None], S[P] + prod, S[P])
                if variance:
                    Qsum[P] = np.where(match, Qsum[P] + (w * w) * var[Q], Qsum[P])
        ok = ((Wsum >= 0) if edit == "W_ge_0" else (Wsum > 0)) & (ids != -1)
        quot = S / Wsum[..., None]
        if edit == "flush_subnormals":
            quot = flush(quot)
        out = np.empty((H, W, 4), F)
        out[..., :3] = np.where(ok[..., None], quot, rgb)
        out[..., 3] = F(1.0)
        var_out = np.where(ok, Qsum / (Wsum * Wsum), var).astype(F) if variance else None
    return out, var_out


def edited_denoise(image, guides, p, variance, edit):
    """-> (image, V0 or None)"""
    v0 = edited_estimate(image, guides, edit) if variance else None
    out, var = image, v0
    for i in range(p.iterations):
        out, var = edited_pass(out, var, guides, i, p, 6.0, edit)
    return out, v0


BITE_RECIPES = (R("finite_specials", True), R("subnormal_block", True), R("subnormal_block"), R("nonfinite_seed"),
                R("nonfinite_seed", True, "+inf", 0))
_bite = {}


def bite_counts():
    """{(edit or None, variance)}: (pixels differing from the restatement on plain noise, on the recipe set), summed over 1 and 3 passes."""
    if not _bite:
        ids = synthetic_ids(67, 131)
        g = plane_guides(ids)
        for variance in (False, True):
            for edit in (None,) + EDITS:
                counts = []
                for recipes in ((di.NOISE,), BITE_RECIPES):
                    total = 0
                    for rec in recipes:
                        img = di.build(ids, rec, 9)
                        for it in (1, 3):
                            p = dr.Params(iterations=it)
                            want, want_v0 = dv.denoise(img, g, p) if variance else (dr.denoise(img, g, p), None)
                            got, got_v0 = edited_denoise(img, g, p, variance, edit)
                            differ = ~dc.same(got, want).all(-1)
                            if variance:
                                differ |= ~dc.same(got_v0, want_v0)
                            total += int(differ.sum())
                    counts.append(total)
                _bite[edit, variance] = tuple(counts)
    return _bite


@pytest.mark.parametrize("variance", [False, True], ids=["fixed", "variance"])
def test_the_unedited_copies_are_the_restatements(variance):
    assert bite_counts()[None, variance] == (0, 0)


@pytest.mark.parametrize("edit", EDITS)
def test_a_pass_that_breaks_one_rule_differs_on_the_recipes(edit):
    """Each edited copy is a kernel bug the renderer's own images cannot show: on plain noise the first four equal the restatement on
    every pixel (n_ge_0 differs there too, at the one-pixel id: its estimate is 0 / 0)."""
    for variance in (False, True):
        if edit == "n_ge_0" and not variance:
            continue  # (stage V belongs to the variance mode)
        on_noise, on_recipes = bite_counts()[edit, variance]
        print(f"{edit}, {'variance' if variance else 'fixed'} mode: differs from the restatement on {on_noise} pixels of plain noise, "
              f"on {on_recipes} pixels of the recipe set")
        assert on_recipes > 0
        if edit != "n_ge_0":
            assert on_noise == 0
