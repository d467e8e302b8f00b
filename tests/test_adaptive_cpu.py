"""Adaptive sampling without a GPU: the properties of its definition as tests/adaptive_reference.py restates it (the recurrence against
float64 and against textbook Welford, the butterfly, the decision rule, non-finite luminances), one restatement run driven by the CPU
oracle's frames — where the non-vacuity condition of tests/test_gpu_adaptive.py is checked before any GPU is used — and the ABI."""
import os
import re

import numpy as np

import adaptive_reference as ar
import first_hit_cases as fh

pkg = fh.pkg
F32 = np.float32
U24 = 2.0 ** -24


def _sequences(K, count, seed):
    """per step k' = 1 .. K a float32 difference d of the running mean and the new mean's luminance l (non-negative)"""
    rng = np.random.default_rng(seed)
    d = (rng.standard_normal((K, count)) * np.exp(rng.uniform(-12, 2, (K, count)))).astype(F32)
    d /= np.arange(1, K + 1, dtype=F32)[:, None]
    l = np.exp(rng.uniform(-8, 4, (K, count))).astype(F32)
    return d, l


def test_recurrence_against_float64():
    """M2 is a sum of K non-negative terms of three float32 roundings each (d d, kf (kf - 1), their product) plus K - 1 additions: the
    float32 recurrence is within a relative (K + 4) 2^-24 of the same formulas in float64 from the same float32 inputs."""
    for F in (0, 1, 5):
        K = 64
        d, _ = _sequences(K, 4096, 10 + F)
        k0 = max(F, 1)
        m2 = np.zeros(d.shape[1], F32)
        m64 = np.zeros(d.shape[1], np.float64)
        terms = 0
        for k_next in range(F + 1, K + 1):
            m2 = ar.fold_m2(m2, k_next, k0, d[k_next - 1])
            if k_next > k0:
                dd = d[k_next - 1].astype(np.float64)
                m64 = m64 + (float(k_next) * (float(k_next) - 1.0)) * (dd * dd)
                terms += 1
            assert m2.dtype == F32
            if terms == 0:
                assert (m2 == 0).all()
                continue
            ok = m64 > 1e-30  # (above the float32 subnormals, where a relative bound has no meaning)
            assert ok.sum() > 3000
            rel = np.abs(m2[ok].astype(np.float64) - m64[ok]) / m64[ok]
            assert rel.max() <= (terms + 4) * U24, (F, k_next, rel.max())
        assert terms == K - k0


def test_estimate_against_float64():
    """e adds to M2's error: j kf (1), the quotient (1), s (1), s s (2 + 1), q (6 + 1), e (1) -> (K + 4 + 10) 2^-24 for l >= 0."""
    K, F = 32, 0
    d, l = _sequences(K, 4096, 3)
    m2 = np.zeros(d.shape[1], F32)
    m64 = np.zeros(d.shape[1], np.float64)
    for k_next in range(1, K + 1):
        m2 = ar.fold_m2(m2, k_next, 1, d[k_next - 1])
        if k_next > 1:
            m64 = m64 + (float(k_next) * (k_next - 1.0)) * d[k_next - 1].astype(np.float64) ** 2
    e = ar.pixel_estimate(m2, K, 1, l[-1])
    e64 = m64 / ((K - 1.0) * K) / (1.0 + l[-1].astype(np.float64)) ** 4
    ok = (e64 > 1e-30) & (e64 < 1e30)
    assert ok.sum() > 1000
    assert (np.abs(e[ok] - e64[ok]) / e64[ok]).max() <= (K + 14) * U24


def test_float64_value_is_textbook_welford():
    """With F = 0 the sum is Welford's M2 of the samples x_k = k m_k - (k - 1) m_(k-1)."""
    rng = np.random.default_rng(7)
    K = 40
    x = np.exp(rng.uniform(-3, 3, (K, 500)))
    m = (np.cumsum(x, 0) / np.arange(1, K + 1)[:, None]).astype(F32).astype(np.float64)  # the running means, as float32 values
    xs = np.empty_like(m)
    xs[0] = m[0]
    for k in range(2, K + 1):
        xs[k - 1] = k * m[k - 1] - (k - 1) * m[k - 2]
    ours = np.zeros(500)
    for k in range(2, K + 1):
        d = m[k - 1] - m[k - 2]
        ours = ours + (float(k) * (k - 1.0)) * (d * d)
    mean, M2 = np.zeros(500), np.zeros(500)
    for k in range(1, K + 1):
        delta = xs[k - 1] - mean
        mean = mean + delta / k
        M2 = M2 + delta * (xs[k - 1] - mean)
    assert np.allclose(ours, M2, rtol=1e-9, atol=0)
    assert np.allclose(M2, ((xs - xs.mean(0)) ** 2).sum(0), rtol=1e-9, atol=0)  # (and Welford's is the sum of squared deviations)


def test_butterfly_leaves_64_equal_lanes():
    rng = np.random.default_rng(1)
    lanes = np.exp(rng.uniform(-30, 30, (2000, 64))).astype(F32)
    lanes[::7, 13:] = 0.0  # ragged tiles
    lanes[5, 3] = np.inf
    lanes[6, 3] = np.nan
    s = ar.butterfly(lanes)
    assert s.dtype == F32
    bits = s.view(np.uint32)
    assert (bits == bits[:, :1]).all()
    fin = np.isfinite(s[:, 0])
    exact = lanes.astype(np.float64).sum(1)
    assert (np.abs(s[fin, 0] - exact[fin]) <= 6 * U24 * 1.0001 * exact[fin]).all()  # six levels of additions of non-negative terms


def test_decision_rule_at_the_range_ends():
    inf, nan = F32(np.inf), F32(np.nan)
    table = [  # (k, k0, err, thr, min, max) -> active
        ((0, 1, 0.0, 1e-4, 2, 2), True),       # F = 0: k - k0 = -1 < min - 1
        ((1, 1, 0.0, 1e-4, 2, 2), True),       # one short of min
        ((2, 1, 1.0, 1e-4, 2, 2), False),      # k = max
        ((2, 1, 0.0, 1e-4, 2, 65535), False),  # min reached, err below
        ((2, 1, 1e-4, 1e-4, 2, 65535), False), # err == thr is not above
        ((2, 1, np.nextafter(F32(1e-4), inf), 1e-4, 2, 65535), True),
        ((2, 1, 0.0, 0.0, 2, 65535), False),   # thr = 0: only a positive err keeps a tile
        ((2, 1, 1e-45, 0.0, 2, 65535), True),  # the smallest subnormal
        ((65534, 1, inf, ar.FLT_MAX, 2, 65535), True),   # +inf is above FLT_MAX
        ((65535, 1, inf, ar.FLT_MAX, 2, 65535), False),  # k = max
        ((100, 1, ar.FLT_MAX, ar.FLT_MAX, 2, 65535), False),
        ((100, 1, nan, 0.0, 2, 65535), False),  # NaN compares false
        ((65533, 1, 0.0, 1.0, 65535, 65535), True),   # k - k0 = 65532 < 65534
        ((65535, 2, 0.0, 1.0, 65535, 65535), False),
        ((7, 5, 0.0, 1.0, 4, 24), True),        # F = 5: k - k0 = 2 < 3
        ((8, 5, 0.0, 1.0, 4, 24), False),
        ((8, 5, 2.0, 1.0, 4, 24), True),
    ]
    for args, want in table:
        assert bool(ar.active(*args)) is want, args


def test_non_finite_luminances():
    inf, nan = F32(np.inf), F32(np.nan)
    # e = (M2 / (j kf)) / (1 + l)^4, then e > 0 ? e : 0
    assert ar.pixel_estimate(F32(1.0), 4, 1, inf) == 0.0          # finite / inf = 0
    assert ar.pixel_estimate(F32(1.0), 4, 1, -inf) == 0.0         # (1 - inf)^4 = +inf
    assert ar.pixel_estimate(F32(1.0), 4, 1, nan) == 0.0          # NaN -> 0
    assert ar.pixel_estimate(inf, 4, 1, F32(2.0)) == inf          # an infinite M2 stays +inf
    assert ar.pixel_estimate(inf, 4, 1, inf) == 0.0               # inf / inf = NaN -> 0
    assert ar.pixel_estimate(nan, 4, 1, F32(2.0)) == 0.0
    assert ar.pixel_estimate(F32(1.0), 4, 1, F32(-1.0)) == inf    # s = 0: v / 0 = +inf
    assert ar.pixel_estimate(F32(0.0), 4, 1, F32(-1.0)) == 0.0    # 0 / 0 = NaN -> 0
    assert ar.pixel_estimate(F32(1.0), 1, 1, F32(2.0)) == 0.0     # j = 0
    # d = inf - inf = NaN poisons M2, which then reports 0 for ever
    m2 = ar.fold_m2(F32(1.0), 3, 1, nan)
    assert np.isnan(m2) and ar.pixel_estimate(m2, 3, 1, F32(1.0)) == 0.0
    assert ar.fold_m2(F32(1.0), 3, 1, inf) == inf
    assert ar.fold_m2(F32(3.0), 1, 1, nan) == 3.0                 # k' <= k0: not folded
    # a tile with one infinite pixel is infinite, with a NaN-free sum otherwise
    e = np.zeros((8, 8), F32)
    e[3, 4] = inf
    assert ar.tile_error(e, ar.tile_pixels(8, 8))[0, 0] == inf


def test_tile_layout():
    n = ar.tile_pixels(27, 43)
    assert n.shape == (4, 6) and n[0, 0] == 64 and n[0, 5] == 24 and n[3, 0] == 24 and n[3, 5] == 9 and n.sum() == 27 * 43
    e = np.arange(27 * 43, dtype=F32).reshape(27, 43)
    lanes = ar.tile_lanes(e)
    assert lanes[1, 2, 3 * 8 + 5] == e[8 + 3, 16 + 5] and lanes[3, 5, 2 * 8 + 2] == e[26, 42]
    assert lanes[3, 5, 3 * 8] == 0 and lanes[3, 5, 3] == 0


def test_restatement_on_oracle_frames(oracle):
    """Default scene at 43x27, K = 24, min 4, max 24, thr = the median over the tiles of err at k = 8: the expected counts are not vacuous,
    every tile shows its own U_k, and the records follow the table."""
    case = fh.Case("default_43x27", "default", 43, 27)
    blob, ns, nc, basic = fh.inputs(case)
    K = 24
    frames = oracle.render(case.width, case.height, basic, blob, pkg.envmap.synthetic_sky_rgba32f(32), num_spheres=ns, num_cuboids=nc, ray_depth=8,
                           spp=1, focal_length=case.focal_length, aperture=case.aperture, num_frames=K, dump_each=True)
    U = np.concatenate([np.zeros((1,) + frames.shape[1:], F32), frames])
    for F in (0, 5):
        t = ar.tabulate(U, F)
        assert t.K == K and t.k0 == max(F, 1) and (t.err[0] == 0).all() and (t.m2[0] == 0).all()
        thr = ar.median_threshold(t, 8)
        assert thr > 0
        sim = ar.Sim(t).run(26, thr, 4, 24)
        counts = sim.k
        assert ar.non_vacuous(counts, 4, 24), np.unique(counts)
        assert counts.min() >= t.k0 + 3 and counts.max() <= 24
        assert not sim.active(thr, 4, 24).any() and sim.status(thr, 4, 24, 1)["active_tiles"] == 0
        before = counts.copy()
        assert (sim.run(2, thr, 4, 24).k == before).all()  # two more passes change nothing
        img = sim.image(U)
        for ty, tx in ((0, 0), (3, 5), (1, 2)):
            k = counts[ty, tx]
            assert img[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].tobytes() == U[k][8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].tobytes()
        rec = sim.records()
        assert (rec["k"] == counts).all() and (rec["n"] == ar.tile_pixels(27, 43)).all() and (rec["err"] <= thr).sum() >= (counts < 24).sum()
        # thr = 0 reactivates every tile below max with a positive err; +FLT_MAX stops every tile that has min samples
        again = ar.Sim(t).run(3, F32(0.0), 4, 24)
        assert (again.k == F + 3).all()
        assert not again.run(5, ar.FLT_MAX, 4, 24).active(ar.FLT_MAX, 4, 24).any() and (again.k == t.k0 + 3).all()


def test_abi():
    header = open(pkg.native.HEADER).read()
    names = ("pt_adaptive_set_params", "pt_adaptive_render", "pt_adaptive_status", "pt_adaptive_read_tiles", "pt_adaptive_read_noise")
    declared = pkg.native.declared_symbols()
    for n in names:
        assert re.search(r"PT_API\s+int\s+" + n + r"\s*\(", header), n
        assert n in declared
    assert "pt_adaptive.hip" in pkg.native.SOURCES
    assert os.path.exists(os.path.join(pkg.native.CSRC, "pt_adaptive.hip"))
    for m in ("SetAdaptive", "RenderAdaptive", "AdaptiveStatus", "AdaptiveTiles", "AdaptiveNoise"):
        assert callable(getattr(pkg.PathTracer, m)), m
    assert pkg.path_tracer.ADAPTIVE_TILE_DTYPE == ar.TILE_DTYPE
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    for m in ("SetAdaptive", "RenderAdaptive", "AdaptiveStatus", "AdaptiveTiles", "AdaptiveNoise"):
        assert re.search(r"\b" + m + r"\(", host), m
