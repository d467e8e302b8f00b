"""Saving, restoring and ending an adaptive state, without a GPU: the ABI; the rebuild restatement (tests/adaptive_state_reference.py)
against the states tabulated from the CPU oracle's frames, on non-finite inputs, and the levelling of pt_adaptive_end replayed on the
table — where the non-vacuity conditions of tests/test_gpu_adaptive_state.py are checked before any GPU is used — and the checkpoint
file formats with a stand-in tracer."""
import os
import re
import struct

import numpy as np
import pytest

import adaptive_reference as ar
import adaptive_state_reference as asr
import first_hit_cases as fh

pkg = fh.pkg
F32 = np.float32
K, MIN, MAX = 24, 4, 24
SAVE, END = 9, 26

_frames = {}


def oracle_frames(oracle, width, height, spp=1):
    """U_0 .. U_K of the default scene from the CPU oracle.  Made once, never changed."""
    key = (width, height, spp)
    if key not in _frames:
        case = fh.Case(f"default_{width}x{height}", "default", width, height)
        blob, ns, nc, basic = fh.inputs(case)
        frames = oracle.render(case.width, case.height, basic, blob, pkg.envmap.synthetic_sky_rgba32f(32), num_spheres=ns, num_cuboids=nc,
                               ray_depth=8, spp=spp, focal_length=case.focal_length, aperture=case.aperture, num_frames=K, dump_each=True)
        U = np.concatenate([np.zeros((1,) + frames.shape[1:], F32), frames])
        U.setflags(write=False)
        _frames[key] = U
    return _frames[key]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_abi():
    header = open(pkg.native.HEADER).read()
    declared = pkg.native.declared_symbols()
    for n in ("pt_adaptive_read_m2", "pt_adaptive_write_state", "pt_adaptive_end"):
        assert re.search(r"PT_API\s+int\s+" + n + r"\s*\(", header), n
        assert n in declared
    assert "or pt_adaptive_end" in header
    assert "pt_adaptive_state.hip" in pkg.native.SOURCES
    assert os.path.exists(os.path.join(pkg.native.CSRC, "pt_adaptive_state.hip"))
    for m in ("AdaptiveM2", "AdaptiveState", "RestoreAdaptive", "EndAdaptive"):
        assert callable(getattr(pkg.PathTracer, m)), m
    assert isinstance(pkg.PathTracer.AdaptiveLive, property) and pkg.PathTracer.AdaptiveLive.fset is None
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    for m in ("AdaptiveM2", "AdaptiveState", "RestoreAdaptive", "EndAdaptive", "AdaptiveLive"):
        assert re.search(r"\b" + m + r"\(", host), m
    doc = open(os.path.join(pkg.native.REPO, "INTEGRATION.md")).read()
    for n in ("pt_adaptive_read_m2", "pt_adaptive_write_state", "pt_adaptive_end"):
        assert re.search(r"DllImport[^\n]*\n?[^\n]*" + n, doc), n


def test_rebuild_reproduces_the_tabulated_states(oracle):
    """(U_k, M2_k, k, k0) -> the e and err a pass left at k, for every k of the table, k = F included (e = 0, err = +0)"""
    U = oracle_frames(oracle, 43, 27)
    for F in (0, 5):
        t = ar.tabulate(U, F)
        for k in range(F, K + 1):
            e, err = asr.rebuild(U[k], t.m2[k - F], np.full(t.n.shape, k, np.int32), t.k0)
            assert (bits(e) == bits(t.e[k - F])).all(), (F, k)
            assert (bits(err) == bits(t.err[k - F])).all(), (F, k)
        e, err = asr.rebuild(U[F], t.m2[0], np.full(t.n.shape, F, np.int32), t.k0)
        assert not bits(e).any() and not bits(err).any()  # +0 everywhere, as pt_adaptive_init_kernel leaves it
        # a state whose tiles stand at different counts: every tile rebuilt with its own k
        sim = ar.Sim(t).run(SAVE, ar.median_threshold(t, 8), MIN, MAX)
        m2, want_e = sim.stats()
        e, err = asr.rebuild(sim.image(U), m2, sim.k, t.k0)
        assert (bits(e) == bits(want_e)).all() and (bits(err) == bits(sim.err())).all()


def test_rebuild_on_non_finite_inputs():
    inf, nan = F32(np.inf), F32(np.nan)
    sub = F32(1e-45)
    m2 = np.array([nan, inf, -inf, F32(-3.0), sub, -sub, ar.FLT_MAX, F32(0.0), F32(-0.0), F32(2.5)], F32)
    grey = lambda l: np.array([l, l, l, 1.0], F32)  # l(grey) = l up to rounding
    colours = [grey(F32(0.25)), grey(F32(-1.0)), grey(inf), grey(-inf), grey(nan), grey(ar.FLT_MAX), grey(F32(0.0))]
    rows, width = len(colours), len(m2)
    image = np.repeat(np.stack(colours)[:, None, :], width, 1)
    sums = np.repeat(m2[None, :], rows, 0)
    k = np.full(ar.tile_grid(rows, width), 7, np.int32)
    with np.errstate(all="ignore"):
        e, err = asr.rebuild(image, sums, k, 1)
        assert e.dtype == F32 and not np.isnan(e).any() and not (e < 0).any() and not np.signbit(e).any()
        # l = 0.25 (q finite): NaN -> 0, +inf stays, -inf and negatives -> 0, a subnormal underflows to 0, FLT_MAX stays finite
        assert e[0, 0] == 0 and e[0, 1] == inf and e[0, 2] == 0 and e[0, 3] == 0 and e[0, 4] == 0 and e[0, 5] == 0 and 0 < e[0, 6] < inf
        assert e[6, 9] == F32(2.5) / (F32(6.0) * F32(7.0)) and e[6, 6] == ar.FLT_MAX / (F32(6.0) * F32(7.0))  # l = 0: q = 1
        # l = +inf, -inf, NaN, FLT_MAX: q = +inf or NaN: finite / inf = 0, inf / inf = NaN -> 0
        assert not e[2:6].any()
        assert not np.isnan(err).any() and (err >= 0).all() and np.isinf(err[0, 0]) and np.isinf(err[0, 1])
        # l = -1 exactly: s = 0, q = 0: a positive M2 gives +inf, zero gives 0 / 0 = NaN -> 0, a negative one -inf -> 0
        z = ar.pixel_estimate(np.array([1.0, 0.0, -1.0, nan, inf, -inf, sub], F32), 7, 1, F32(-1.0))
        assert z.tolist() == [inf, 0, 0, 0, inf, 0, 0]  # (a subnormal over 42 underflows to 0 first)
        # ... and an image whose luminance is -1 bit for bit, through the rebuild
        minus = np.repeat(asr.colour_with_luminance_minus_one()[None, None, :], 3, 1)
        assert (ar.lum(minus) == F32(-1.0)).all()
        ez, _ = asr.rebuild(minus, np.array([[1.0, 0.0, nan]], F32), np.full((1, 1), 7, np.int32), 1)
        assert ez.tolist() == [[inf, 0, 0]]
        # j < 1: whatever M2 holds, e = 0 and err = +0
        e0, err0 = asr.rebuild(image, sums, np.full(k.shape, 1, np.int32), 1)
        assert not bits(e0).any() and not bits(err0).any()


@pytest.mark.parametrize("F", (0, 5))
def test_levelling_on_the_table(oracle, F):
    """pt_adaptive_end's passes — the sampler's own under (0, 65535, kmax) — bring every tile to exactly kmax in kmax - kmin passes and not
    one earlier; the image is then U[kmax]; further passes change nothing."""
    U = oracle_frames(oracle, 43, 27)
    t = ar.tabulate(U, F)
    thr = ar.median_threshold(t, 8)
    for passes in (0, SAVE, END):
        sim = ar.Sim(t).run(passes, thr, MIN, MAX)
        kmin, kmax = int(sim.k.min()), int(sim.k.max())
        assert passes == 0 or kmin < kmax
        if kmin < kmax:
            short = ar.Sim(t)
            short.k = sim.k.copy()
            short.run(kmax - kmin - 1, asr.END_PARAMS[0], asr.END_PARAMS[1], kmax)
            assert int(short.k.min()) == kmax - 1
        got_max, ran = asr.level(sim)
        assert (got_max, ran) == (kmax, kmax - kmin) and (sim.k == kmax).all()
        assert sim.image(U).tobytes() == U[kmax].tobytes()
        assert not sim.active(asr.END_PARAMS[0], asr.END_PARAMS[1], kmax).any()
        assert (sim.run(3, asr.END_PARAMS[0], asr.END_PARAMS[1], kmax).k == kmax).all()
    # the decision under the levelling parameters is k < kmax whatever err holds, up to the largest count there is
    for k, k0, err, kmax, want in ((0, 1, 0.0, 1, True), (65534, 1, 0.0, 65535, True), (65535, 1, np.inf, 65535, False), (7, 5, np.nan, 8, True),
                                   (8, 5, np.inf, 8, False), (65534, 65534, 0.0, 65535, True)):
        assert bool(ar.active(k, k0, err, asr.END_PARAMS[0], asr.END_PARAMS[1], kmax)) is want, (k, k0, err, kmax)


def _conditions(U, F):
    t = ar.tabulate(U, F)
    thr = ar.median_threshold(t, 8)
    sim = ar.Sim(t).run(SAVE, thr, MIN, MAX)
    save_counts, active = np.unique(sim.k), int(sim.active(thr, MIN, MAX).sum())
    end_counts = sim.run(END - SAVE, thr, MIN, MAX).k.copy()
    return save_counts, active, end_counts


@pytest.mark.parametrize("what,F", [(w, F) for w in ("43x27", "43x27_rows_8_23", "16x16") for F in (0, 5)])
def test_the_gpu_cases_are_not_vacuous_on_the_oracle(oracle, what, F):
    """at the save point (9 passes) at least three distinct counts and an active tile; at the end (26) adaptive_reference.non_vacuous"""
    U = oracle_frames(oracle, 16, 16) if what == "16x16" else oracle_frames(oracle, 43, 27)
    if what == "43x27_rows_8_23":
        U = U[:, 8:24]
    save_counts, active, end_counts = _conditions(U, F)
    print(f"\n  {what} F={F}: save-point counts {save_counts.tolist()}, {active} of {end_counts.size} active; end-point counts {np.unique(end_counts).tolist()}")
    assert len(save_counts) >= 3 and active >= 1
    assert ar.non_vacuous(end_counts, MIN, MAX), np.unique(end_counts)


# ------------------------------------------------------------------------------------------------ checkpoint files
_V1 = struct.Struct("<8s8i2i2f")  # the version 1 layout, restated: what the writer before version 2 produced


class _Tracer:
    """Just what checkpoint.py touches; records every call that would change a tracer."""

    def __init__(self, w=11, h=9, frame=3, live=None):
        self.Width, self.Height, self.y0, self.rows = w, h, 0, h
        self.band_rows, self.band_world, self.band_rank = 0, 1, 0
        self.RayDepth, self.SPP, self.FocalLength, self.ApertureDiameter = 8, 1, 20.0, 0.14
        self.FrameIndex = frame
        rng = np.random.RandomState(w * 100 + h)
        self.Result = rng.rand(h, w, 4).astype(F32)
        self.Result[..., 3] = 1.0
        self.calls = []
        if live is not None:
            self.AdaptiveLive = live
            self.AdaptiveParams = (float(F32(3e-5)), 5, 77)
            self._tiles = np.empty(((h + 7) // 8, (w + 7) // 8), ar.TILE_DTYPE)
            self._tiles["k"] = frame + rng.randint(0, 9, self._tiles.shape)
            self._tiles["k0"] = max(frame, 1)
            self._tiles["err"] = rng.rand(*self._tiles.shape).astype(F32)
            self._tiles["n"] = ar.tile_pixels(h, w)
            self._m2 = rng.rand(h, w).astype(F32)
            self._m2[0, 0], self._m2[1, 1] = np.nan, np.inf

    def AdaptiveState(self):
        return {"frame_index": self.FrameIndex, "image": self.Result, "tiles": self._tiles, "m2": self._m2}

    def WriteResult(self, img, frame):
        self.calls.append(("WriteResult", img.copy(), frame))

    def RestoreAdaptive(self, image, frame_index, tiles, m2):
        self.calls.append(("RestoreAdaptive", image.copy(), frame_index, tiles.copy(), m2.copy()))

    def SetAdaptive(self, threshold, min_samples, max_samples):
        self.calls.append(("SetAdaptive", threshold, min_samples, max_samples))


def _v1_bytes(t):
    return _V1.pack(b"PTCKPT1\0", t.Width, t.Height, t.y0, t.rows, t.band_rows, t.band_world, t.band_rank, t.FrameIndex, t.RayDepth, t.SPP,
                    t.FocalLength, t.ApertureDiameter) + t.Result.tobytes()


def test_checkpoint_v2_round_trip(tmp_path):
    ck = pkg.checkpoint
    a = _Tracer(live=True)
    path = str(tmp_path / "a.ptck")
    ck.save_checkpoint(path, a)
    raw = open(path, "rb").read()
    assert raw[:8] == b"PTCKPT2\0" and len(raw) == 56 + 20 + 9 * 11 * 16 + 2 * 2 * 16 + 9 * 11 * 4
    assert raw[8:56] == _v1_bytes(a)[8:56]  # the version 1 header fields unchanged
    assert struct.unpack("<f4i", raw[56:76]) == (float(F32(3e-5)), 5, 77, 2, 2)
    assert raw[76:] == a.Result.tobytes() + a._tiles.tobytes() + a._m2.tobytes()
    hdr, img = ck.read_checkpoint_file(path)
    assert hdr["version"] == 2 and hdr["frame_index"] == 3 and img.tobytes() == a.Result.tobytes()
    b = _Tracer(frame=0, live=False)
    got = ck.load_checkpoint(path, b)
    assert got["version"] == 2 and [c[0] for c in b.calls] == ["RestoreAdaptive", "SetAdaptive"]
    _, image, frame, tiles, m2 = b.calls[0]
    assert frame == 3 and image.tobytes() == a.Result.tobytes() and tiles.tobytes() == a._tiles.tobytes() and m2.tobytes() == a._m2.tobytes()
    assert tiles.shape == (2, 2) and m2.shape == (9, 11)
    assert b.calls[1][1:] == (float(F32(3e-5)), 5, 77)
    # geometry and strict parameter checks as for version 1, before the tracer is touched
    wrong = _Tracer(w=12, live=False)
    with pytest.raises(ck.CheckpointError, match="width"):
        ck.load_checkpoint(path, wrong)
    other = _Tracer(live=False)
    other.RayDepth = 13
    with pytest.raises(ck.CheckpointError, match="ray_depth"):
        ck.load_checkpoint(path, other)
    assert not wrong.calls and not other.calls
    assert ck.load_checkpoint(path, other, strict=False)["ray_depth"] == 8 and other.calls[0][0] == "RestoreAdaptive"


def test_checkpoint_v1_is_unchanged(tmp_path):
    ck = pkg.checkpoint
    old = str(tmp_path / "old.ptck")
    src = _Tracer()
    open(old, "wb").write(_v1_bytes(src))  # a file as the writer before version 2 left it
    b = _Tracer(frame=0, live=True)
    hdr = ck.load_checkpoint(old, b)
    assert hdr["frame_index"] == 3 and [c[0] for c in b.calls] == ["WriteResult"] and b.calls[0][2] == 3
    assert b.calls[0][1].tobytes() == src.Result.tobytes()
    # without a live state the writer's bytes are version 1's, with and without the attribute
    for t in (_Tracer(), _Tracer(live=False)):
        path = str(tmp_path / "new.ptck")
        ck.save_checkpoint(path, t)
        assert open(path, "rb").read() == _v1_bytes(t)


def test_checkpoint_v2_refuses_damaged_files_before_the_tracer_is_touched(tmp_path):
    ck = pkg.checkpoint
    a = _Tracer(live=True)
    path = str(tmp_path / "a.ptck")
    ck.save_checkpoint(path, a)
    raw = open(path, "rb").read()

    def patched(offset, fmt, *values):
        return raw[:offset] + struct.pack(fmt, *values) + raw[offset + struct.calcsize(fmt):]

    bad_record = bytearray(raw)
    first = 76 + 9 * 11 * 16
    bad = {
        "truncated header": (raw[:40], "truncated"),
        "truncated adaptive header": (raw[:70], "truncated"),
        "wrong magic": (b"PTCKPT3\0" + raw[8:], "magic"),
        "tiles_y": (patched(68, "<i", 3), "tile grid"),
        "tiles_x": (patched(72, "<i", 1), "tile grid"),
        "short payload": (raw[:-4], "payload"),
        "long payload": (raw + bytes(16), "payload"),
        "no M2": (raw[:-9 * 11 * 4], "payload"),
        "min_samples": (patched(60, "<i", 1), "adaptive parameters"),
        "max below min": (patched(64, "<i", 4), "adaptive parameters"),
        "threshold": (patched(56, "<f", float("nan")), "adaptive parameters"),
        "record n": (bytes(bad_record[:first + 12]) + struct.pack("<i", 63) + bytes(bad_record[first + 16:]), "tile records"),
        "record k0": (bytes(bad_record[:first + 4]) + struct.pack("<i", 2) + bytes(bad_record[first + 8:]), "tile records"),
        "record k": (bytes(bad_record[:first]) + struct.pack("<i", 2) + bytes(bad_record[first + 4:]), "tile records"),
        "record k large": (bytes(bad_record[:first]) + struct.pack("<i", 65536) + bytes(bad_record[first + 4:]), "tile records"),
    }
    for what, (data, match) in bad.items():
        p = str(tmp_path / "bad.ptck")
        open(p, "wb").write(data)
        b = _Tracer(frame=0, live=False)
        with pytest.raises(ck.CheckpointError, match=match):
            ck.load_checkpoint(p, b)
        assert not b.calls, what
