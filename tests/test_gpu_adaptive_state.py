"""A live adaptive state saved, restored and ended on the GPU (pt_adaptive_read_m2 / pt_adaptive_write_state / pt_adaptive_end;
pt_adaptive_rebuild_kernel in csrc/pt_adaptive_state.hip).  Every comparison is byte equality: a handle that was
given another's state shows the same image, records (err included), e and M2, and stays equal to it — and to the restatement of
tests/adaptive_reference.py — through the passes that follow; the rebuild alone against tests/adaptive_state_reference.py on adversarial
M2; a refused call touches nothing; an ended state is the image of kmax pt_render frames with pt_render accepted again; checkpoints of
a live state continue bit for bit; the cost of a restore is printed."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import pytest

import adaptive_reference as ar
import adaptive_state_reference as asr
import first_hit_cases as fh

pytestmark = pytest.mark.gpu
pkg = fh.pkg
N = pkg.native
F32 = np.float32
K, MIN, MAX = 24, 4, 24
SAVE, END = 9, 26  # passes at the save point and at the end


@dataclass(frozen=True)
class SCase:
    name: str
    case: fh.Case
    F: int = 0
    spp: int = 1
    tiling: tuple = ()


def _d(w, h, ap=0.14):
    return fh.Case(f"default_{w}x{h}_ap{ap}", "default", w, h, aperture=ap)


CASES = [
    SCase("43x27_F0", _d(43, 27), 0),
    SCase("43x27_F5", _d(43, 27), 5),
    SCase("43x27_F0_ap0", _d(43, 27, 0.0), 0),
    SCase("43x27_F5_spp3", _d(43, 27), 5, spp=3),
    SCase("43x27_F0_tile_8_16", _d(43, 27), 0, tiling=("tile", 8, 16)),
    SCase("43x27_F5_tile_8_16", _d(43, 27), 5, tiling=("tile", 8, 16)),
    SCase("43x27_F0_interleaved_1_2_8", _d(43, 27), 0, tiling=("interleaved", 1, 2, 8)),
    SCase("16x16_F0", _d(16, 16), 0),
    SCase("16x16_F5", _d(16, 16), 5),
    SCase("8x8_F0", _d(8, 8), 0),
    SCase("1x1_F5", _d(1, 1), 5),
]
BY = {c.name: c for c in CASES}
ONE_TILE = ("8x8_F0", "1x1_F5")  # exempt from the non-vacuity condition

_env = None
_uniform = {}
_runs = {}


def env():
    global _env
    if _env is None:
        _env = pkg.envmap.synthetic_sky_rgba32f(32)
    return _env


def tracer(sc, tiled=True, with_env=True):
    pt = fh.make_tracer(sc.case, env=env() if with_env else None, ray_depth=8)
    if sc.spp != 1:
        pt.SPP = sc.spp
    if tiled and sc.tiling:
        if sc.tiling[0] == "tile":
            pt.SetTile(*sc.tiling[1:])
        else:
            pt.SetInterleavedTile(*sc.tiling[1:])
    return pt


def local_rows(sc):
    h = sc.case.height
    if not sc.tiling:
        return list(range(h))
    if sc.tiling[0] == "tile":
        return list(range(sc.tiling[1], sc.tiling[1] + sc.tiling[2]))
    rank, world, band = sc.tiling[1:]
    return [y for y in range(h) if (y // band) % world == rank]


def uniform(sc):
    """U_0 .. U_K of the whole image: read back after each of K pt_render frames on a handle of its own.  Made once, never changed."""
    key = (sc.case, sc.spp)
    if key not in _uniform:
        pt = tracer(sc, tiled=False)
        U = [pt.Result.copy()]
        for _ in range(K):
            pt.Render()
            U.append(pt.Result.copy())
        pt.Dispose()
        U = np.stack(U)
        U.setflags(write=False)
        _uniform[key] = U
    return _uniform[key]


def table(sc):
    U = uniform(sc)[:, local_rows(sc)]
    t = ar.tabulate(U, sc.F)
    return U, t, ar.median_threshold(t, 8)


def look(pt):
    return dict(image=pt.Result.copy(), tiles=pt.AdaptiveTiles(), e=pt.AdaptiveNoise(), m2=pt.AdaptiveM2(), status=pt.AdaptiveStatus(),
                frame=pt.FrameIndex)


def want(sim, U, thr, spp):
    m2, e = sim.stats()
    return dict(image=sim.image(U), tiles=sim.records(), e=e, m2=m2, status=sim.status(thr, MIN, MAX, spp), frame=sim.t.F)


def assert_same(got, exp, what):
    """every read-out byte for byte (the records with their err; NaN payloads included)"""
    for f in ("image", "tiles", "e", "m2"):
        assert got[f].shape == exp[f].shape and got[f].tobytes() == exp[f].tobytes(), (what, f)
    assert got["status"] == exp["status"] and got["frame"] == exp["frame"], (what, got["status"], exp["status"], got["frame"], exp["frame"])


def assert_look(got, exp, what):
    """against the restatement (whose records are built field by field)"""
    for f in ("image", "e", "m2"):
        assert got[f].tobytes() == np.ascontiguousarray(exp[f], F32).tobytes(), (what, f)
    for f in ("k", "k0", "n"):
        assert (got["tiles"][f] == exp["tiles"][f]).all(), (what, f)
    assert got["tiles"]["err"].tobytes() == np.ascontiguousarray(exp["tiles"]["err"], F32).tobytes(), (what, "err")
    assert got["status"] == exp["status"] and got["frame"] == exp["frame"], (what, got["status"], exp["status"])


def start(sc, thr, passes):
    """a handle with F pt_render frames and `passes` adaptive passes"""
    pt = tracer(sc)
    for _ in range(sc.F):
        pt.Render()
    pt.SetAdaptive(float(thr), MIN, MAX)
    if passes:
        pt.RenderAdaptive(passes)
    return pt


def run(sc):
    """Handle A: F frames, 9 passes, its state read; a fresh handle B given that state; 17 more passes on both.  The restatement beside
    them.  The non-vacuity condition is asserted on the expected counts before the sampler runs."""
    if sc.name in _runs:
        return _runs[sc.name]
    U, t, thr = table(sc)
    sim = ar.Sim(t).run(SAVE, thr, MIN, MAX)
    exp = {SAVE: want(sim, U, thr, sc.spp)}
    save_counts, save_active = sim.k.copy(), int(sim.active(thr, MIN, MAX).sum())
    exp[END] = want(sim.run(END - SAVE, thr, MIN, MAX), U, thr, sc.spp)
    if sc.name not in ONE_TILE:
        assert len(np.unique(save_counts)) >= 3 and save_active >= 1, (np.unique(save_counts), save_active)
        assert ar.non_vacuous(sim.k, MIN, MAX), np.unique(sim.k)
    a = start(sc, thr, SAVE)
    assert a.rows == U.shape[1]
    got_a = {SAVE: look(a)}
    state = a.AdaptiveState()
    debug_m2 = N.debug_adaptive_m2(a._h, a.rows, a.Width)
    b = tracer(sc)
    live_before = b.AdaptiveLive
    b.RestoreAdaptive(state["image"], state["frame_index"], state["tiles"], state["m2"])
    live_after = b.AdaptiveLive
    b.SetAdaptive(float(thr), MIN, MAX)
    got_b = {SAVE: look(b)}
    a.RenderAdaptive(END - SAVE)
    b.RenderAdaptive(END - SAVE)
    got_a[END], got_b[END] = look(a), look(b)
    a.Dispose()
    b.Dispose()
    _runs[sc.name] = dict(a=got_a, b=got_b, exp=exp, state=state, debug_m2=debug_m2, live=(live_before, live_after), thr=thr, U=U, table=t)
    return _runs[sc.name]


NAMES = [c.name for c in CASES]


@pytest.mark.parametrize("name", NAMES)
def test_a_restored_state_equals_the_saved_one(name):
    r = run(BY[name])
    assert r["live"] == (False, True)
    assert r["state"]["frame_index"] == BY[name].F and r["state"]["m2"].tobytes() == r["debug_m2"].tobytes()
    assert_same(r["b"][SAVE], r["a"][SAVE], f"{name} at the save point")
    assert_look(r["a"][SAVE], r["exp"][SAVE], f"{name}: the saved handle against the restatement")
    assert (r["b"][SAVE]["image"][..., 3] == 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_a_restored_state_continues_bit_for_bit(name):
    r = run(BY[name])
    assert_same(r["b"][END], r["a"][END], f"{name} after {END} passes")
    assert_look(r["b"][END], r["exp"][END], f"{name}: the restored handle against the restatement")
    if name not in ONE_TILE:
        assert r["a"][END]["tiles"].tobytes() != r["a"][SAVE]["tiles"].tobytes()  # (the 17 passes did something)


# ------------------------------------------------------------------------------------------------ the rebuild alone
def _adversarial(rows, width, F, seed):
    """an image with ordinary, huge, negative, l = -1 and non-finite colours; M2 with NaN, +-inf, negatives, subnormals, FLT_MAX; records at
    k = F and k > F with garbage in err"""
    rng = np.random.default_rng(seed)
    image = np.exp(rng.uniform(-6, 3, (rows, width, 4))).astype(F32)
    image[..., 3] = 7.0  # (forced to 1 by the call)
    special = [asr.colour_with_luminance_minus_one(), np.array([np.inf, 0, 0, 1], F32), np.array([0, -np.inf, 0, 1], F32),
               np.array([np.nan, 1, 1, 1], F32), np.array([ar.FLT_MAX] * 4, F32), np.array([-0.5, -0.25, -3.0, 1], F32), np.zeros(4, F32)]
    m2 = np.exp(rng.uniform(-20, 10, (rows, width))).astype(F32)
    values = [np.nan, np.inf, -np.inf, -3.0, 1e-45, -1e-45, 1e-39, float(ar.FLT_MAX), -float(ar.FLT_MAX), 0.0, -0.0]
    flat_i, flat_m = image.reshape(-1, 4), m2.reshape(-1)
    n = flat_m.size
    for i in range(min(n, 400)):
        p = int(rng.integers(n))
        if i % 2:
            flat_i[p] = special[(i // 2) % len(special)]
        flat_m[p] = F32(values[i % len(values)]) if i % 3 else flat_m[p]
    if n == 1:
        flat_m[0] = F32(np.inf)
    ty, tx = ar.tile_grid(rows, width)
    tiles = np.empty((ty, tx), ar.TILE_DTYPE)
    k = F + rng.integers(0, 9, (ty, tx))
    k.flat[0] = F                      # a tile no pass has touched ...
    k.flat[-1] = 65535 if n > 1 else F + 3  # ... and the largest count there is
    tiles["k"], tiles["k0"], tiles["n"] = k, max(F, 1), ar.tile_pixels(rows, width)
    tiles["err"] = np.frombuffer(rng.integers(0, 2 ** 32, ty * tx, dtype=np.uint64).astype(np.uint32).tobytes(), F32).reshape(ty, tx)
    return image, tiles, m2


@pytest.mark.parametrize("size", [(43, 27), (1, 1)])
@pytest.mark.parametrize("F", (0, 5))
def test_rebuild_alone_equals_the_restatement(size, F):
    width, rows = size
    sc = SCase("rebuild", _d(width, rows))
    image, tiles, m2 = _adversarial(rows, width, F, 100 * width + F)
    pt = tracer(sc, with_env=False)  # (needs neither an environment nor a frame)
    pt.RestoreAdaptive(image, F, tiles, m2)
    got = look(pt)
    pt.Dispose()
    stored = image.copy()
    stored[..., 3] = 1.0
    with np.errstate(all="ignore"):
        e, err = asr.rebuild(stored, m2, tiles["k"], max(F, 1))
    assert got["image"].tobytes() == stored.tobytes() and got["frame"] == F
    assert got["m2"].tobytes() == m2.tobytes()  # as bits: NaN payloads, -0, subnormals
    assert got["e"].tobytes() == e.tobytes()
    assert not np.isnan(got["e"]).any() and not np.signbit(got["e"]).any()
    for f in ("k", "k0", "n"):
        assert (got["tiles"][f] == tiles[f]).all(), f
    assert got["tiles"]["err"].tobytes() == err.tobytes()
    fresh = tiles["k"] - tiles["k0"] < 1  # no statistics yet: e = 0, err = +0 whatever M2 holds
    assert not got["tiles"]["err"][fresh].view(np.uint32).any()
    assert not got["e"][asr.pixel_counts(fresh, rows, width)].view(np.uint32).any()
    assert (width, rows) == (1, 1) or (fresh.any() and np.isinf(got["tiles"]["err"]).any() and (got["tiles"]["err"] > 0).sum() > 3)


# ------------------------------------------------------------------------------------------------ refusals
def test_a_refused_write_touches_nothing():
    sc = BY["43x27_F5"]
    U, t, thr = table(sc)
    pt = start(sc, thr, 6)
    before = look(pt)
    state = pt.AdaptiveState()
    L, h = pt._lib, pt._h
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    img, m2 = np.ascontiguousarray(U[7]), state["m2"].copy()  # (another image: a call that got through would show)
    m2[:] = 1.0

    def write(image=img, ipitch=0, frame=5, tiles=state["tiles"], sums=m2, mpitch=0):
        return L.pt_adaptive_write_state(h, None if image is None else image.ctypes.data_as(fp), ipitch, frame,
                                         None if tiles is None else tiles.ctypes.data_as(vp), None if sums is None else sums.ctypes.data_as(fp), mpitch)

    def edited(field, value, at=(0, 0)):
        rec = state["tiles"].copy()
        rec[field][at] = value
        return rec

    bad, oor = N.PT_E_BAD_ARGUMENT, N.PT_E_OUT_OF_RANGE
    assert write(image=None) == bad and write(tiles=None) == bad and write(sums=None) == bad
    assert write(ipitch=43 * 16 - 1) == bad and write(mpitch=43 * 4 - 1) == bad and write(ipitch=1) == bad
    assert write(frame=-1) == bad
    assert write(tiles=edited("n", 63)) == oor and write(tiles=edited("n", 24, (3, 5))) == oor  # (the corner tile holds 3 x 3 = 9)
    assert write(tiles=edited("k0", 4)) == oor and write(tiles=edited("k0", 1, (2, 2))) == oor
    assert write(tiles=edited("k", 4)) == oor and write(tiles=edited("k", 65536, (1, 1))) == oor and write(tiles=edited("k", -1)) == oor
    assert write(frame=4) == oor and write(frame=6) == oor  # (k0 = max(frame_index, 1) no longer holds)
    after = look(pt)
    assert_same(after, before, "after the refused calls")
    pt.RenderAdaptive(1)
    sim = ar.Sim(t).run(7, thr, MIN, MAX)
    assert_look(look(pt), want(sim, U, thr, 1), "a pass after the refused calls")
    # pt_adaptive_read_m2: the refusals of pt_adaptive_read_noise
    buf = np.full((27, 45), -1.0, F32)
    assert L.pt_adaptive_read_m2(h, None, 0) == bad and L.pt_adaptive_read_m2(h, buf.ctypes.data_as(fp), 43 * 4 - 1) == bad
    assert L.pt_adaptive_read_m2(h, buf.ctypes.data_as(fp), 45 * 4) == N.PT_OK
    assert (buf[:, 43:] == -1).all() and buf[:, :43].tobytes() == pt.AdaptiveM2().tobytes()
    # a pitched write reads the rows where the pitches say
    wide_i, wide_m = np.full((27, 44, 4), 9.0, F32), np.full((27, 47), 9.0, F32)
    wide_i[:, :43], wide_m[:, :43] = img, state["m2"]
    assert write(image=wide_i, ipitch=44 * 16, sums=wide_m, mpitch=47 * 4) == N.PT_OK
    got = look(pt)
    assert got["image"].tobytes() == img.tobytes() and got["m2"].tobytes() == state["m2"].tobytes() and got["frame"] == 5
    pt.Dispose()
    # without a live state: the image and the frame index stay, and no state appears
    pt = tracer(sc)
    for _ in range(3):
        pt.Render()
    L, h = pt._lib, pt._h
    assert L.pt_adaptive_read_m2(h, buf.ctypes.data_as(fp), 45 * 4) == bad and L.pt_adaptive_end(h, None) == bad
    assert write(frame=-1) == bad and write(tiles=edited("n", 1)) == oor
    assert not pt.AdaptiveLive and pt.FrameIndex == 3 and pt.Result.tobytes() == uniform(sc)[3].tobytes()
    pt.Render()
    assert pt.Result.tobytes() == uniform(sc)[4].tobytes()
    pt.Dispose()


def test_a_group_handle_is_refused():
    group = fh.make_tracer(_d(43, 27), devices=[0, 0])
    L, h = group._lib, group._h
    fp = C.POINTER(C.c_float)
    img, m2 = np.zeros((27, 43, 4), F32), np.zeros((27, 43), F32)
    tiles = np.zeros((4, 6), ar.TILE_DTYPE)
    tiles["k0"], tiles["n"] = 1, ar.tile_pixels(27, 43)
    out = C.c_int(-7)
    assert L.pt_adaptive_read_m2(h, m2.ctypes.data_as(fp), 0) == N.PT_E_BAD_ARGUMENT
    assert L.pt_adaptive_write_state(h, img.ctypes.data_as(fp), 0, 0, tiles.ctypes.data_as(C.c_void_p), m2.ctypes.data_as(fp), 0) == N.PT_E_BAD_ARGUMENT
    assert L.pt_adaptive_end(h, C.byref(out)) == N.PT_E_BAD_ARGUMENT and out.value == -7
    assert not group.AdaptiveLive
    group.Dispose()


# ------------------------------------------------------------------------------------------------ pt_adaptive_end
@pytest.mark.parametrize("name,passes", [("43x27_F0", SAVE), ("43x27_F5", END), ("43x27_F0_tile_8_16", SAVE)])
def test_end_levels_to_the_uniform_image(name, passes):
    sc = BY[name]
    U, t, thr = table(sc)
    sim = ar.Sim(t).run(passes, thr, MIN, MAX)
    kmax = int(sim.k.max())
    assert int(sim.k.min()) < kmax
    pt = start(sc, thr, passes)
    params = pt.AdaptiveParams
    assert pt.EndAdaptive() == kmax
    assert pt.FrameIndex == kmax and not pt.AdaptiveLive
    assert pt._lib.pt_adaptive_status(pt._h, None, None, None, None, None) == N.PT_E_BAD_ARGUMENT
    assert pt._lib.pt_adaptive_end(pt._h, None) == N.PT_E_BAD_ARGUMENT  # a second end
    twin = tracer(sc)
    for _ in range(kmax):
        twin.Render()
    image = pt.Result
    assert image.tobytes() == twin.Result.tobytes() and image.tobytes() == U[kmax].tobytes()
    assert pt.Render() == twin.Render() == (kmax + 1) * sc.spp
    assert pt.Result.tobytes() == twin.Result.tobytes() and pt.FrameIndex == kmax + 1
    # the temporal stage is accepted again; the host's parameters were neither read nor changed: a new state runs under them
    if not sc.tiling:  # (the denoiser needs a handle that owns the whole image)
        pt.SetDenoiseTemporal(True)
        assert pt._lib.pt_denoise_render(pt._h, 0) == N.PT_OK
        pt.SetDenoiseMoments(True)
        assert pt._lib.pt_denoise_render(pt._h, 0) == N.PT_OK
        pt.SetDenoiseMoments(False)
        pt.SetDenoiseTemporal(False)
    assert pt.AdaptiveParams == params
    pt.RenderAdaptive(1)
    st = pt.AdaptiveStatus()
    assert st["min_count"] == st["max_count"] == kmax + 1 + (kmax + 1 < MAX) and pt.AdaptiveLive
    pt.Dispose()
    twin.Dispose()


@pytest.mark.parametrize("F", (0, 5))
def test_end_of_a_state_that_never_diverged_launches_nothing(F):
    sc = BY[f"43x27_F{F}"]
    U = uniform(sc)
    ty, tx = ar.tile_grid(27, 43)
    tiles = np.zeros((ty, tx), ar.TILE_DTYPE)
    tiles["k"], tiles["k0"], tiles["n"] = F, max(F, 1), ar.tile_pixels(27, 43)
    pt = tracer(sc, with_env=False)  # (no environment: a pass would be refused, and none is needed)
    pt.RestoreAdaptive(U[F], F, tiles, np.zeros((27, 43), F32))
    assert pt.AdaptiveLive and pt.AdaptiveStatus()["max_count"] == F
    out = C.c_int(-7)
    assert pt._lib.pt_adaptive_end(pt._h, C.byref(out)) == N.PT_OK and out.value == F
    stored = U[F].copy()
    stored[..., 3] = 1.0  # (U_0 is the zero image a fresh handle holds; a written image has alpha 1)
    assert pt.FrameIndex == F and not pt.AdaptiveLive and pt.Result.tobytes() == stored.tobytes()
    assert pt._lib.pt_adaptive_end(pt._h, None) == N.PT_E_BAD_ARGUMENT
    # a diverged state on the same handle needs passes, and they need an environment: refused, nothing touched
    tiles["k"][1, 2] = F + 2
    pt.RestoreAdaptive(U[F], F, tiles, np.zeros((27, 43), F32))
    before = look(pt)
    assert pt._lib.pt_adaptive_end(pt._h, C.byref(out)) == N.PT_E_NO_ENVIRONMENT and out.value == F
    assert_same(look(pt), before, "after the refused end")
    pt.EnvironmentMap = env()
    assert pt.EndAdaptive() == F + 2 and pt.FrameIndex == F + 2
    pt.Dispose()
    # with an environment: pt_render goes on from F
    pt = tracer(sc)
    tiles["k"][1, 2] = F
    pt.RestoreAdaptive(U[F], F, tiles, np.zeros((27, 43), F32))
    assert pt.EndAdaptive() == F
    pt.Render()
    assert pt.Result.tobytes() == U[F + 1].tobytes()
    pt.Dispose()


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_of_a_live_state_continues_bit_for_bit(tmp_path):
    sc = BY["43x27_F5"]
    r = run(sc)
    a = start(sc, r["thr"], SAVE)
    path = str(tmp_path / "live.ptck")
    a.SaveCheckpoint(path)
    assert open(path, "rb").read(8) == b"PTCKPT2\0"
    assert os.path.getsize(path) == 56 + 20 + 27 * 43 * 16 + 24 * 16 + 27 * 43 * 4
    a.Dispose()
    c = tracer(sc)
    hdr = c.LoadCheckpoint(path)
    assert hdr["version"] == 2 and hdr["frame_index"] == 5 and c.AdaptiveLive
    assert c.AdaptiveParams == (float(r["thr"]), MIN, MAX)
    assert_same(look(c), r["a"][SAVE], "loaded from the checkpoint")
    c.RenderAdaptive(END - SAVE)
    got = look(c)
    c.Dispose()
    assert_same(got, r["a"][END], "continued from the checkpoint")  # the uninterrupted handle: image, records, e, M2
    # a damaged record is refused before the tracer is touched
    raw = bytearray(open(path, "rb").read())
    raw[76 + 27 * 43 * 16 + 12:76 + 27 * 43 * 16 + 16] = (63).to_bytes(4, "little")
    open(path, "wb").write(bytes(raw))
    d = tracer(sc)
    with pytest.raises(pkg.checkpoint.CheckpointError):
        d.LoadCheckpoint(path)
    assert not d.AdaptiveLive and d.FrameIndex == 0
    d.Dispose()


def test_checkpoint_without_a_live_state_is_version_1():
    import tempfile
    sc = BY["43x27_F5"]
    U = uniform(sc)
    a = tracer(sc)
    for _ in range(5):
        a.Render()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "plain.ptck")
        a.SaveCheckpoint(path)
        raw = open(path, "rb").read()
        assert raw[:8] == b"PTCKPT1\0" and len(raw) == 56 + 27 * 43 * 16 and raw[56:] == U[5].tobytes()
        b = tracer(sc)
        hdr = b.LoadCheckpoint(path)
        # ... and an ended state is a plain image again
        a.SetAdaptive(1e-4, MIN, MAX)
        a.RenderAdaptive(2)
        assert a.EndAdaptive() == 7
        a.SaveCheckpoint(path)
        ended, image = pkg.checkpoint.read_checkpoint_file(path)
        assert ended["version"] == 1 and ended["frame_index"] == 7 and image.tobytes() == U[7].tobytes()
    assert hdr["version"] == 1 and hdr["frame_index"] == 5 and not b.AdaptiveLive and b.FrameIndex == 5
    b.Render()
    assert b.Result.tobytes() == U[6].tobytes()
    assert a.Result.tobytes() == U[7].tobytes()
    a.Dispose()
    b.Dispose()


# ------------------------------------------------------------------------------------------------ cost
def test_the_cost_of_a_restore_is_recorded():
    """1920x1080: pt_adaptive_write_state (the uploads of 16 + 8 B per pixel from pageable memory, alpha, the rebuild kernel) beside a
    pt_write_result of the same image on the same handle; pt_timer_*, fastest of three.  Printed, recorded in DESIGN.md 3.5; nothing
    is asserted about the figures."""
    big = fh.Case("default_1080p_ap0", "default", 1920, 1080, aperture=0.0)
    pt = fh.make_tracer(big, env=env(), ray_depth=8)
    pt.Render()
    pt.Render()
    pt.SetAdaptive(0.0, 65535, 65535)
    pt.RenderAdaptive(2)
    state = pt.AdaptiveState()

    def fastest(fn):
        ms = []
        for _ in range(3):
            pt.Synchronize()
            pt.TimerBegin()
            fn()
            ms.append(pt.TimerEnd())
        return min(ms)
    restore = fastest(lambda: pt.RestoreAdaptive(state["image"], state["frame_index"], state["tiles"], state["m2"]))
    again = look(pt)
    plain = fastest(lambda: pt.WriteResult(state["image"], state["frame_index"]))
    pt.Dispose()
    print(f"\n  adaptive state cost 1080p: pt_adaptive_write_state {restore:.4f} ms; pt_write_result of the same image {plain:.4f} ms")
    assert again["image"].tobytes() == state["image"].tobytes() and again["tiles"].tobytes() == state["tiles"].tobytes()
    assert again["m2"].tobytes() == state["m2"].tobytes()
