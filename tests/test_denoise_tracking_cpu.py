"""Object tracking of the temporal stage without a GPU: the properties of the numpy restatement (tests/denoise_tracking_reference.py)
that tests/test_gpu_denoise_tracking.py compares the kernel and the host's object map with."""
import struct

import numpy as np
import pytest

import denoise_reference as dr
import denoise_temporal_reference as dt
import denoise_tracking_reference as dk
import first_hit_cases as fh

H, W = 23, 40
F = np.float32
KEEP, MOVED, DROP = dk.KEEP, dk.MOVED, dk.DROP


# ------------------------------------------------------------------------------------------------ the tracked kernel's restatement
def plane_guides(ids=None):
    """A plane z = 0 seen head-on from z = 10: pos = (x, y, 0) / 10, normal +z, t = 10 (as test_denoise_temporal_cpu.py builds its own)."""
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    yy, xx = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    g["pos"][..., 0], g["pos"][..., 1] = xx * F(0.1), yy * F(0.1)
    g["normal"][:] = np.asarray((0.0, 0.0, 1.0), F)
    g["t"] = F(10.0)
    g["id"] = 0 if ids is None else ids
    return g


def plane_camera():
    """The camera that sees plane_guides: pixel (x, y)'s centre on the plane point (x, y, 0) / 10."""
    return np.diag([20.0 / W, 20.0 / H, -0.1]).astype(F), np.array([(W - 1) / 20.0, (H - 1) / 20.0, 10.0], F)


def noise(seed=0):
    c = np.ones((H, W, 4), F)
    c[..., :3] = np.random.default_rng(seed).uniform(0.2, 0.8, (H, W, 3)).astype(F)
    return c


def history(count=8.0, seed=9):
    h = noise(seed)
    h[..., 3] = F(count)
    return h


def passthrough(c, n):
    out = c.copy()
    out[..., 3] = F(n)
    return out


def table_of(**entries):
    t = dk.keep_table()
    for k, (state, a, b) in entries.items():
        k = int(k[1:])
        t["state"][k], t["a"][k], t["b"][k] = state, a, b
    return t


def mixed_ids():
    ids = np.zeros((H, W), np.int32)
    ids[:4] = -1
    ids[4:, 28:] = 256
    ids[10:16, 5:20] = 7
    return ids


def test_an_all_keep_table_gives_the_untracked_definition_bit_for_bit():
    g, c, hist = plane_guides(mixed_ids()), noise(1), history()
    B, O = plane_camera()
    O = O + np.array([0.03, 0.04, 0.0], F)  # fractional bilinear weights
    for n, cap in ((0, 32), (2, 32), (3, 1)):
        want = dt.integrate(c, n, g, hist, g, B, O, max_history=cap)
        got = dk.integrate_tracked(c, n, g, hist, g, B, O, dk.keep_table(), cap=cap)
        assert got.tobytes() == want.tobytes()
        assert (got[..., 3] > n).any()
    # the 10,240 bytes as read back are accepted as they are
    assert dk.integrate_tracked(c, 2, g, hist, g, B, O, np.frombuffer(dk.keep_table().tobytes(), np.uint8)).tobytes() == \
        dt.integrate(c, 2, g, hist, g, B, O).tobytes()


def test_drop_and_a_miss_give_the_image_and_n_exactly():
    ids = mixed_ids()
    g, c, hist = plane_guides(ids), noise(2), history()
    B, O = plane_camera()
    t = table_of(k7=(DROP, 0.0, 0.0))
    I = dk.integrate_tracked(c, 3, g, hist, g, B, O, t)
    gone = (ids == 7) | (ids == -1)
    assert I[gone].tobytes() == passthrough(c, 3)[gone].tobytes()
    # every other pixel is what the untracked definition gives: a DROP entry touches its own id only
    assert I[~gone].tobytes() == dt.integrate(c, 3, g, hist, g, B, O)[~gone].tobytes() and (I[~gone][..., 3] > 3).all()
    # an id the map has no entry for is not looked up
    g2 = g.copy()
    g2["id"][ids == 7] = 320
    hg2 = g2.copy()
    I2 = dk.integrate_tracked(c, 3, g2, hist, hg2, B, O, dk.keep_table())
    assert I2[ids == 7].tobytes() == passthrough(c, 3)[ids == 7].tobytes()


@pytest.mark.parametrize("n", [0, 1, 5])
@pytest.mark.parametrize("cap", [1, 7, 32])
def test_count_bounds_hold_exactly(n, cap):
    ids = mixed_ids()
    g, c = plane_guides(ids), noise(3)
    hist = history()
    hist[..., 3] = np.random.default_rng(4).uniform(0.0, 100.0, (H, W)).astype(F)
    B, O = plane_camera()
    t = table_of(k0=(MOVED, 1.0, (-0.13, 0.07, 0.0)), k256=(DROP, 0.0, 0.0))
    I = dk.integrate_tracked(c, n, g, hist, g, B, O, t, cap=cap)
    count = I[..., 3]
    assert (count >= F(n)).all() and (count <= F(n) + F(cap)).all()
    assert (count[(ids == -1) | (ids == 256)] == F(n)).all()
    assert (count[ids == 0] > F(n)).mean() > 0.8 and (count[ids == 7] > F(n)).all()
    assert dk.cap_of(32, 0) == 32 and dk.cap_of(32, 5) == 5 and dk.cap_of(4, 9) == 4


def test_an_object_shifted_by_whole_pixels_finds_its_shifted_history():
    """A fronto-parallel plane of one id that carries a colour ramp along x and moved by +3 pixels (0.3 units) since the history: with the
    map (a = 1, b = -0.3: the history point of P) pixel x finds the history colour of pixel x - 3 within rounding, without the map that of
    pixel x.  n = 0: I is the history alone."""
    ids = np.full((H, W), -1, np.int32)
    ids[3:20, :] = 5
    g = plane_guides(ids)
    hist = np.zeros((H, W, 4), F)
    ramp = (np.arange(W, dtype=F) / F(64.0))
    hist[..., 0], hist[..., 1], hist[..., 2], hist[..., 3] = ramp, F(0.5), ramp * F(0.5), F(8.0)
    B, O = plane_camera()
    c = noise(5)
    t = table_of(k5=(MOVED, 1.0, (-0.3, 0.0, 0.0)))
    tracked = dk.integrate_tracked(c, 0, g, hist, g, B, O, t)
    untracked = dt.integrate(c, 0, g, hist, g, B, O)
    inner = (slice(4, 19), slice(4, W - 1))
    assert (tracked[inner][..., 3] > 0).all() and (untracked[inner][..., 3] > 0).all()
    assert np.abs(tracked[inner][..., 0] - ramp[1:W - 4]).max() < 1e-4   # the colour of x - 3
    assert np.abs(untracked[inner][..., 0] - ramp[4:W - 1]).max() < 1e-4  # the colour of x
    assert np.abs(tracked[inner][..., 0] - untracked[inner][..., 0]).min() > 3 / 64 - 1e-4
    assert np.abs(tracked[inner][..., 3] - 8.0).max() < 1e-3
    # the three leftmost columns of the object look beyond the image's edge: nothing found
    assert (tracked[4:19, :2, 3] == 0).all()


# ------------------------------------------------------------------------------------------------ the host's restatement: classification
def scene():
    blob, ns, nc, _ = fh.inputs(fh.BY_NAME["default_75x43_f0"])
    return bytes(blob), ns, nc


def patched(blob, offset, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, *values)
    return bytes(b)


def floats(blob, offset, count):
    return np.frombuffer(blob, np.float32, count, offset).copy()


def test_identical_scenes_keep_every_object_that_exists():
    blob, ns, nc = scene()
    m = dk.object_map(blob, ns, nc, blob, ns, nc)
    exists = np.zeros(dk.ENTRIES, bool)
    exists[:ns] = True
    exists[256:256 + nc] = True
    assert not m.tracked and (m.states[exists] == KEEP).all() and (m.states[~exists] == DROP).all()
    assert (m.table["a"][exists] == 1).all() and (m.table["b"] == 0).all() and (m.table["a"][~exists] == 0).all() and (m.table["zero"] == 0).all()
    assert m.table.tobytes() == dk.object_map(blob, ns, nc, blob, ns, nc).table.tobytes() and len(m.table.tobytes()) == 10240


def test_a_moved_sphere_maps_by_its_translation():
    blob, ns, nc = scene()
    p = floats(blob, 80 * 4, 4)
    cur = patched(blob, 80 * 4, "<3f", p[0] + F(0.5), p[1] - F(0.25), p[2])
    m = dk.object_map(blob, ns, nc, cur, ns, nc)
    assert m.tracked and m.states[4] == MOVED and (np.delete(m.states[:ns], 4) == KEEP).all() and (m.states[256:256 + nc] == KEEP).all()
    assert (m.table["a"][4] == 1).all() and np.allclose(m.table["b"][4], (-0.5, 0.25, 0.0), atol=1e-6)
    # the history point of the current centre is the history's centre
    assert np.allclose(m.a64[4] * floats(cur, 320, 3) + m.b64[4], p[:3], atol=1e-12)


def test_a_changed_radius_maps_by_the_ratio_about_the_centres():
    blob, ns, nc = scene()
    p = floats(blob, 80 * 9, 4)
    cur = patched(blob, 80 * 9 + 12, "<f", 2.0)
    m = dk.object_map(blob, ns, nc, cur, ns, nc)
    a = float(p[3]) / 2.0
    assert m.states[9] == MOVED and np.allclose(m.a64[9], a, rtol=1e-15) and np.allclose(m.b64[9], p[:3].astype(float) * (1 - a), rtol=1e-12)
    assert m.table["a"].dtype == np.float32 and (m.table["a"][9] == F(a)).all()
    # a surface point of the current sphere lands on the history's surface
    P = floats(cur, 720, 3).astype(float) + np.array([0.0, 2.0, 0.0])
    assert abs(np.linalg.norm(m.a64[9] * P + m.b64[9] - p[:3]) - float(p[3])) < 1e-12


def test_a_moved_cuboid_whose_extent_changed_by_one_ulp_is_moved_not_dropped():
    blob, ns, nc = scene()
    at = 20480 + 96 * 6
    mn, mx = floats(blob, at, 3), floats(blob, at + 16, 3)
    d = np.array([0.3, 0.0, -0.7], F)
    mn2, mx2 = mn + d, mx + d
    mx2[0] = np.nextafter(mx2[0], F(np.inf))
    cur = patched(patched(blob, at, "<3f", *mn2), at + 16, "<3f", *mx2)
    m = dk.object_map(blob, ns, nc, cur, ns, nc)
    k = 256 + 6
    assert m.tracked and m.states[k] == MOVED and (np.delete(m.states[256:256 + nc], 6) == KEEP).all()
    assert np.abs(m.a64[k] - 1).max() < 1e-6 and m.a64[k][0] != 1.0
    assert np.allclose(m.a64[k] * mn2 + m.b64[k], mn, atol=1e-12) and np.allclose(m.a64[k] * mx2 + m.b64[k], mx, atol=1e-5)


@pytest.mark.parametrize("kind, index", [("sphere", 4), ("cuboid", 2)])
def test_every_single_material_bit_drops_the_object_and_no_other(kind, index):
    blob, ns, nc = scene()
    at = 80 * index + 16 if kind == "sphere" else 20480 + 96 * index + 32
    k = index if kind == "sphere" else 256 + index
    for word in range(16):
        for bit in (0, 22, 31):
            b = bytearray(blob)
            b[at + 4 * word + bit // 8] ^= 1 << (bit % 8)
            for h, c in ((blob, bytes(b)), (bytes(b), blob)):
                m = dk.object_map(h, ns, nc, c, ns, nc)
                assert m.tracked and m.states[k] == DROP, (word, bit)
                assert (m.states == DROP).sum() == dk.ENTRIES - ns - nc + 1


def test_pad_bytes_are_not_compared():
    blob, ns, nc = scene()
    at = 20480 + 96 * 3
    cur = patched(patched(blob, at + 12, "<I", 0xdeadbeef), at + 28, "<f", float("nan"))
    m = dk.object_map(blob, ns, nc, cur, ns, nc)
    assert not m.tracked and m.states[259] == KEEP


def test_counts_shrunk_and_grown():
    blob, ns, nc = scene()
    for h, c in (((ns, nc), (ns - 1, nc)), ((ns - 1, nc), (ns, nc)), ((ns, nc), (ns, nc - 2)), ((ns, nc - 2), (ns, nc))):
        m = dk.object_map(blob, h[0], h[1], blob, c[0], c[1])
        lo_s, lo_c = min(h[0], c[0]), min(h[1], c[1])
        assert m.tracked
        assert (m.states[:lo_s] == KEEP).all() and (m.states[lo_s:256] == DROP).all()
        assert (m.states[256:256 + lo_c] == KEEP).all() and (m.states[256 + lo_c:] == DROP).all()
    assert not dk.object_map(blob, 0, 0, blob, 0, 0).tracked and (dk.object_map(blob, 0, 0, blob, 0, 0).states == DROP).all()


@pytest.mark.parametrize("bad", [0.0, -1.3, float("nan"), float("inf"), -0.0])
def test_a_degenerate_radius_or_extent_drops(bad):
    blob, ns, nc = scene()
    cur = patched(blob, 80 * 4 + 12, "<f", bad)
    for h, c in ((blob, cur), (cur, blob)):
        m = dk.object_map(h, ns, nc, c, ns, nc)
        assert m.states[4] == DROP and (m.table["a"][4] == 0).all() and (m.table["b"][4] == 0).all() and m.tracked
    at = 20480 + 96 * 6
    mn, mx = floats(blob, at, 3), floats(blob, at + 16, 3)
    if bad == bad and abs(bad) != float("inf"):
        cur = patched(blob, at + 16 + 4, "<f", float(mn[1] + F(bad)))  # the y extent becomes `bad` (0 and -1.3; -0: zero again)
    else:
        cur = patched(blob, at + 16 + 4, "<f", bad)                      # max.y itself NaN / inf
    for h, c in ((blob, cur), (cur, blob)):
        assert dk.object_map(h, ns, nc, c, ns, nc).states[262] == DROP
    # the same value on both sides is no edit: bit-equal geometry is KEEP whatever it holds
    assert dk.object_map(cur, ns, nc, cur, ns, nc).states[262] == KEEP and not dk.object_map(cur, ns, nc, cur, ns, nc).tracked


def test_a_map_that_overflows_binary32_drops():
    blob, ns, nc = scene()
    hist = patched(blob, 80 * 4, "<4f", 3e38, 0.0, 0.0, 1.0)
    cur = patched(blob, 80 * 4, "<4f", -3e38, 0.0, 0.0, 1.0)  # b = 6e38: finite in double, not in binary32
    assert dk.object_map(hist, ns, nc, cur, ns, nc).states[4] == DROP
