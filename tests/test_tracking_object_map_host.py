"""The host's object map (csrc/pt_object_map.hpp, what pt_denoise_render builds for pt_denoise_set_object_tracking) without a GPU: the
header compiled on its own with g++ and compared, byte for byte, with the numpy restatement (tests/denoise_tracking_reference.py) on
the classification table of tests/test_denoise_tracking_cpu.py — degenerate geometry, which no GPU test of the denoiser renders, included
(the integrator's own degenerate scenes: tests/degenerate_cases.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import denoise_tracking_reference as dk
import first_hit_cases as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opentk-pathtracer_amd", "csrc")
F = np.float32


@pytest.fixture(scope="module")
def host_map(tmp_path_factory):
    d = tmp_path_factory.mktemp("object_map")
    src = d / "object_map.cpp"
    src.write_text('#include "pt_object_map.hpp"\n'
                   'extern "C" int object_map(const unsigned char *h, int hs, int hc, const unsigned char *c, int ns, int nc, unsigned char *map)\n'
                   "{\n    return ptmap::build(h, hs, hc, c, ns, nc, map) ? 1 : 0;\n}\n")
    so = d / "object_map.so"
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lib = C.CDLL(str(so))
    lib.object_map.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    lib.object_map.restype = C.c_int

    def build(h, hs, hc, c, ns, nc):
        out = np.full(dk.ENTRIES, 0x55, dtype=np.uint8).repeat(32).view(dk.MAP_DTYPE).copy()
        tracked = lib.object_map(h, hs, hc, c, ns, nc, out.ctypes.data_as(C.c_void_p))
        return out, bool(tracked)
    return build


def scene():
    blob, ns, nc, _ = fh.inputs(fh.BY_NAME["full_64x36"])  # all 320 slots in use
    return bytes(blob), ns, nc


def patched(blob, offset, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, *values)
    return bytes(b)


def agree(host_map, h, hs, hc, c, ns, nc):
    got, tracked = host_map(h, hs, hc, c, ns, nc)
    want = dk.object_map(h, hs, hc, c, ns, nc)
    assert tracked == want.tracked
    assert (got["state"] == want.states).all(), np.argwhere(got["state"] != want.states)[:8].tolist()
    assert got.tobytes() == want.table.tobytes()
    return want


def test_identical_moved_resized_recoloured_and_padded(host_map):
    blob, ns, nc = scene()
    assert (ns, nc) == (256, 64)
    assert not agree(host_map, blob, ns, nc, blob, ns, nc).tracked
    cur = patched(blob, 80 * 194, "<4f", -12.25, 5.5, -6.75, 0.6)                    # a sphere moved
    cur = patched(cur, 80 * 7 + 12, "<f", 0.75)                                       # a radius changed
    cur = patched(cur, 80 * 9 + 16 + 4 * 5, "<f", 0.123)                              # one material float
    at = 20480 + 96 * 49
    mn, mx = np.frombuffer(blob, F, 3, at), np.frombuffer(blob, F, 3, at + 16)
    d = np.array([0.3, 0.0, -0.7], F)
    mx2 = mx + d
    mx2[0] = np.nextafter(mx2[0], F(np.inf))
    cur = patched(patched(cur, at, "<3f", *(mn + d)), at + 16, "<3f", *mx2)           # a cuboid moved, one extent an ulp off
    cur = patched(patched(cur, 20480 + 96 * 3 + 12, "<I", 0xdeadbeef), 20480 + 96 * 3 + 28, "<f", float("nan"))  # pad words
    want = agree(host_map, blob, ns, nc, cur, ns, nc)
    assert want.tracked and [int(want.states[k]) for k in (194, 7, 9, 256 + 49, 256 + 3)] == [dk.MOVED, dk.MOVED, dk.DROP, dk.MOVED, dk.KEEP]
    agree(host_map, cur, ns, nc, blob, ns, nc)


@pytest.mark.parametrize("counts", [((256, 64), (255, 64)), ((255, 64), (256, 64)), ((48, 7), (48, 5)), ((0, 0), (0, 0)), ((0, 0), (256, 64))])
def test_counts(host_map, counts):
    blob, _, _ = scene()
    agree(host_map, blob, *counts[0], blob, *counts[1])


@pytest.mark.parametrize("bad", [0.0, -0.0, -1.3, float("nan"), float("inf"), float("-inf"), 1e-45, 3.4028235e38])
def test_degenerate_geometry(host_map, bad):
    blob, ns, nc = scene()
    at = 20480 + 96 * 6
    for cur in (patched(blob, 80 * 4 + 12, "<f", bad),        # a radius
                patched(blob, 80 * 4 + 4, "<f", bad),         # a centre coordinate
                patched(blob, at + 16 + 4, "<f", bad),        # a cuboid's max.y
                patched(blob, at, "<f", bad)):                # a cuboid's min.x
        for h, c in ((blob, cur), (cur, blob), (cur, cur)):
            agree(host_map, h, ns, nc, c, ns, nc)
    if bad != bad or bad <= 0.0 or bad == float("inf"):
        cur = patched(blob, 80 * 4 + 12, "<f", bad)
        assert dk.object_map(blob, ns, nc, cur, ns, nc).states[4] == dk.DROP


def test_a_map_beyond_binary32_drops(host_map):
    blob, ns, nc = scene()
    hist = patched(blob, 80 * 4, "<4f", 3e38, 0.0, 0.0, 1.0)
    cur = patched(blob, 80 * 4, "<4f", -3e38, 0.0, 0.0, 1.0)       # b = 6e38: finite in double, not in binary32
    assert agree(host_map, hist, ns, nc, cur, ns, nc).states[4] == dk.DROP
    hist = patched(blob, 80 * 4 + 12, "<f", 3e38)
    cur = patched(blob, 80 * 4 + 12, "<f", 1e-3)                     # a = 3e41
    assert agree(host_map, hist, ns, nc, cur, ns, nc).states[4] == dk.DROP
    assert agree(host_map, cur, ns, nc, hist, ns, nc).states[4] == dk.MOVED  # (a = 3.3e-42: a denormal, finite)
