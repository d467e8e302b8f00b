"""Object tracking of the temporal stage (pt_denoise_set_object_tracking) restated in numpy:
object_map() is the host's side — the history set's scene snapshot against the scene in force, classified per guide id and, for an object
that moved or was resized, the map history point = a * P + b, formed in float64 from the binary32 fields and rounded to binary32 once;
integrate_tracked() is the tracked kernel — denoise_temporal_reference.integrate (imported, not edited) with the three differences of the
definition and no others: a pixel whose id is DROP (or no id of the map) passes through like a miss, P' = a * P + b (one binary32 product,
one binary32 sum per component) stands in for P_p of a MOVED id in the projection and in the plane term of every tap, and `cap` stands in
for max_history.  csrc/pt_denoise.hip (pt_temporal_tracked_kernel) must reproduce integrate_tracked bit for bit and
csrc/mi355pt_queries.cpp (denoise_object_map) the states exactly (tests/test_gpu_denoise_tracking.py);
tests/test_denoise_tracking_cpu.py checks the properties of the restatement itself.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import denoise_reference as dr
import denoise_temporal_reference as dt

F = dr.F
MAX_SPHERES, MAX_CUBOIDS = 256, 64
ENTRIES = MAX_SPHERES + MAX_CUBOIDS
KEEP, MOVED, DROP = 0, 1, 2
SPHERE_SIZE, CUBOID_SIZE, CUBOIDS_OFFSET, BLOB_SIZE = 80, 96, 20480, 26624
MAP_DTYPE = np.dtype([("a", np.float32, 3), ("state", np.int32), ("b", np.float32, 3), ("zero", np.int32)])
assert MAP_DTYPE.itemsize == 32


class ObjectMap(NamedTuple):
    table: np.ndarray   # (320,) MAP_DTYPE: what the kernel reads
    states: np.ndarray  # (320,) int32 = table["state"]
    a64: np.ndarray     # (320, 3) float64: a before its rounding (KEEP: 1, DROP: 0)
    b64: np.ndarray     # (320, 3) float64
    tracked: bool       # an id that exists is not KEEP, or the counts differ: the tracked kernel has to run


def entry_layout(k: int):
    """-> (byte offset of object k in the blob, bytes of geometry in front of its 64 material bytes, word indices of its geometry floats)"""
    if k < MAX_SPHERES:
        return SPHERE_SIZE * k, 16, (0, 1, 2, 3)
    return CUBOIDS_OFFSET + CUBOID_SIZE * (k - MAX_SPHERES), 32, (0, 1, 2, 4, 5, 6)  # (words 3 and 7: std140 pad, not compared)


def object_map(hist_blob: bytes, hist_ns: int, hist_nc: int, cur_blob: bytes, cur_ns: int, cur_nc: int) -> ObjectMap:
    assert len(hist_blob) == BLOB_SIZE and len(cur_blob) == BLOB_SIZE
    table = np.zeros(ENTRIES, MAP_DTYPE)
    a64, b64 = np.zeros((ENTRIES, 3)), np.zeros((ENTRIES, 3))
    tracked = hist_ns != cur_ns or hist_nc != cur_nc
    for k in range(ENTRIES):
        sphere = k < MAX_SPHERES
        i = k if sphere else k - MAX_SPHERES
        exists = (i < hist_ns and i < cur_ns) if sphere else (i < hist_nc and i < cur_nc)
        at, geo, words = entry_layout(k)
        state = DROP
        if exists and hist_blob[at + geo:at + geo + 64] == cur_blob[at + geo:at + geo + 64]:
            gh = np.frombuffer(hist_blob, np.float32, geo // 4, at)
            gc = np.frombuffer(cur_blob, np.float32, geo // 4, at)
            if all(gh[w].tobytes() == gc[w].tobytes() for w in words):
                state = KEEP
                a64[k] = 1.0
            else:
                h, c = gh.astype(np.float64), gc.astype(np.float64)
                with np.errstate(all="ignore"):
                    if sphere:
                        eh, ec = np.full(3, h[3]), np.full(3, c[3])
                    else:
                        eh, ec = h[4:7] - h[0:3], c[4:7] - c[0:3]
                    a = eh / ec
                    b = h[0:3] - a * c[0:3]
                    a32, b32 = a.astype(F), b.astype(F)
                ok = ((eh > 0).all() and (ec > 0).all() and np.isfinite(eh).all() and np.isfinite(ec).all() and np.isfinite(h[0:3]).all()
                      and np.isfinite(c[0:3]).all() and np.isfinite(a32).all() and np.isfinite(b32).all())
                if ok:
                    state = MOVED
                    a64[k], b64[k] = a, b
        if exists and state != KEEP:
            tracked = True
        table["state"][k] = state
    table["a"], table["b"] = a64.astype(F), b64.astype(F)
    return ObjectMap(table, table["state"].copy(), a64, b64, bool(tracked))


def keep_table() -> np.ndarray:
    """Every id KEEP (a = 1, b = 0)."""
    table = np.zeros(ENTRIES, MAP_DTYPE)
    table["a"] = F(1.0)
    return table


def moved_guides(guides, table):
    """The current guides as the tracked kernel sees them: pos = P' for a MOVED id (a * P + b: two roundings), id = -1 where the entry is
    DROP, or where the id is no index of the map.  Normal and t are untouched: planeDen = sigma_plane * t_p and the normal weight stay."""
    table = np.asarray(table).view(MAP_DTYPE).reshape(ENTRIES)
    ids = guides["id"]
    known = (ids >= 0) & (ids < ENTRIES)
    k = np.where(known, ids, 0)
    state = np.where(known, table["state"][k], DROP)
    a, b = table["a"][k].astype(F), table["b"][k].astype(F)
    out = guides.copy()
    with np.errstate(all="ignore"):
        moved = (a * guides["pos"] + b).astype(F)
    out["pos"] = np.where((state == MOVED)[..., None], moved, guides["pos"])
    out["id"] = np.where((state == KEEP) | (state == MOVED), ids, -1)
    return out


def integrate_tracked(image, n, guides, hist_image, hist_guides, B, O, table, params: dr.Params = dr.Params(), cap: int = dt.DEFAULT_MAX_HISTORY):
    """-> I (H, W, 4) float32 of a tracked render: arguments as denoise_temporal_reference.integrate, plus the object map (320 entries of
    MAP_DTYPE, or the 10,240 bytes read back) and cap = edit_max_history == 0 ? max_history : min(max_history, edit_max_history)."""
    assert hist_image is not None
    return dt.integrate(image, n, moved_guides(guides, table), hist_image, hist_guides, B, O, params, cap)


def cap_of(max_history: int, edit_max_history: int) -> int:
    return max_history if edit_max_history == 0 else min(max_history, edit_max_history)
