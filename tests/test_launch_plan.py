"""CPU tests of the launch plan (csrc/pt_integrate_persistent.hip: plan_launch, through the library's host-only export
pt_debug_plan_launch): which kernel a launch takes, its grid and LDS sizes, its ticket count and every FrameArgs field "set by the
launch" — compared with the decisions recorded from the PARENT commit's launch_integrate (tests/golden/launch_plans.json; its header
names the commit and how the table was taken).  docs/kernels.md, "Which kernel a launch takes", holds the dispatch table."""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
SIMPLE, POOL, PERSISTENT, MULTISAMPLE = 0, 1, 2, 3
INVALID_VALUE, NOT_SUPPORTED = 1, 801  # hipErrorInvalidValue, hipErrorNotSupported
UNSIGNED = {"ticketsConsumed", "tilesFrameMagic", "tilesXMagic"}
IN_FIELDS = ["width", "height", "tilesX", "tilesY", "numSpheres", "numCuboids", "spp", "envFormat", "variant", "batchFrames", "tagged", "drainCompaction",
             "queueChunk", "numCUs", "gridBytes", "hasGrid", "hasTimeline", "hasStartedFlags", "hasFeed", "wantFeed",
             "parkedMax", "parkCapacity", "parkMin", "noBatchPass", "batchPassMinTiles", "noSphereGrid", "forceLeanLds", "carryLast", "gridCarry"]
OUT_FIELDS = ["error", "family", "kernelRow", "minWavesPerSimd", "timeline", "spp1", "matLds", "grid", "carry", "compact", "feed", "workgroups", "ldsBytes",
              "poolTiles", "ticketsConsumed", "fed", "materialsInLds", "gridLdsBytes", "sceneLdsBytes", "parkedMax", "contCapacity", "contBatchMin",
              "drainCompaction", "startedFlagsSet", "tilesFrameMagic", "tilesXMagic", "feedSet", "displaySet", "workgroupsPerCU", "batchPass", "queueLdsBytes",
              "staticLdsBytes", "fitPerCU"]

# The dispatch tables, in the library's order (kPersistentKernels, kMultisampleKernels): minWavesPerSimd, timeline, spp1, matLds, grid, carry, compact, feed
KEY = ["minWavesPerSimd", "timeline", "spp1", "matLds", "grid", "carry", "compact", "feed"]
PERSISTENT_ROWS = [
    (6, 0, 1, 1, 0, 1, 0, 1), (6, 0, 1, 1, 0, 0, 0, 1), (6, 1, 1, 1, 0, 0, 1, 0), (6, 0, 1, 1, 0, 1, 0, 0), (6, 0, 1, 1, 0, 0, 0, 0), (6, 0, 1, 1, 0, 0, 1, 0),
    (6, 0, 1, 0, 1, 1, 0, 0), (5, 0, 1, 0, 1, 1, 0, 0), (6, 0, 1, 0, 1, 0, 0, 0), (6, 0, 1, 0, 0, 0, 1, 0),
    (5, 0, 0, 1, 0, 0, 1, 0), (5, 0, 0, 0, 1, 0, 1, 0), (5, 0, 0, 0, 0, 0, 1, 0),
]
# (the batch-pass kernel has no timeline / carry / compact / feed arguments and runs at its own launch bound of 5; the parent's recorder shows 0 for them)
MULTISAMPLE_ROWS = [(5, 0, 0, 1, 0, 0, 0, 0), (5, 0, 0, 0, 1, 0, 0, 0), (5, 0, 0, 0, 0, 0, 0, 0)]
KNOWN_UNREACHABLE = set()  # (family, row) pairs no input reaches: none


class PlanIn(C.Structure):
    _fields_ = [(n, C.c_int) for n in IN_FIELDS]


class PlanOut(C.Structure):
    _fields_ = [(n, C.c_uint if n in UNSIGNED else C.c_int) for n in OUT_FIELDS]


@pytest.fixture(scope="module")
def table():
    doc = json.load(open(FIXTURE))
    assert doc["parent_commit"] == "4e6ffb449df081df6a6f89bfa6c309e7a645ba6e" and doc["inputs"] == IN_FIELDS
    cols = doc["columns"]
    n_in = 1 + len(doc["inputs"])
    return [(dict(zip(cols[1:n_in], r[1:n_in])), dict(zip(cols[n_in:], r[n_in:])), r[0]) for r in doc["rows"]]


def plan(native_lib, inputs):
    fn = native_lib.pt_debug_plan_launch
    fn.argtypes = [C.POINTER(PlanIn), C.POINTER(PlanOut)]
    fn.restype = C.c_int
    out = PlanOut()
    assert fn(C.byref(PlanIn(**inputs)), C.byref(out)) == 0
    return {n: getattr(out, n) for n in OUT_FIELDS}


def row_of(o):
    rows = {PERSISTENT: PERSISTENT_ROWS, MULTISAMPLE: MULTISAMPLE_ROWS}[o["family"]]
    return rows.index(tuple(o[k] for k in KEY))


def test_plan_equals_the_parents_decisions(native_lib, table):
    """Every recorded value (-1 = the parent does not show it) is what plan_launch answers; a queue-kernel plan names the dispatch-table
    row with exactly the parent's template arguments."""
    wrong = []
    for inputs, want, scene in table:
        got = plan(native_lib, inputs)
        bad = {k: (got[k], v) for k, v in want.items() if v != -1 and got[k] != v}
        if want["error"] == 0 and want["family"] >= PERSISTENT and got["kernelRow"] != row_of(want):
            bad["kernelRow"] = (got["kernelRow"], row_of(want))
        if want["error"] == 0 and want["family"] < PERSISTENT and got["kernelRow"] != -1:
            bad["kernelRow"] = (got["kernelRow"], -1)
        if bad:
            wrong.append((scene, inputs, bad))
    assert not wrong, f"{len(wrong)} of {len(table)} plans differ (got, parent); first: {wrong[:3]}"


def test_the_recorded_table_covers_every_decision(table):
    """Asserted on the fixture alone, so that a thin matrix cannot pass: every row of both dispatch tables, the simple and the pool kernel and
    both error returns occur; the LDS-fit loop leaves through each of its three exits; the 1,280-byte granule edge is met from both sides."""
    ok = [(i, o) for i, o, _ in table if o["error"] == 0]
    reached = {(o["family"], row_of(o)) for _, o in ok if o["family"] >= PERSISTENT}
    every = {(PERSISTENT, r) for r in range(len(PERSISTENT_ROWS))} | {(MULTISAMPLE, r) for r in range(len(MULTISAMPLE_ROWS))}
    assert reached | KNOWN_UNREACHABLE == every and not reached & KNOWN_UNREACHABLE
    assert {o["family"] for _, o in ok} == {SIMPLE, POOL, PERSISTENT, MULTISAMPLE}
    assert {o["poolTiles"] for _, o in ok if o["family"] == POOL} == {8, 2}  # variants 2 and 6
    assert {o["error"] for _, o, _ in table} == {0, INVALID_VALUE, NOT_SUPPORTED}
    assert any(o["fed"] == 1 and o["ticketsConsumed"] == o["workgroups"] for _, o in ok)
    assert any(i["hasStartedFlags"] and not o["startedFlagsSet"] for i, o in ok) and any(o["workgroups"] < i["numCUs"] * o["workgroupsPerCU"] for i, o in ok if o["family"] >= PERSISTENT)
    # LDS-fit loop.  Carry is first asked for on a full-size spp = 1 image (>= 12,000 tiles) without drain compaction, per-wavefront timeline or
    # (unless grid_carry) sphere grid; "dropped" = such a launch that does not carry.
    spp1 = [(i, o) for i, o in ok if o["family"] == PERSISTENT and o["spp1"] == 1]
    asked = [(i, o) for i, o in spp1 if i["tilesX"] * i["tilesY"] >= 12000 and i["carryLast"] and o["drainCompaction"] == 0 and not i["hasTimeline"] and
             (o["grid"] == 0 or i["gridCarry"])]
    assert any(o["carry"] == 1 for _, o in asked) and any(o["carry"] == 0 for _, o in asked), "carry kept / carry dropped"
    lists = [(i, o) for i, o in spp1 if i["tagged"] and o["drainCompaction"] == 0 and i["parkedMax"] < 0 and o["carry"] == 0]
    assert any(16 <= o["parkedMax"] < 64 for _, o in lists) and any(o["parkedMax"] == 64 for _, o in lists), "parked lists shrunk / left alone"
    assert any(o["materialsInLds"] == 0 and o["grid"] == 0 and not i["forceLeanLds"] for i, o in ok if o["family"] >= PERSISTENT), "materials leave LDS to keep a workgroup"
    assert any(o["materialsInLds"] == 1 for _, o in ok if o["family"] >= PERSISTENT)
    # granule edge: 21 granules of 1,280 bytes run six workgroups per CU, 22 run five although six times the bytes are below 160 KB
    granules = lambda o: -(-(o["ldsBytes"] + o["staticLdsBytes"]) // 1280)
    six = [(i, o) for i, o in ok if o["family"] >= PERSISTENT and o["workgroupsPerCU"] >= 6]
    assert any(granules(o) == 21 and o["fitPerCU"] == 6 for _, o in six), "a launch in the last granule that fits six times"
    assert any(granules(o) == 22 and o["fitPerCU"] == 5 and 6 * (o["ldsBytes"] + o["staticLdsBytes"]) <= 160 * 1024 for _, o in six), "... and one just over it"


def test_a_plan_without_a_table_row_is_not_produced(native_lib, table):
    """Every queue-kernel plan of the matrix names a row of the library's own table (launch_integrate refuses a plan that names none:
    hipErrorInvalidValue and a line on stderr, never a neighbouring kernel)."""
    for inputs, want, _ in table:
        got = plan(native_lib, inputs)
        if got["error"] != INVALID_VALUE and got["family"] >= PERSISTENT:
            rows = PERSISTENT_ROWS if got["family"] == PERSISTENT else MULTISAMPLE_ROWS
            assert 0 <= got["kernelRow"] < len(rows) and rows[got["kernelRow"]] == tuple(got[k] for k in KEY), inputs
