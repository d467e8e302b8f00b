"""CPU tests of the sphere runs of the default kernels' in-order sphere loop (ptgrid::sphere_runs -> FrameArgs::sphereRunStart ->
ray_trace_t<..., SHARE>, csrc/pt_device.hpp), on the layouts of sphere_run_cases.py:
  * the run bits the host computes (through the host-only export pt_debug_sphere_runs) equal the rule restated in Python;
  * the layouts can SEE a wrong bit: on the oracle alone, every run boundary changes pixels when its sphere is evaluated with its
    predecessor's x and z — so the bit-exact GPU comparisons of test_gpu_sphere_runs.py cannot pass with a bit wrongly cleared;
  * the launches of test_gpu_sphere_runs.py take the kernel rows they claim (pt_debug_plan_launch).
Nothing here needs a GPU."""
import numpy as np
import pytest

import sphere_run_cases as R

FRAMES = 4


WORDS = ("pipelined", "striped", "batch_pass")  # the three renderings of words_2_to_7 (sphere_run_cases.words_counts)


def words_cases(native_lib):
    """-> {rendering: case}; a rendering whose launch forms keep the materials in LDS for no count of 64 or more is missing"""
    return {k: R.words_2_to_7(n) for k, n in R.words_counts(native_lib).items() if n}


# ------------------------------------------------------------------------------------------------ the run bits
def test_run_bits_of_every_case_equal_the_restated_rule(pkg, native_lib):
    words = words_cases(native_lib)
    assert set(words) == set(WORDS), "no count of 64 or more keeps the materials in LDS: a words_2_to_7 case is gone"
    cases = R.CASES + list(words.values())
    for c in cases:
        sc = c.scene()
        blob, ns = sc.ubo_bytes(), sc.num_spheres
        assert ns == c.num_spheres
        got = pkg.native.debug_sphere_runs(blob, ns)
        assert got == R.expected_runs(blob, ns), f"{c.name}: run bits {got:#x}"
        assert got & 1 and got >> ns == (1 << (256 - ns)) - 1
        # ... and the layout has the runs its name promises: a new run exactly where a column starts, unless the column before has the same bits
        starts, i = [], 0
        for k, (xi, zl, count) in enumerate(c.runs):
            if k == 0 or (c.runs[k - 1][0], c.runs[k - 1][1]) != (xi, zl):
                starts.append(i)
            i += count
        assert [0] + R.boundaries(blob, ns) == starts, c.name
    # the signed zero: equal values, different bits
    blob = R.SIGNED_ZERO.scene().ubo_bytes()
    w, f = np.frombuffer(blob, np.uint32), np.frombuffer(blob, np.float32)
    assert f[20 * 5] == f[20 * 4] and w[20 * 5] != w[20 * 4] and w[20 * 5 + 2] == w[20 * 4 + 2] and 5 in R.boundaries(blob, 17)


def test_run_bits_of_random_blobs_equal_the_restated_rule(pkg, native_lib):
    """2,000 random GameObjectsUBO images whose x and z words come from pools of four bit patterns each (runs of every length occur; +0.0
    and -0.0 are both in the x pool), every other word random bits; counts around the 32- and 64-sphere words and at both ends."""
    rng = np.random.RandomState(20)
    pool_x = np.array([0.0, -0.0, 1.5, -7.25], np.float32).view(np.uint32)
    pool_z = np.array([-5.0, -6.4, 0.0, 3.0e-39], np.float32).view(np.uint32)  # (a denormal too: the rule compares bits, not values)
    lengths = set()
    for trial in range(2000):
        ns = (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256)[trial % 11]
        w = rng.randint(0, 1 << 32, 6656, dtype=np.uint64).astype(np.uint32)
        stay = rng.rand(256) < rng.choice([0.3, 0.7, 0.95])  # sphere i keeps its predecessor's words
        xi, zi = rng.randint(0, 4, 256), rng.randint(0, 4, 256)
        for i in range(1, 256):
            if stay[i]:
                xi[i], zi[i] = xi[i - 1], zi[i - 1]
        w[0:5120:20], w[2:5120:20] = pool_x[xi], pool_z[zi]
        got, want = pkg.native.debug_sphere_runs(w.view(np.float32), ns), R.expected_runs(w.tobytes(), ns)
        assert got == want, f"trial {trial}, {ns} spheres: {got:#x} != {want:#x}"
        starts = [i for i in range(ns) if want >> i & 1] + [ns]
        lengths |= set(np.diff(starts).tolist())
    assert set(range(1, 33)) <= lengths and max(lengths) > 64, sorted(lengths)


# ------------------------------------------------------------------------------------------------ the layouts can see a wrong bit
def _accumulations(oracle, blob, sc):
    """-> the depth-1 and the depth-6 accumulation of FRAMES frames"""
    basic, env = R.camera_ubo(), R.env()
    return tuple(oracle.render(R.WIDTH, R.HEIGHT, basic, blob, env, num_frames=FRAMES, **R.oracle_kwargs(sc, depth)) for depth in (1, R.DEPTH))


def _changed_beyond_the_first_bounce(true, other) -> int:
    """Pixels whose depth-1 accumulation is the same bit for bit and whose depth-6 accumulation differs.  (The first bounce of the
    spp = 1 kernels runs in the tile pass, whose culled loop does not share: only later bounces go through the run loop.)"""
    same1 = (true[0].view(np.uint32) == other[0].view(np.uint32)).all(-1)
    diff6 = (true[1].view(np.uint32) != other[1].view(np.uint32)).any(-1)
    return int((same1 & diff6).sum())


@pytest.mark.parametrize("name", [c.name for c in R.WITH_BOUNDARIES] + [f"words_2_to_7_{k}" for k in WORDS])
def test_every_run_boundary_is_visible_to_the_oracle(oracle, native_lib, name):
    """For every run boundary i: the blob in which sphere i has sphere i - 1's x and z — what the loop computes for sphere i's
    discriminant when bit i is wrongly clear — renders differently in at least one pixel whose first bounce is unchanged.  No boundary
    is left out, with one exception that is asserted rather than skipped: where the two centres differ in BITS but not in VALUE (+0.0
    and -0.0, the signed_zero case), o.x - c.x is the same number either way, no image can tell, and the test demands exactly that;
    those bits are pinned by the run-bit tests above alone."""
    c = R.BY_NAME[name] if name in R.BY_NAME else words_cases(native_lib).get(name[len("words_2_to_7_"):])
    assert c is not None, "no count of 64 or more keeps the materials in LDS"
    sc = c.scene()
    blob, ns = sc.ubo_bytes(), sc.num_spheres
    f = np.frombuffer(blob, np.float32)
    true = _accumulations(oracle, blob, sc)
    bounds = R.boundaries(blob, ns)
    assert bounds, "a case without boundaries belongs to the test below"
    changed, invisible = {}, []
    for i in bounds:
        other = _accumulations(oracle, R.shares_wrongly(blob, i), sc)
        if f[20 * i] == f[20 * (i - 1)] and f[20 * i + 2] == f[20 * (i - 1) + 2]:
            invisible.append(i)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(true, other)), f"{c.name}: boundary {i}"
        else:
            changed[i] = _changed_beyond_the_first_bounce(true, other)
    print(f"{c.name}: {len(bounds)} boundaries, {len(bounds) - len(changed) - len(invisible)} left out, {len(invisible)} between equal values; "
          f"pixels changed beyond the first bounce: minimum {min(changed.values())}, per boundary {changed}")
    assert sorted(list(changed) + invisible) == bounds
    assert invisible == ([5, 14] if c.name == "signed_zero" else [])
    blind = [i for i, n in changed.items() if n < 1]
    assert not blind, f"{c.name}: boundaries {blind} change no pixel beyond the first bounce"


@pytest.mark.parametrize("name", [c.name for c in R.WITHOUT_BOUNDARIES])
def test_a_sphere_moved_out_of_its_run_is_visible_to_the_oracle(oracle, name):
    """one_run and tiny have no boundary; the opposite mistake — a bit wrongly SET is harmless, but a sphere whose z left the run while its
    bit stayed clear is not — must show: moving the middle sphere's z to another level changes the image."""
    c = R.BY_NAME[name]
    sc = c.scene()
    blob, ns = sc.ubo_bytes(), sc.num_spheres
    assert R.boundaries(blob, ns) == []
    i = ns // 2
    z = np.frombuffer(blob, np.float32)[20 * i + 2]
    moved = R.with_centre_words(blob, i, z=R.ZS[2] if z != R.ZS[2] else R.ZS[0])
    assert R.expected_runs(moved, ns) != R.expected_runs(blob, ns) or ns == 1
    true, other = _accumulations(oracle, blob, sc), _accumulations(oracle, moved, sc)
    n = int((true[1].view(np.uint32) != other[1].view(np.uint32)).any(-1).sum())
    print(f"{c.name}: sphere {i} moved in z changes {n} pixels")
    assert n >= 1


# ------------------------------------------------------------------------------------------------ the rows the GPU cases reach
def _rows(native_lib, width, height, spp, frames, ns, only=None, **knobs):
    out = {}
    for form_name, form in R.launch_forms(width, height, spp, frames).items():
        if only is None or form_name.startswith(only):
            p = R.plan(native_lib, form, ns, **knobs)
            assert p["error"] == 0 and p["matLds"] == 1 and p["grid"] == 0, (form_name, ns, p)
            out[form_name] = (p["family"], p["kernelRow"])
    return out


def test_the_gpu_cases_reach_the_rows_they_claim(native_lib):
    """What test_gpu_sphere_runs.py launches, by plan_launch (through sphere_run_cases.launch_forms, a restatement of how the host
    launches).  Every plan keeps the materials in LDS and walks no grid, and
      128 x 72, spp 1            persistent row 4, however the frames reach the GPU (row stripes, one pipelined launch, single tagged frames;
                                 also the parts of a group handle and the cut-down sphere counts of the edit sequence); an image of fewer
                                 than 32 rows would go out as one untagged launch with drain compaction, row 5 — no GPU case has one
      1000 x 768, spp 1          row 3 for a launch over the whole image (12,000 tiles: the pixel travels with its path) — which a handle
                                 takes once it has pipelined frames; the two row stripes of a single frame on a fresh handle have 6,000 tiles
                                 each and take row 4, so the GPU test pipelines first
      spp 3                      the multisample family's row 0 for an untagged frame on an idle handle — a kernel that shares runs — and
                                 persistent row 10 for pipelined launches, which does NOT (its bounce is instantiated without SHARE)
      spp 3, batch_pass_min_tiles = 0    the multisample family's row 0 either way.
    Rows 4, 5, 3 and multisample row 0 are instantiations that share runs (R.SHARING_ROWS)."""
    counts = sorted({c.num_spheres for c in R.CASES} | {46, 45, 44, 43, 38})
    for ns in counts:
        for height in (72, 40, 36, 32):  # (the image, and what one part of a two-part group may own)
            for frames in (4, 3):
                assert set(_rows(native_lib, R.WIDTH, height, 1, frames, ns).values()) == {(R.PERSISTENT, 4)}, ns
        assert _rows(native_lib, R.WIDTH, 24, 1, 4, ns, only="striped") == {"striped0": (R.PERSISTENT, 5)}
    assert {(R.PERSISTENT, 3), (R.PERSISTENT, 4), (R.PERSISTENT, 5), (R.MULTISAMPLE, 0)} <= R.SHARING_ROWS and (R.PERSISTENT, 10) not in R.SHARING_ROWS
    for ns in (47, 61):
        assert set(_rows(native_lib, 1000, 768, 1, 1, ns, only="pipelined").values()) == {(R.PERSISTENT, 3)}
        assert set(_rows(native_lib, 1000, 768, 1, 1, ns, only="striped").values()) == {(R.PERSISTENT, 4)}
    for ns in (47, 63, 5, 48):
        assert set(_rows(native_lib, R.WIDTH, R.HEIGHT, 3, 2, ns, only="pipelined").values()) == {(R.PERSISTENT, 10)}
        assert set(_rows(native_lib, R.WIDTH, R.HEIGHT, 3, 2, ns, only="striped").values()) == {(R.MULTISAMPLE, 0)}
        assert set(_rows(native_lib, R.WIDTH, R.HEIGHT, 3, 3, ns, batchPassMinTiles=0).values()) == {(R.MULTISAMPLE, 0)}


def test_the_words_cases_take_the_largest_counts_their_launches_share_runs_at(native_lib):
    """words_2_to_7, per rendering: at its count every launch form that rendering can take is a sharing row with the grid switched off,
    one more sphere and one of them loses the materials; the layout has a run across every multiple of 32 below the count.  (When this
    was written: 125, 186 and 79 spheres — the 32-sphere words 3, 5 and 2.)"""
    counts = R.words_counts(native_lib)
    assert all(counts[k] >= 65 for k in WORDS), counts
    spp1, spp3 = R.launch_forms(R.WIDTH, R.HEIGHT, 1, 4), R.launch_forms(R.WIDTH, R.HEIGHT, 3, 3)
    forms = {"pipelined": (spp1, {}), "striped": ({k: v for k, v in spp1.items() if k.startswith("striped")}, {}), "batch_pass": (spp3, dict(batchPassMinTiles=0))}
    want_rows = {"pipelined": {(R.PERSISTENT, 4)}, "striped": {(R.PERSISTENT, 4)}, "batch_pass": {(R.MULTISAMPLE, 0)}}
    for k in WORDS:
        n, (fs, knobs) = counts[k], forms[k]
        plans = [R.plan(native_lib, f, n, **R.GRID_OFF, **knobs) for f in fs.values()]
        assert all(p["error"] == 0 and p["matLds"] == 1 and p["grid"] == 0 for p in plans)
        assert {(p["family"], p["kernelRow"]) for p in plans} == want_rows[k] <= R.SHARING_ROWS
        if n < 256:
            assert any(R.plan(native_lib, f, n + 1, **R.GRID_OFF, **knobs)["matLds"] == 0 for f in fs.values()), k
        blob = R.words_2_to_7(n).scene().ubo_bytes()
        bounds = R.boundaries(blob, n)
        assert all(w not in bounds for w in range(32, n, 32)) and (n - 1) // 32 >= 2
    print("words_2_to_7 counts:", counts, "last words:", {k: (counts[k] - 1) // 32 for k in WORDS})
