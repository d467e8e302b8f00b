"""The run sharing of the default kernels' in-order sphere loop (ray_trace_t<..., SHARE>, macro PT_RUN_SPHERE in csrc/pt_device.hpp) on
the layouts of sphere_run_cases.py, bit for bit against the CPU oracle through the C ABI: run lengths 1 to 63, all three kinds of
boundary, counts that are no multiple of four, runs across the 32-sphere words the kernel reads its bits in, and scene edits that
create, split and cut runs (the host recomputes the bits only when an upload or a count change marks the scene dirty).
test_sphere_runs_cpu.py shows on the oracle alone that every boundary of these layouts changes pixels when its bit is wrong, and by
pt_debug_plan_launch which kernel rows the launches below take (the images here cannot tell which row ran).  The instantiations that share
runs are the spp = 1 kernels with materials in LDS and no grid (persistent rows 0 - 5) and the multisample kernel's row 0; persistent row 10
(spp > 1, in-lane sample chain) runs the plain loop.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import sphere_run_cases as R
from test_gpu_parity import assert_bit_exact

pytestmark = pytest.mark.gpu

SPP3_CASES = ["mixed47", "long63", "one_run5", "one_run63", "no_runs"]


def tracer(pkg, sc, width=R.WIDTH, height=R.HEIGHT, spp=1, **extra):
    pt = pkg.PathTracer(R.env(), width, height, R.DEPTH, spp, R.FOCAL_LENGTH, R.APERTURE, **extra)
    pt.UploadScene(sc)
    pt.UploadBasicData(R.camera_ubo(width, height))
    return pt


def want(oracle, blob, sc_or_kw, frames, width=R.WIDTH, height=R.HEIGHT, spp=1, **extra):
    kw = sc_or_kw if isinstance(sc_or_kw, dict) else R.oracle_kwargs(sc_or_kw, spp=spp)
    return oracle.render(width, height, R.camera_ubo(width, height), bytes(blob), R.env(), num_frames=frames, **kw, **extra)


def pipeline_first(pkg, pt):
    """Make the handle one that has pipelined frames, then restart it: from then on it launches single frames tagged too, as ONE launch over
    the whole image (choose_launch_mode, csrc/mi355pt_launch.cpp), instead of two untagged row stripes — the launch forms `pipelined1` /
    `pipelinedN` of sphere_run_cases.launch_forms, whose rows test_sphere_runs_cpu.py pins."""
    for _ in range(16):  # (frames are held back while the GPU is busy with the handle's earlier ones: the first eight do it in practice)
        for _ in range(8):
            pt.Render()
        pt.Synchronize()
        if pkg.native.debug_launch_stats(pt._h)["saw_batch"]:
            break
    assert pkg.native.debug_launch_stats(pt._h)["saw_batch"], "128 back-to-back frames were never pipelined"
    pt.ResetRenderer()


# ------------------------------------------------------------------------------------------------ row 4
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_every_layout_equals_the_oracle(pkg, native_lib, oracle, name):
    """128 x 72, one sample per pixel, four frames: persistent row 4."""
    sc = R.BY_NAME[name].scene()
    pt = tracer(pkg, sc)
    for _ in range(4):
        pt.Render()
    got = pt.Result
    pt.Dispose()
    assert_bit_exact(got, want(oracle, sc.ubo_bytes(), sc, 4), name)


def _without_grid(pkg, render):
    pkg.native.debug_set("no_sphere_grid", 1)
    try:
        return render()
    finally:
        pkg.native.debug_set("no_sphere_grid", 0)


@pytest.mark.parametrize("how", ["pipelined", "striped"])
def test_runs_beyond_sphere_64_without_the_grid(pkg, native_lib, oracle, how):
    """Run bits beyond the second 32-sphere word: a scene of 64 or more spheres only takes the in-order loop with the sphere grid switched
    off (knob no_sphere_grid), and only shares runs while its materials still fit in LDS.  The count is the largest at which the launch
    plan says so for the launches THIS rendering can take (sphere_run_cases.words_counts; when this was written):
      pipelined   four back-to-back frames — row stripes, then tagged launches over the whole image: 125 spheres, runs across 64 and 96
      striped     four frames with the handle drained after each — untagged row stripes only, whose smaller queues leave the materials
                  room up to 186 spheres: runs across 64, 96, 128 and 160
    The layout has a run across every multiple of 32 below its count."""
    n = R.words_counts(native_lib)[how]
    assert n >= 65, "no count above 64 keeps the materials in LDS"
    sc = R.words_2_to_7(n).scene()
    blob = sc.ubo_bytes()
    assert not set(range(32, n, 32)) & set(R.boundaries(blob, n))

    def render():
        pt = tracer(pkg, sc)
        for _ in range(4):
            pt.Render()
            if how == "striped":
                pt.Synchronize()
        if how == "striped":
            assert not pkg.native.debug_launch_stats(pt._h)["saw_batch"]
        got = pt.Result
        pt.Dispose()
        return got

    assert_bit_exact(_without_grid(pkg, render), want(oracle, blob, sc, 4), f"{n} spheres, no grid, {how}")


def test_runs_beyond_sphere_64_in_the_batch_pass_kernel(pkg, native_lib, oracle):
    """The same at three samples per pixel through the multisample kernel (batch_pass_min_tiles = 0), whose parked continuations leave the
    materials room up to 79 spheres when this was written: a run across spheres 63 / 64."""
    n = R.words_counts(native_lib)["batch_pass"]
    assert n >= 65, "no count above 64 keeps the materials in LDS"
    sc = R.words_2_to_7(n).scene()

    def render():
        pkg.native.debug_set("batch_pass_min_tiles", 0)
        try:
            pt = tracer(pkg, sc, spp=3)
            for _ in range(2):
                for _ in range(3):
                    pt.Render()
                pt.Synchronize()
            got = pt.Result
            pt.Dispose()
            return got
        finally:
            pkg.native.debug_set("batch_pass_min_tiles", 16384)

    assert_bit_exact(_without_grid(pkg, render), want(oracle, sc.ubo_bytes(), sc, 6, spp=3), f"{n} spheres, no grid, spp 3")


# ------------------------------------------------------------------------------------------------ three samples per pixel
@pytest.fixture(scope="module")
def spp3_reference(oracle):
    """case -> the oracle's accumulations after 2 and after 15 frames at three samples per pixel (computed once, left unchanged)"""
    out = {}
    for name in SPP3_CASES:
        sc = R.BY_NAME[name].scene()
        frames = want(oracle, sc.ubo_bytes(), sc, 15, spp=3, dump_each=True)
        out[name] = (frames[1].copy(), frames[14].copy())
    return out


@pytest.mark.parametrize("name", SPP3_CASES)
def test_three_samples_per_pixel_fresh_and_pipelined(pkg, native_lib, oracle, spp3_reference, name):
    """spp 3, two frames.  On a fresh handle the first frame is an untagged launch: the batch-pass kernel (multisample row 0), which
    shares runs.  What follows is pipelined and takes the in-lane sample chain (persistent row 10) — as do both frames on a handle that has
    pipelined before.  Row 10 runs the PLAIN sphere loop (its bounce is instantiated without SHARE) and never reads the run bits: that
    half is a parity test of the plain loop on these layouts and cannot see a wrong bit."""
    sc = R.BY_NAME[name].scene()
    pt = tracer(pkg, sc, spp=3)
    pt.Render()
    pt.Render()
    assert_bit_exact(pt.Result, spp3_reference[name][0], f"{name} spp 3, fresh handle")
    pipeline_first(pkg, pt)
    pt.Render()
    pt.Render()
    got = pt.Result
    pt.Dispose()
    assert_bit_exact(got, spp3_reference[name][0], f"{name} spp 3, pipelined (row 10: the plain loop)")


def test_three_samples_per_pixel_in_the_batch_pass_kernel(pkg, native_lib, oracle, spp3_reference):
    """The same cases through the multisample kernel (row 0, which shares runs) for every launch: pipelined launches over a small image
    only take it with the knob batch_pass_min_tiles = 0.  Five launches of three frames, the later ones with cached tile masks."""
    pkg.native.debug_set("batch_pass_min_tiles", 0)
    try:
        for name in SPP3_CASES:
            pt = tracer(pkg, R.BY_NAME[name].scene(), spp=3)
            for _ in range(5):
                for _ in range(3):
                    pt.Render()
                pt.Synchronize()
            got = pt.Result
            pt.Dispose()
            assert_bit_exact(got, spp3_reference[name][1], f"{name} spp 3, batch pass")
    finally:
        pkg.native.debug_set("batch_pass_min_tiles", 16384)


# ------------------------------------------------------------------------------------------------ row 3
@pytest.mark.parametrize("name", ["mixed47", "n61"])
def test_the_headline_kernel_at_the_smallest_carrying_size(pkg, native_lib, oracle, name):
    """1000 x 768 = 12,000 tiles, the smallest image whose launch carries the pixel with its path (persistent row 3, the headline
    kernel) — for a launch over the whole image.  A single frame on a fresh handle goes out as two row stripes of 6,000 tiles (row 4), so
    the handle pipelines frames first and is restarted; the one frame compared is then one tagged launch."""
    W, H = 1000, 768
    sc = R.BY_NAME[name].scene()
    pt = tracer(pkg, sc, W, H)
    pipeline_first(pkg, pt)
    pt.Render()
    got = pt.Result
    pt.Dispose()
    assert_bit_exact(got, want(oracle, sc.ubo_bytes(), sc, 1, W, H), f"{name} 1000 x 768")


# ------------------------------------------------------------------------------------------------ edits
class EditScript:
    """mixed47 and the edits applied to it, on a host copy of the GameObjectsUBO (what the oracle renders).  Runs of mixed47 start at
    0 1 3 6 10 15 22 30 39."""

    def __init__(self):
        self.sc = R.BY_NAME["mixed47"].scene()
        self.blob = bytearray(self.sc.ubo_bytes())
        self.ns = self.sc.num_spheres

    def kw(self):
        return dict(R.oracle_kwargs(self.sc), num_spheres=self.ns)

    def upload(self, offset, data):
        data = np.ascontiguousarray(data).view(np.uint8)
        self.blob[offset:offset + data.nbytes] = data.tobytes()

    def count(self, ns):
        self.ns = ns

    def sphere(self, i):
        return np.frombuffer(bytes(self.blob[80 * i:80 * i + 80]), np.float32).copy()

    def steps(self):
        """-> [(what, function that applies the edit)]"""
        def onto_predecessor():  # sphere 10 starts the run of five: with sphere 9's x and z it joins the run before (0 1 3 6 11 15 ...)
            d = self.sphere(10)
            d[0], d[2] = self.sphere(9)[0], self.sphere(9)[2]
            self.upload(800, d)

        def split():  # sphere 25, the middle of the run of seven (22 - 28): 3 + 1 + 3
            d = self.sphere(25)
            d[2] = R.ZS[0]
            self.upload(80 * 25, d)

        def only_y():
            d = self.sphere(12)
            d[1] += np.float32(0.9)
            self.upload(80 * 12, d)

        def only_radius():
            d = self.sphere(16)
            d[3] = np.float32(1.05)
            self.upload(80 * 16, d)

        def only_material():
            d = self.sphere(33)
            d[4:7] = (0.1, 0.9, 0.4)
            self.upload(80 * 33, d)

        def across_two_records():  # 16 bytes: the last 8 of sphere 30's record (material padding) and x, y of sphere 31, which leaves its run
            d = np.concatenate([self.sphere(30)[18:20], np.array([R.XS[5], self.sphere(31)[1] + np.float32(0.3)], np.float32)])
            self.upload(80 * 30 + 72, d)

        def across_two_centres():  # 76 bytes from sphere 40's z to sphere 41's x: both leave the last run, each in its own way
            d = np.frombuffer(bytes(self.blob[80 * 40 + 8:80 * 41 + 4]), np.float32).copy()
            d[0], d[-1] = R.ZS[2], R.XS[3]
            self.upload(80 * 40 + 8, d)

        def identical():  # the early return: nothing is copied, nothing marked dirty
            self.upload(0, np.frombuffer(bytes(self.blob), np.uint8).copy())
            self.upload(80 * 25, self.sphere(25))

        return [("x and z moved onto the predecessor's", onto_predecessor), ("z changed inside a run of seven", split), ("only y", only_y),
                ("only the radius", only_radius), ("only a material word", only_material), ("16 bytes across two records", across_two_records),
                ("76 bytes across two centres", across_two_centres), ("identical bytes", identical)] + \
               [(f"NumSpheres = {n}", (lambda n=n: self.count(n))) for n in (46, 45, 44, 43, 38, 47)]


class Edited(EditScript):
    """... and the same edits sent to a renderer through GameObjectsUBO.SubData and NumSpheres, like the reference's editor does."""

    def __init__(self, pkg, **extra):
        super().__init__()
        self.pt = tracer(pkg, self.sc, **extra)

    def upload(self, offset, data):
        data = np.ascontiguousarray(data).view(np.uint8)
        self.pt.GameObjectsUBO.SubData(offset, data.nbytes, data)
        super().upload(offset, data)

    def count(self, ns):
        super().count(ns)
        self.pt.NumSpheres = ns


def test_partial_uploads_and_count_changes_move_the_runs(pkg, native_lib, oracle):
    """After every edit: restart, three frames, compare with the oracle on the edited scene.  By the time the counts change, the 76-byte
    edit has taken spheres 40 and 41 out of the last run: it is 42 - 46.  The counts 46, 45, 44 move the tail loop (ns % 4 spheres evaluated
    on their own) through it and end the four-sphere steps (ns & ~3 = 44) inside it; 43 ends them at 40, on a boundary; 38 ends them at 36,
    inside the run 32 - 38 that the 16-byte edit left, with two spheres of that run in the tail loop."""
    e = Edited(pkg)
    bits = []
    for what, edit in e.steps():
        edit()
        bits.append(pkg.native.debug_sphere_runs(bytes(e.blob), e.ns))
        e.pt.ResetRenderer()
        for _ in range(3):
            e.pt.Render()
        assert_bit_exact(e.pt.Result, want(oracle, e.blob, e.kw(), 3), f"after: {what}")
    e.pt.Dispose()
    mixed47 = R.BY_NAME["mixed47"].scene()
    first = pkg.native.debug_sphere_runs(mixed47.ubo_bytes(), 47)
    assert bits[0] == (first & ~(1 << 10)) | 1 << 11 and bits[1] == bits[0] | 1 << 25 | 1 << 26, "the edits create and split the runs they claim"
    assert bits[2] == bits[3] == bits[4] == bits[1] and bits[5] == bits[4] | 1 << 31 | 1 << 32 and bits[6] == bits[5] | 1 << 40 | 1 << 41 | 1 << 42
    assert bits[7] == bits[6]


def test_edits_between_pipelined_frames_reach_later_frames_only(pkg, native_lib, oracle):
    """The same edits with three frames rendered after each one and no restart: frames that are still pending or in flight when an upload
    arrives keep the scene — and the run bits — they were accepted with.  Pipelined launches against frame-by-frame launches
    (pt_set_frame_batch(1)), and both against the oracle accumulating over the edited scenes."""
    def run(batch):
        e = Edited(pkg)
        if batch:
            e.pt.SetFrameBatch(batch)
        for _ in range(3):
            e.pt.Render()
        for _, edit in e.steps():
            edit()
            for _ in range(3):
                e.pt.Render()
        out = e.pt.Result
        e.pt.Dispose()
        return out

    o = EditScript()  # (the oracle's side: the same edits on the host copy alone)
    image = want(oracle, o.blob, o.kw(), 3)
    for k, (_, edit) in enumerate(o.steps()):
        edit()
        image = want(oracle, o.blob, o.kw(), 3, frame_start=3 * (k + 1), image=image)
    pipelined = run(None)
    assert_bit_exact(pipelined, run(1), "pipelined vs frame-by-frame launches")
    assert_bit_exact(pipelined, image, "pipelined launches vs the oracle")


def test_group_handle_parts_compute_their_own_bits(pkg, native_lib, oracle):
    """A group handle of two parts on one device: uploads fan out, every part keeps its own copy of the scene and computes its own run
    bits — n61 as uploaded, then with a run created by a partial upload."""
    sc = R.BY_NAME["n61"].scene()
    pt = tracer(pkg, sc, devices=[0, 0])
    for _ in range(4):
        pt.Render()
    assert_bit_exact(pt.Result, want(oracle, sc.ubo_bytes(), sc, 4), "n61 on a group handle")
    blob = bytearray(sc.ubo_bytes())
    d = np.frombuffer(bytes(blob[80 * 29:80 * 30]), np.float32).copy()  # sphere 29 starts a run of one: onto sphere 28's x and z
    d[0], d[2] = np.frombuffer(bytes(blob[80 * 28:80 * 28 + 12]), np.float32)[[0, 2]]
    pt.GameObjectsUBO.SubData(80 * 29, 80, d)
    blob[80 * 29:80 * 30] = d.tobytes()
    assert pkg.native.debug_sphere_runs(bytes(blob), 61) == pkg.native.debug_sphere_runs(sc.ubo_bytes(), 61) & ~(1 << 29)
    pt.ResetRenderer()
    for _ in range(3):
        pt.Render()
    got = pt.Result
    pt.Dispose()
    assert_bit_exact(got, want(oracle, blob, sc, 3), "n61 on a group handle, after an upload that creates a run")
