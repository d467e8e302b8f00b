"""Scene geometry as scalar operands (ray_trace_t<..., SCALAR> in csrc/pt_device.hpp): the spp = 1 kernels with materials in LDS and no grid
(persistent rows 0 - 5) read four spheres with one 16-dword scalar load from the packed copy `sphereGeom` behind the device's GameObjectsUBO
(csrc/pt_kernels.hpp: kSphereGeomOffset) and a cuboid's min / max with one 8-dword scalar load from the block itself.  Every image here is
compared with the CPU oracle as uint32, at 128 x 72 (row 4) and at 1000 x 768 with pipelined launches (row 3, the headline kernel); the
rows are pinned by pt_debug_plan_launch in the test at the top, which needs no GPU — like the host-side tests of the copy behind it.

Cases: sphere counts around the four-sphere step, the ns % 4 tail and the 32-sphere run words, each with an even, an odd and no cuboid trip;
uploads that must reach the copy (whole scene, sub-ranges, ragged ranges, sphere 0) and one that must not matter (sphere 255's slot); count
changes that leave stale entries behind the count; geometry words that a scalar operand must hand to the VALU with the same bits as the
vector operand did (+0, -0, infinite, NaN and denormal values, a cuboid with min > max); and a group handle, whose parts keep a copy each.
GPU tests: `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import sphere_run_cases as R
from test_gpu_parity import assert_bit_exact
from test_gpu_sphere_runs import pipeline_first

F = np.float32
SPHERE_COUNTS, CUBOID_COUNTS = (0, 1, 3, 4, 5, 33, 125), (0, 1, 2, 7)
BIG = (1000, 768)  # 12,000 tiles: the smallest image whose whole-image launch carries the pixel with its path (row 3)
UBO_BYTES, CUBOIDS_AT = 26624, 20480


def base_scene():
    """125 spheres in runs across the 32-sphere words (sphere_run_cases.words_2_to_7) and the default room's 7 cuboids."""
    return R.words_2_to_7(125).scene()


def base_blob() -> bytearray:
    return bytearray(base_scene().ubo_bytes())


def words(blob, off, n):
    return np.frombuffer(bytes(blob[off:off + 4 * n]), F).copy()


def want(oracle, blob, ns, nc, frames, size=(R.WIDTH, R.HEIGHT), **extra):
    kw = dict(R.oracle_kwargs(base_scene()), num_spheres=ns, num_cuboids=nc)
    return oracle.render(size[0], size[1], R.camera_ubo(*size), bytes(blob), R.env(), num_frames=frames, **kw, **extra)


# ------------------------------------------------------------------------------------------------ no GPU: rows, upload ranges
def _rows(native_lib, width, height, frames, ns, nc, only):
    out = set()
    for name, form in R.launch_forms(width, height, 1, frames).items():
        if name.startswith(only):
            p = R.plan(native_lib, form, ns, nc, **(R.GRID_OFF if ns >= 64 else {}))
            assert p["error"] == 0 and p["matLds"] == 1 and p["grid"] == 0, (name, ns, nc, p)
            out.add((p["family"], p["kernelRow"]))
    return out


def test_the_cases_reach_rows_4_and_3(native_lib):
    """128 x 72: persistent row 4 however the frames reach the GPU; 1000 x 768: row 3 for the whole-image launches of a handle that has
    pipelined (single tagged frames and launches of two).  125 spheres take the in-order loop only with the sphere grid switched off."""
    for ns in SPHERE_COUNTS:
        for nc in CUBOID_COUNTS:
            assert _rows(native_lib, R.WIDTH, R.HEIGHT, 3, ns, nc, "") == {(R.PERSISTENT, 4)}, (ns, nc)
            assert _rows(native_lib, BIG[0], BIG[1], 2, ns, nc, "pipelined") == {(R.PERSISTENT, 3)}, (ns, nc)


def geom_range(lib, offset, size):
    lib.pt_debug_sphere_geom_range.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.pt_debug_sphere_geom_range.restype = C.c_int
    out = (C.c_int * 2)()
    assert lib.pt_debug_sphere_geom_range(offset, size, out) == 0
    return int(out[0]), int(out[1])


class HostCopy:
    """The GameObjectsUBO and the packed copy as the upload path maintains them, on the host: an upload writes its bytes into the block and
    refreshes the spheres pt_debug_sphere_geom_range names (the function pt_upload_game_objects calls) from the block."""

    def __init__(self, lib):
        self.lib, self.blob, self.geom = lib, bytearray(UBO_BYTES), np.zeros((256, 4), np.uint32)

    def upload(self, offset, data):
        data = bytes(data)
        self.blob[offset:offset + len(data)] = data
        first, count = geom_range(self.lib, offset, len(data))
        assert 0 <= first and first + count <= 256
        for i in range(first, first + count):
            self.geom[i] = np.frombuffer(bytes(self.blob[80 * i:80 * i + 16]), np.uint32)

    def check(self, what):
        expect = np.frombuffer(bytes(self.blob[:256 * 80]), np.uint32).reshape(256, 20)[:, :4]
        assert (self.geom == expect).all(), f"sphereGeom differs from the block after: {what}"


def upload_sequences():
    """-> [(what, [(offset, bytes)])]: the upload sequences of the GPU tests below, each applied on top of the whole base scene."""
    b = base_blob()
    rnd = np.random.RandomState(7)
    noise = lambda n: rnd.randint(0, 256, n, dtype=np.uint8).tobytes()
    per_object = [(80 * i, bytes(b[80 * i:80 * i + 80])) for i in range(125)] + [(CUBOIDS_AT + 96 * j, bytes(b[CUBOIDS_AT + 96 * j:CUBOIDS_AT + 96 * j + 96])) for j in range(7)]
    return [("one upload per object", []),
            ("the whole block at once", [(0, noise(UBO_BYTES))]),
            ("a sphere in the middle of a run and a cuboid's max", [(80 * 60, noise(16)), (CUBOIDS_AT + 96 * 3 + 16, noise(12))]),
            ("sphere 0", [(0, noise(80))]),
            ("sphere 255's slot", [(80 * 255, noise(80))]),
            ("the last byte of sphere 255's slot and the first cuboid", [(80 * 256 - 1, noise(97))]),
            ("from inside sphere 40's material to inside sphere 41's material", [(80 * 40 + 20, noise(100))]),
            ("inside sphere 40's material only", [(80 * 40 + 16, noise(64))]),
            ("ending inside sphere 41's geometry", [(80 * 40 + 40, noise(48))]),
            ("one byte of a radius", [(80 * 17 + 15, noise(1))]),
            ("spheres 100 to 140 in one range", [(80 * 100, noise(80 * 41))]),
            ("cuboids only", [(CUBOIDS_AT, noise(96 * 64))]),
            ("nothing", [(80 * 3, b"")])], per_object


def test_the_copy_follows_every_upload_on_the_host(native_lib):
    """After each sequence sphereGeom[i] equals bytes 80 i .. 80 i + 15 of the block for every i < 256 (pt::sphere_geom_range decides what
    the refresh kernel copies; the kernel itself runs the same sequences in test_the_copy_follows_every_upload_on_the_device)."""
    sequences, per_object = upload_sequences()
    for what, uploads in sequences:
        h = HostCopy(native_lib)
        for off, data in per_object:
            h.upload(off, data)
        h.check("one upload per object")
        for off, data in uploads:
            h.upload(off, data)
        h.check(what)


def test_upload_ranges_name_exactly_the_touched_spheres(native_lib):
    """Every (offset, size) around a record boundary, the ends of the Spheres[] array and the block: the range is the set of spheres with
    at least one byte in [offset, offset + size)."""
    offsets = sorted({o for k in (0, 1, 17, 254, 255) for o in range(80 * k - 2, 80 * k + 19) if o >= 0} | {20479, 20480, 20481, 26623})
    for off in offsets:
        for size in (0, 1, 2, 15, 16, 17, 79, 80, 81, 160, 161, 6144):
            if off + size > UBO_BYTES:
                continue
            touched = [i for i in range(256) if size > 0 and off < 80 * i + 80 and 80 * i < off + size]
            first, count = geom_range(native_lib, off, size)
            assert (list(range(first, first + count)) == touched) if touched else count == 0, (off, size)


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def read_copy(pkg, pt, part=0):
    """(the device's GameObjectsUBO as bytes, sphereGeom as (256, 4) uint32) of one part, behind everything queued"""
    lib = pkg.native.load()
    lib.pt_debug_read_sphere_geom.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pt_debug_read_sphere_geom.restype = C.c_int
    blob, geom = np.zeros(UBO_BYTES, np.uint8), np.zeros((256, 4), np.uint32)
    pkg.native.check(lib.pt_debug_read_sphere_geom(pt._h, part, blob.ctypes.data, geom.ctypes.data), pt._h)
    return blob.tobytes(), geom


def assert_copy_matches(pkg, pt, blob, what, parts=1):
    for part in range(parts):
        dev, geom = read_copy(pkg, pt, part)
        assert dev == bytes(blob), f"{what}: part {part}'s GameObjectsUBO differs from what was uploaded"
        expect = np.frombuffer(dev[:256 * 80], np.uint32).reshape(256, 20)[:, :4]
        assert (geom == expect).all(), f"{what}: part {part}'s sphereGeom differs from its GameObjectsUBO"


class Renderer:
    """One renderer with the base scene, and a host copy of its GameObjectsUBO (what the oracle renders)."""

    def __init__(self, pkg, size=(R.WIDTH, R.HEIGHT), **extra):
        self.pkg, self.size = pkg, size
        self.blob = base_blob()
        self.pt = pkg.PathTracer(R.env(), size[0], size[1], R.DEPTH, 1, R.FOCAL_LENGTH, R.APERTURE, **extra)
        self.pt.UploadScene(base_scene())
        self.pt.UploadBasicData(R.camera_ubo(*size))
        self.ns, self.nc = 125, 7
        if size == BIG:
            pipeline_first(pkg, self.pt)

    def upload(self, offset, data):
        data = np.ascontiguousarray(data).view(np.uint8)
        self.pt.GameObjectsUBO.SubData(offset, data.nbytes, data)
        self.blob[offset:offset + data.nbytes] = data.tobytes()

    def counts(self, ns, nc):
        self.ns, self.nc = ns, nc
        self.pt.NumSpheres = ns
        self.pt.NumCuboids = nc

    def restart(self, blob=None):
        if blob is not None:
            self.upload(0, np.frombuffer(bytes(blob), np.uint8))
        self.pt.ResetRenderer()

    def render(self, frames):
        for _ in range(frames):
            self.pt.Render()

    def want(self, oracle, frames, **extra):
        return want(oracle, self.blob, self.ns, self.nc, frames, self.size, **extra)


@pytest.fixture(scope="module")
def grid_off(pkg, native_lib):
    """125 spheres take the in-order loop (and rows 3 / 4) only with the sphere grid switched off; the smaller counts never build one."""
    pkg.native.debug_set("no_sphere_grid", 1)
    yield
    pkg.native.debug_set("no_sphere_grid", 0)


@pytest.fixture(scope="module", params=["row4", "row3"])
def shape(request, pkg, native_lib, grid_off):
    """One renderer per shape for the whole module: (name, Renderer, frames per comparison).  Row 3 has pipelined before and launches
    every frame tagged over the whole image; its two frames per comparison go out back to back."""
    r = Renderer(pkg, BIG if request.param == "row3" else (R.WIDTH, R.HEIGHT))
    yield request.param, r, (2 if request.param == "row3" else 3)
    r.pt.Dispose()


@gpu
def test_the_copy_follows_every_upload_on_the_device(pkg, native_lib):
    """The thirteen sequences of upload_sequences() through pt_upload_game_objects and the refresh kernel itself: after each one the
    device's block equals the bytes uploaded and the device's sphereGeom[i] equals bytes 80 i .. 80 i + 15 of it for every i < 256
    (read back behind everything queued; nothing is rendered from the random bytes)."""
    sequences, _ = upload_sequences()
    r = Renderer(pkg)
    assert_copy_matches(pkg, r.pt, r.blob, "one upload per object")
    for what, uploads in sequences:
        r.restart(base_blob())
        for off, data in uploads:
            if data:  # (an empty range is the host-side case: the binding hands the library no pointer for it)
                r.upload(off, np.frombuffer(data, np.uint8))
        assert_copy_matches(pkg, r.pt, r.blob, what)
    r.pt.Dispose()


@gpu
@pytest.mark.parametrize("nc", CUBOID_COUNTS)
@pytest.mark.parametrize("ns", SPHERE_COUNTS)
def test_sphere_and_cuboid_counts(oracle, shape, ns, nc):
    """The four-sphere step with and without a tail (0, 1, 3, 4, 5), across the first 32-sphere word (33) and over four of them with
    ns % 4 = 1 (125); no cuboid, one (the odd trip), two, seven.  The objects behind the counts stay in the block and in the copy."""
    name, r, frames = shape
    r.restart(base_blob())
    r.counts(ns, nc)
    r.render(frames)
    assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: {ns} spheres, {nc} cuboids")


def moved_sphere_and_cuboid_max(r):
    """sphere 60 (inside the run 54 - 65) half a unit up and towards the camera, cuboid 3's max shrunk: 16 + 12 bytes"""
    s = words(r.blob, 80 * 60, 4)
    s[1] += F(0.5)
    s[2] -= F(0.75)
    mx = words(r.blob, CUBOIDS_AT + 96 * 3 + 16, 3)
    mn = words(r.blob, CUBOIDS_AT + 96 * 3, 3)
    return (80 * 60, s), (CUBOIDS_AT + 96 * 3 + 16, (mn + (mx - mn) * F(0.5)).astype(F))


@gpu
def test_sub_range_upload_between_frames_without_a_synchronise(pkg, oracle, shape):
    """Frames, a sub-range upload of a sphere's geometry and of a cuboid's max, frames again — nothing waits in between: the frames
    accepted before the upload keep the old scene, those after it see the new one (the refresh of the copy is ordered like the upload).
    Then the same with the image read before the upload: the first image is the old scene's."""
    name, r, frames = shape
    r.restart(base_blob())
    r.counts(125, 7)
    old = bytes(r.blob)
    r.render(frames)
    for off, data in moved_sphere_and_cuboid_max(r):
        r.upload(off, data)
    r.render(frames)
    got = r.pt.Result
    first = want(oracle, old, 125, 7, frames, r.size)
    assert_bit_exact(got, r.want(oracle, frames, frame_start=frames, image=first.copy()), f"{name}: old scene, then the uploaded one")
    assert_copy_matches(pkg, r.pt, r.blob, name)
    r.restart(old)
    r.render(frames)
    assert_bit_exact(r.pt.Result, first, f"{name}: the old scene")
    for off, data in moved_sphere_and_cuboid_max(r):
        r.upload(off, data)
    r.pt.ResetRenderer()
    r.render(frames)
    assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: the uploaded scene")


@gpu
def test_count_change_leaves_stale_entries_behind_the_count(pkg, oracle, shape):
    """33 spheres, then 5: entries 5 .. 124 of the copy keep their spheres and must not be visited; then 4 (no tail) and back to 33."""
    name, r, frames = shape
    r.restart(base_blob())
    for ns in (33, 5, 4, 33):
        r.counts(ns, 7)
        r.pt.ResetRenderer()
        r.render(frames)
        assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: NumSpheres = {ns}")
    assert_copy_matches(pkg, r.pt, r.blob, name)


@gpu
def test_both_ends_of_the_block(pkg, oracle, shape):
    """Sphere 0 moved and resized (the start of the copy), then sphere 255's slot filled with a huge sphere around the camera at 125
    spheres (the end of the copy: uploaded, copied, never read by a launch)."""
    name, r, frames = shape
    r.restart(base_blob())
    r.counts(125, 7)
    s = words(r.blob, 0, 4)
    s[1] += F(1.25)
    s[3] = F(1.1)
    r.upload(0, s)
    r.pt.ResetRenderer()
    r.render(frames)
    assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: sphere 0 changed")
    huge = words(r.blob, 80 * 124, 20)
    huge[0:4] = (R.POSITION[0], R.POSITION[1], R.POSITION[2], 3.0)
    r.upload(80 * 255, huge)
    r.pt.ResetRenderer()
    r.render(frames)
    assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: sphere 255's slot filled")
    assert_copy_matches(pkg, r.pt, r.blob, name)
    assert (read_copy(pkg, r.pt)[1][255] == huge[0:4].view(np.uint32)).all()


@gpu
def test_ragged_uploads(pkg, oracle, shape):
    """A range that starts inside sphere 40's material and ends inside sphere 41's (41's geometry is rewritten with changed words), one
    that stays inside sphere 40's material (geometry untouched), and one that ends inside sphere 41's geometry (x and y only)."""
    name, r, frames = shape
    r.restart(base_blob())
    r.counts(125, 7)
    a = words(r.blob, 80 * 40 + 20, 25)      # sphere 40 words 5 .. 19, sphere 41 words 0 .. 9
    a[0:2] = (0.2, 0.9)                      # albedo y, z of sphere 40
    a[15 + 1] += F(0.6)                      # sphere 41's y
    a[15 + 3] = F(0.5)                       # sphere 41's radius
    b = words(r.blob, 80 * 40 + 16, 16)      # sphere 40's material only
    b[4:7] = (0.7, 0.1, 0.1)                 # emissive
    for what, off, data in (("material to material across a geometry", 80 * 40 + 20, a), ("inside one material", 80 * 40 + 16, b)):
        r.upload(off, data)
        r.pt.ResetRenderer()
        r.render(frames)
        assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: {what}")
    c = words(r.blob, 80 * 40 + 40, 12)      # sphere 40 words 10 .. 19, sphere 41's x and y
    c[10] = words(r.blob, 80 * 35, 1)[0]     # x of another column: sphere 41 leaves its run
    c[11] -= F(0.4)
    r.upload(80 * 40 + 40, c)
    r.pt.ResetRenderer()
    r.render(frames)
    assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: ending inside a geometry")
    assert_copy_matches(pkg, r.pt, r.blob, name)


def camera_sphere(radius):
    """a sphere centred on the camera: every primary ray starts at its centre"""
    return np.array([R.POSITION[0], R.POSITION[1], R.POSITION[2], radius], F)


ODD_GEOMETRY = {
    # name -> [(byte offset, float32 words)] on the base scene.  Sphere 2 stands in a four-sphere step and in a run, sphere 124 is the tail
    "radius +0": [(80 * 2 + 12, [0.0]), (80 * 124 + 12, [0.0])],
    "radius -0": [(80 * 2 + 12, [-0.0]), (80 * 124 + 12, [-0.0])],
    "radius infinite": [(80 * 2 + 12, [np.inf]), (80 * 124 + 12, [-np.inf])],
    "radius NaN": [(80 * 2 + 12, [np.nan]), (80 * 124 + 12, [np.nan])],
    # a denormal centre word in a step and in the tail, and a sphere of denormal r * r around the camera: -r * r + |oc|^2 = -1e-40 there, so
    # the sphere is hit from inside at t2 = sqrt(1e-40) — unless a denormal operand is flushed on its way, then it is missed
    "denormal": [(80 * 2, [1e-40]), (80 * 124 + 8, [-1e-40]), (80 * 3, camera_sphere(1e-20))],
    "cuboid min > max": [(CUBOIDS_AT + 96 * 2, [3.0, 3.0, 3.0]), (CUBOIDS_AT + 96 * 2 + 16, [-3.0, -3.0, -3.0]),
                         (CUBOIDS_AT + 96 * 5, [np.inf]), (CUBOIDS_AT + 96 * 5 + 20, [np.nan]), (CUBOIDS_AT + 96 * 6 + 4, [-0.0, 1e-40])],
}


@gpu
@pytest.mark.parametrize("what", list(ODD_GEOMETRY))
def test_geometry_words_reach_the_valu_bit_for_bit(pkg, oracle, shape, what):
    """A scalar operand is the same 32 bits as the vector operand it replaces, whatever they encode: zero and negative-zero radii, an
    infinite and a NaN radius, denormal centre words and a denormal r * r, and cuboids whose min lies beyond their max or holds
    infinities, NaNs, -0 and denormals — in a four-sphere step, in the ns % 4 tail, and in both cuboid trips."""
    name, r, frames = shape
    r.restart(base_blob())
    r.counts(125, 7)
    for off, data in ODD_GEOMETRY[what]:
        r.upload(off, np.asarray(data, F))
    r.pt.ResetRenderer()
    r.render(frames)
    assert_bit_exact(r.pt.Result, r.want(oracle, frames), f"{name}: {what}")
    assert_copy_matches(pkg, r.pt, r.blob, f"{name}: {what}")


@gpu
def test_group_handle_over_one_device_twice(pkg, native_lib, oracle, grid_off):
    """Two parts on one device: each keeps its own block and its own copy, and both follow a sub-range upload."""
    r = Renderer(pkg, devices=[0, 0])
    r.counts(125, 7)
    r.render(3)
    assert_bit_exact(r.pt.Result, r.want(oracle, 3), "group handle, base scene")
    assert_copy_matches(pkg, r.pt, r.blob, "group handle", parts=2)
    for off, data in moved_sphere_and_cuboid_max(r):
        r.upload(off, data)
    assert_copy_matches(pkg, r.pt, r.blob, "group handle after a sub-range upload", parts=2)
    r.pt.ResetRenderer()
    r.render(3)
    got = r.pt.Result
    r.pt.Dispose()
    assert_bit_exact(got, r.want(oracle, 3), "group handle after a sub-range upload")
