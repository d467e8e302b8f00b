"""A fixed table of small scenes with degenerate and extreme objects, shared by test_degenerate_cpu.py (what every case is aimed at,
proved on the oracle alone) and test_gpu_degenerate.py (the HIP path against the oracle on the same table).  Neither GPU code nor the
reference's sources are imported here.

A case is a scene built with pkg.scene and then patched at blob level (Material clamps its arguments, the blob does not), a camera,
an image size, depth, spp, aperture and an environment key.  Blob offsets: sphere i at 80 i (centre 0, radius 12, material 16),
cuboid j at 20480 + 96 j (min 0, max 16, material 32); inside a material: albedo 0, specularChance 12, emissiv 16,
specularRoughness 28, absorbance 32, refractionChance 44, refractionRoughness 48, ior 52.

Every case names the objects it is about (`bad`, in the id order of the first-hit query: sphere i = i, cuboid j = 256 + j), the blob
its image is compared with on the CPU (`base`: the same scene with those objects repaired, removed, or — for slots past the count —
zeroed) and what it is aimed at (`aim`):
  hit        the bad objects are the first hit of at least 10 % of the pixels
  candidate  the bad objects can never be hit; their REPAIRED twins are the first hit of at least 10 % of the pixels, i.e. that many
             rays evaluate the bad object where a benign one would have been accepted
  bounce     the class acts from the second bounce on (materials, Beer's law): more than 2 bounces in at least 10 % of the pixels
  none       slots past the object count: no ray ever reads them
`still` cases are those whose point is that the image does NOT move against `base` (never-hit objects, slots past the count).

The stage: twelve spheres on a 4 x 3 lattice at z = -12 (x = -4.5, -1.5, 1.5, 4.5; y = -3, 0, 3; radius 1.25: all exactly
representable), numbered column by column, so that three consecutive spheres share their x and z bits (sphere runs of the default
kernels); a floor plate, a back wall and a box; the camera at (0, 0, -8) looking down -z.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

import configs

pkg = configs.pkg
S = pkg.scene
F = np.float32
NAN, INF = float("nan"), float("inf")
DENORMAL = 1e-40
PT_MAX_SPHERES, PT_MAX_CUBOIDS = 256, 64
SPHERE_STRIDE, CUBOID_BASE, CUBOID_STRIDE = 80, 20480, 96
MAT = dict(albedo=(0, "<3f"), specular_chance=(12, "<f"), emissiv=(16, "<3f"), specular_roughness=(28, "<f"), absorbance=(32, "<3f"),
           refraction_chance=(44, "<f"), refraction_roughness=(48, "<f"), ior=(52, "<f"))
STAGE_POS, STAGE_LOOK = (0.0, 0.0, -8.0), (-90.0, 0.0)
OBLIQUE_POS, OBLIQUE_LOOK = (-5.0, 2.0, -9.0), (-50.0, -15.0)
CAM2_POS, CAM2_LOOK = (5.0, 2.0, -3.0), (20.0, -10.0)  # InvView's translation equals ViewPos bit for bit (first_hit_cases.py)
DEPTH, FRAMES = 8, 2


# ------------------------------------------------------------------------------------------------ patching
def _pack(b, off, fmt, v):
    if fmt == "<3f" and np.ndim(v) == 0:
        v = (v, v, v)
    struct.pack_into(fmt, b, off, *((v,) if fmt == "<f" else v))


def moved_away(blob: bytes, ids) -> bytes:
    """the listed objects (first-hit id numbering) 1000 units up: out of every ray's way, the counts unchanged"""
    f = np.frombuffer(blob, np.float32).copy()
    for k in ids:
        if k < PT_MAX_SPHERES:
            f[20 * k + 1] += F(1000.0)
        else:
            j = k - PT_MAX_SPHERES
            f[5120 + 24 * j + 1] += F(1000.0)
            f[5120 + 24 * j + 5] += F(1000.0)
    return f.tobytes()


def patch_sphere(b: bytearray, i: int, centre=None, radius=None, **mat):
    """sphere i of the blob: centre (3 floats), radius, and any material field by name (MAT)"""
    if centre is not None:
        struct.pack_into("<3f", b, SPHERE_STRIDE * i, *centre)
    if radius is not None:
        struct.pack_into("<f", b, SPHERE_STRIDE * i + 12, radius)
    for k, v in mat.items():
        _pack(b, SPHERE_STRIDE * i + 16 + MAT[k][0], MAT[k][1], v)


def patch_cuboid(b: bytearray, j: int, mn=None, mx=None, **mat):
    if mn is not None:
        struct.pack_into("<3f", b, CUBOID_BASE + CUBOID_STRIDE * j, *mn)
    if mx is not None:
        struct.pack_into("<3f", b, CUBOID_BASE + CUBOID_STRIDE * j + 16, *mx)
    for k, v in mat.items():
        _pack(b, CUBOID_BASE + CUBOID_STRIDE * j + 32 + MAT[k][0], MAT[k][1], v)


def copy_sphere(b: bytearray, src: int, dst: int, geometry_only=True):
    n = 16 if geometry_only else SPHERE_STRIDE
    b[SPHERE_STRIDE * dst:SPHERE_STRIDE * dst + n] = b[SPHERE_STRIDE * src:SPHERE_STRIDE * src + n]


def fill_unused(blob: bytes, ns: int, nc: int, word: int) -> bytes:
    """every 32-bit word of the slots at and beyond the counts set to `word`"""
    w = np.frombuffer(blob, np.uint32).copy()
    w[20 * ns:20 * PT_MAX_SPHERES] = word
    w[CUBOID_BASE // 4 + 24 * nc:] = word
    return w.tobytes()


def remove_objects(blob: bytes, ns: int, nc: int, ids):
    """-> (blob, ns, nc) without the listed objects (first-hit id numbering); the others keep their order, so every tie of the
    reference's strict `t1 < T` falls the same way"""
    b = np.frombuffer(blob, np.uint8)
    sph = [b[80 * i:80 * i + 80] for i in range(ns) if i not in ids]
    cub = [b[CUBOID_BASE + 96 * j:CUBOID_BASE + 96 * j + 96] for j in range(nc) if PT_MAX_SPHERES + j not in ids]
    out = np.zeros(b.size, np.uint8)
    for i, s in enumerate(sph):
        out[80 * i:80 * i + 80] = s
    for j, c in enumerate(cub):
        out[CUBOID_BASE + 96 * j:CUBOID_BASE + 96 * j + 96] = c
    return out.tobytes(), len(sph), len(cub)


# ------------------------------------------------------------------------------------------------ the stage
def material(i: int):
    """Varies per sphere: diffuse, rough mirror, absorbing glass (refraction chance 0.9; roughness 0 and 0.5 alternate)."""
    if i % 3 == 1:
        return S.Material(albedo=S.vec3(1.0), absorbance=S.vec3(0.3, 0.6, 0.9), specular_chance=0.02, ior=1.3, refraction_chance=0.9,
                          refraction_roughness=0.0 if i % 2 else 0.5)
    palette = [(0.59, 0.59, 0.99), (0.9, 0.25, 0.25), (0.3, 0.85, 0.35), (0.95, 0.9, 0.3), (0.8, 0.8, 0.8)]
    return S.Material(albedo=S.vec3(*palette[i % 5]), specular_chance=(i % 4) / 4, specular_roughness=(i % 3) / 3)


def glass(i: int):
    return S.Material(albedo=S.vec3(1.0), absorbance=S.vec3(0.3, 0.6, 0.9), specular_chance=0.02, ior=1.3, refraction_chance=0.9,
                      refraction_roughness=0.0 if i % 2 else 0.5)


LATTICE = [(F(-4.5 + 3.0 * (i // 3)), F(-3.0 + 3.0 * (i % 3)), F(-12.0)) for i in range(12)]


def stage(spheres=12, mat=material, box=True, z=-12.0, boxes=1):
    sc = S.Scene()
    for i in range(spheres):
        x, y, _ = LATTICE[i]
        sc.spheres.append(S.Sphere(np.array([x, y, z], F), F(1.25), i, mat(i)))
    add = lambda pos, dim, m: sc.cuboids.append(S.Cuboid(np.array(pos, F), np.array(dim, F), len(sc.cuboids), m))  # noqa: E731
    add((0.0, -5.0, -12.0), (40.0, 0.5, 25.0), S.Material(albedo=S.vec3(0.2, 0.04, 0.04), specular_roughness=0.051))
    add((0.0, 2.0, -20.0), (40.0, 14.0, 0.5), S.Material(albedo=S.vec3(0.37109375, 0.67578125, 0.3359375)))
    if box:
        add((0.0, -2.75, -10.5), (2.0, 1.0, 1.0), S.Material(albedo=S.vec3(1.0), absorbance=S.vec3(0.05, 0.1, 0.2), specular_chance=0.05, ior=1.5,
                                                          refraction_chance=0.9))
    for k in range(boxes - 1):  # further glass boxes beside it (cuboids 3 ..): the material classes sit on cuboids too
        add(((-5.0, -2.5, 2.5, 5.0)[k], -2.5, -10.5), (1.5, 1.5, 1.0), glass(k))
    return sc


def padded(sc, total: int, flat=False):
    """`sc` padded with ordinary spheres to `total`: small ones on a jittered lattice behind and around the stage's — or, `flat`, in
    the stage's own plane z = -12, between its spheres (every centre of the scene in one plane)"""
    rng = np.random.RandomState(total)
    n0 = sc.num_spheres
    k = 0
    while sc.num_spheres < total:
        gx, gy, gz = k % 10, (k // 10) % 6, k // 60
        k += 1
        pos = np.array([-9.0 + 2.0 * gx + 0.4 * rng.rand(), -4.0 + 1.5 * gy + 0.4 * rng.rand(), -14.0 - 1.2 * gz - 0.3 * rng.rand()], F)
        if flat:  # the gaps of the 4 x 3 lattice and a ring around it
            pos = np.array([-9.0 + 1.5 * gx, -4.5 + 1.5 * gy + (0.0 if gx % 2 else 0.75), -12.0], F)
            if any(abs(pos[0] - x) < 1.6 and abs(pos[1] - y) < 1.6 for x, y, _ in LATTICE):
                continue
        i = sc.num_spheres
        sc.spheres.append(S.Sphere(pos, F(0.3 + 0.15 * rng.rand()), i, material(i + n0)))
    return sc


def full_cuboids(sc):
    """small boxes on the floor up to the 64 of the UBO"""
    j = 0
    while sc.num_cuboids < PT_MAX_CUBOIDS:
        pos = np.array([-9.5 + 1.0 * (j % 20), -4.5 + 0.2 * (j // 20), -10.0 + 0.6 * (j // 20)], F)
        sc.cuboids.append(S.Cuboid(pos, np.array([0.5, 0.5 + 0.1 * (j % 3), 0.5], F), sc.num_cuboids, material(j)))
        j += 1
    return sc


@dataclass(frozen=True)
class Built:
    blob: bytes
    ns: int
    nc: int
    bad: tuple                   # ids of the degenerate objects (first-hit numbering)
    base: tuple                  # (blob, ns, nc) the image is compared with: repaired / removed / zeroed
    repaired: tuple = None       # (blob, ns, nc) with the bad objects benign (aim `candidate`; default: base)


@dataclass(frozen=True)
class Case:
    name: str
    klass: str                   # F1 .. F6, N
    make: object                 # () -> Built
    aim: str                     # hit | candidate | bounce | none
    still: bool = False
    first_hit: bool = False      # in the first-hit table of the GPU tests (geometry classes)
    width: int = 64
    height: int = 36
    position: tuple = STAGE_POS
    look: tuple = STAGE_LOOK
    aperture: float = 0.0
    focal_length: float = 20.0
    env: str = "sky_f32_32"
    spp: int = 1
    depth: int = DEPTH
    fov: float = None            # degrees; None: the host's 103
    grid: object = None          # F6 / N: what pt_debug_sphere_grid reports (True: a grid, False: refused); None: fewer than 64 spheres
    ties: bool = False           # F3: at least 50 pixels with an exact tie t1 == T
    nan_normals: bool = False    # F4 scaled rooms: at least 50 first hits whose cuboid normal is NaN
    q2: bool = False             # F4: hits whose normal has two non-zero components

    @property
    def tier(self):
        return "N" if self.klass == "N" else "F"


_built = {}


def built(case: Case) -> Built:
    if case.name not in _built:
        _built[case.name] = case.make()
    return _built[case.name]


def basic(case: Case) -> bytes:
    cam = pkg.camera.Camera(position=case.position, look_x=case.look[0], look_y=case.look[1])
    return pkg.camera.basic_data_ubo(cam, case.width, case.height, **({} if case.fov is None else dict(fov_degrees=case.fov)))


def env(case: Case):
    return configs.load_env(case.env)


def oracle_kwargs(case: Case, ns: int, nc: int, spp=None) -> dict:
    return dict(num_spheres=ns, num_cuboids=nc, ray_depth=case.depth, spp=case.spp if spp is None else spp, focal_length=case.focal_length,
                aperture=case.aperture)


_images = {}


def oracle_image(oracle, case: Case, which="blob", frames=FRAMES, spp=None, **kw):
    """the oracle's accumulation of `frames` frames of the case's scene (`blob`) or of what it is compared with (`base`); computed once"""
    key = (case.name, which, frames, spp, tuple(sorted(kw.items())))
    if key not in _images:
        b = built(case)
        blob, ns, nc = (b.blob, b.ns, b.nc) if which == "blob" else b.base
        img = oracle.render(case.width, case.height, basic(case), blob, env(case), num_frames=frames, **oracle_kwargs(case, ns, nc, spp), **kw)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


# ------------------------------------------------------------------------------------------------ comparison
def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_colour(got, want):
    """(H, W) bool: RGB words equal as uint32, or both NaN; alpha equal as uint32.  The sign and payload of a NaN are not part of the
    contract: which operand's payload an operation with two NaN operands keeps, and what an accumulation over many frames carries,
    may differ between an x86 and the GPU.  (Measured on an MI355X: generated NaNs were 0xFFC00000 on both sides, propagated ones
    kept 0x7FC00000, and one pixel of one 40-frame case differed in its NaN word: docs/parity.md.)"""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    rgb = (words(g[..., :3]) == words(w[..., :3])) | (np.isnan(g[..., :3]) & np.isnan(w[..., :3]))
    return rgb.all(-1) & (words(g[..., 3]) == words(w[..., 3]))


def nan_only(got, want):
    """(H, W) bool: pixels that same_colour accepts only through NaN == NaN"""
    return same_colour(got, want) & (words(got) != words(want)).any(-1)


def nan_pixels(img):
    return np.isnan(np.asarray(img)[..., :3]).any(-1)


# ------------------------------------------------------------------------------------------------ aim predicates (CPU)
def pinhole_rays(basic_blob: bytes, W: int, H: int):
    """pixel-centre rays of a BasicDataUBO (compute.glsl:352-357) in float64, rounded to float32: (origin (3,), directions (H, W, 3))"""
    b = np.frombuffer(basic_blob, np.float32).astype(np.float64)
    P, V = b[0:16].reshape(4, 4).T, b[16:32].reshape(4, 4).T
    nx, ny = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    eye = np.stack([nx, ny, -np.ones_like(nx), np.zeros_like(nx)], -1) @ P.T
    wd = np.stack([eye[..., 0], eye[..., 1], -np.ones_like(nx), np.zeros_like(nx)], -1) @ V.T
    d = wd[..., :3]
    return np.frombuffer(basic_blob, np.float32)[28:31].copy(), (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def replay(oracle, blob, ns, nc, o, d):
    """The Replayer of first_hit_cases.py over an image of rays -> (winner (H, W) int, T (H, W) float32, tie (H, W) int: the lowest id
    of ANOTHER object that the ray hits with the winner's own entry distance, t1 == T bit for bit as values; -1: none)."""
    import first_hit_cases as fh
    rp = fh.Replayer(oracle, blob, ns, nc)
    H, W = d.shape[:2]
    winner, T, tie = np.full((H, W), -1, np.int32), np.full((H, W), fh.FLOAT_MAX, np.float32), np.full((H, W), -1, np.int32)
    ids = list(range(ns)) + [PT_MAX_SPHERES + j for j in range(nc)]
    for y in range(H):
        for x in range(W):
            rp.set_ray(o, d[y, x])
            t_acc, win, tied = fh.FLOAT_MAX, -1, -1
            for k in ids:
                hit, t1, t2 = rp.leaf(k)
                if hit and t2 > 0.0:
                    if t1 < t_acc:
                        t_acc, win, tied = (t2 if t1 < 0.0 else t1), k, -1
                    elif t1 == t_acc and t1 >= 0.0 and tied < 0:
                        tied = k
            winner[y, x], T[y, x], tie[y, x] = win, t_acc, tied
    return winner, T, tie


_replays = {}


def case_replay(oracle, case: Case, which="blob"):
    key = (case.name, which)
    if key not in _replays:
        b = built(case)
        blob, ns, nc = {"blob": (b.blob, b.ns, b.nc), "base": b.base, "repaired": b.repaired or b.base}[which]
        o, d = pinhole_rays(basic(case), case.width, case.height)
        _replays[key] = replay(oracle, blob, ns, nc, o, d)
    return _replays[key]


def first_hit_share(oracle, case: Case) -> float:
    """share of the pixels whose first hit (pixel-centre pinhole ray, the oracle's leaf functions and acceptance rule) is one of the
    case's bad objects — for aim `candidate`: one of their repaired twins in the repaired scene"""
    winner = case_replay(oracle, case, "repaired" if case.aim == "candidate" else "blob")[0]
    return float(np.isin(winner, built(case).bad).mean())


def bounce_counts(oracle, case: Case, frame=1):
    import ctypes as C
    b = built(case)
    o = oracle
    p = o._params(case.width, case.height, b.ns, b.nc, case.depth, case.spp, case.focal_length, case.aperture, env(case))
    bas, objs, e = o._inputs(basic(case), b.blob, env(case))
    counts = np.zeros((case.height, case.width), np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fn = o.lib.pto_bounce_counts
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, fp, fp, C.c_void_p, C.c_int, ip]
    assert fn(C.byref(p), bas.ctypes.data_as(fp), objs.ctypes.data_as(fp), e.ctypes.data_as(C.c_void_p), frame, counts.ctypes.data_as(ip)) == 0
    return counts


def moved_share(oracle, case: Case) -> float:
    """share of the pixels in which the oracle's image differs (as words, NaN == NaN) from the `base` scene's"""
    return float((~same_colour(oracle_image(oracle, case), oracle_image(oracle, case, "base"))).mean())


# ------------------------------------------------------------------------------------------------ the table
def _blob(sc):
    return bytearray(sc.ubo_bytes()), sc.num_spheres, sc.num_cuboids


def _repaired(sc, b, bad, **kw):
    """the usual shape: `base` = the unpatched scene"""
    return Built(bytes(b), sc.num_spheres, sc.num_cuboids, tuple(bad), (sc.ubo_bytes(), sc.num_spheres, sc.num_cuboids), **kw)


def _removed(sc, b, bad):
    """never-hit objects: `base` = the scene without them, `repaired` = the unpatched scene"""
    ns, nc = sc.num_spheres, sc.num_cuboids
    return Built(bytes(b), ns, nc, tuple(bad), remove_objects(bytes(b), ns, nc, set(bad)), (sc.ubo_bytes(), ns, nc))


# ---- F1: radii
SMALL_RADII = {0: 0.0, 1: -0.0, 2: DENORMAL, 3: 1e-20, 4: -1.25, 5: -1.25, 6: 0.0, 7: -1.25, 8: -1.25, 9: -0.0, 10: -1.25, 11: -1.25}


def f1_small(n=12, flat=False):
    sc = padded(stage(), n, flat)
    b, _, _ = _blob(sc)
    for i, r in SMALL_RADII.items():
        patch_sphere(b, i, radius=r)
    return b, sc


def make_f1_negative():
    sc = stage()
    b, _, _ = _blob(sc)
    for i in range(12):
        patch_sphere(b, i, radius=-1.25)
    return _repaired(sc, b, range(12))


def make_f1_zero():
    """+0, -0, denormal and 1e-20 radii: never hit (a ray would have to pass through the centre exactly)"""
    sc = stage()
    b, _, _ = _blob(sc)
    bad = []
    for i in range(12):
        patch_sphere(b, i, radius=[0.0, -0.0, DENORMAL, 1e-20][i % 4])
        bad.append(i)
    return _removed(sc, b, bad)


def make_f1_huge(radius, centre, twin=None):
    """a huge sphere after nine of the stage's, over the floor alone: it is what every other ray meets.  `twin` (centre, radius): the
    sphere is never hit (r^2 = inf: the root is inf - inf), the image must equal the scene's without it, and the twin stands for it in
    the `candidate` aim — the same sphere where its radius is finite, else the same cone as seen from the camera at a tenth of the size"""
    def make():
        sc = stage(spheres=9)
        sc.cuboids = sc.cuboids[:1]
        m = S.Material(albedo=S.vec3(0.8, 0.7, 0.6), specular_chance=0.3, specular_roughness=0.2)
        sc.spheres.append(S.Sphere(np.array(twin[0] if twin else centre, F), F(twin[1] if twin else 1.0), 9, m))
        b, _, _ = _blob(sc)
        patch_sphere(b, 9, centre=centre, radius=radius)
        return _removed(sc, b, [9]) if twin else _repaired(sc, b, [9])
    return make


# ---- F2: the camera on the geometry (cam2: the ray origin equals ViewPos bit for bit; aperture 0)
def _cam2_scene():
    """the stage's spheres moved in front of cam2 (view direction (0.925, -0.174, 0.337)) on a coarse lattice of exact values"""
    sc = S.Scene()
    k = 0
    for dx in (8.0, 11.0):
        for dy in (-3.0, 0.0, 3.0):
            for dz in (0.0, 4.0):
                sc.spheres.append(S.Sphere(np.array([5.0 + dx, 2.0 + dy, -3.0 + dz], F), F(1.25), k, material(k)))
                k += 1
    sc.cuboids.append(S.Cuboid(np.array([10.0, -4.0, 0.0], F), np.array([40.0, 0.5, 40.0], F), 0, S.Material(albedo=S.vec3(0.2, 0.04, 0.04), specular_roughness=0.051)))
    return sc


def make_f2_centre():
    sc = _cam2_scene()
    sc.spheres.insert(0, S.Sphere(np.array(CAM2_POS, F), F(6.0), 0, glass(1)))  # the camera at its centre; the lattice's first row inside it
    for i, s in enumerate(sc.spheres):
        s.instance = i
    b, _, _ = _blob(sc)
    base = remove_objects(bytes(b), sc.num_spheres, sc.num_cuboids, {0})
    return Built(bytes(b), sc.num_spheres, sc.num_cuboids, (0,), base, (moved_away(bytes(b), [0]), sc.num_spheres, sc.num_cuboids))


def make_f2_surface():
    sc = _cam2_scene()
    # centre = ViewPos + (r, 0, 0), r = 2: |oc|^2 - r^2 == 0 exactly, every ray with d.x > 0 enters at t1 == 0
    sc.spheres.append(S.Sphere(np.array([7.0, 2.0, -3.0], F), F(2.0), sc.num_spheres, glass(0)))
    # and behind the camera a sphere whose surface lies one ulp of its radius short of it (centre = ViewPos - (2, 0, 0), r = 2 - 2^-23:
    # |oc|^2 - r^2 = 4.77e-7 > 0): every ray of the view points away from it with b^2 - c one ulp below b^2 — the case the kernel's
    # early out `c > 0 && b > 1e-10` decides without the square root.  Never hit; not among the bad objects.
    sc.spheres.append(S.Sphere(np.array([3.0, 2.0, -3.0], F), F(2.0), sc.num_spheres, material(0)))
    b, _, _ = _blob(sc)
    patch_sphere(b, sc.num_spheres - 1, radius=float(F(2.0) - F(2.0 ** -23)))
    bad = sc.num_spheres - 2
    return Built(bytes(b), sc.num_spheres, sc.num_cuboids, (bad,), remove_objects(bytes(b), sc.num_spheres, sc.num_cuboids, {bad}),
                 (moved_away(bytes(b), [bad]), sc.num_spheres, sc.num_cuboids))


def make_f2_face():
    sc = _cam2_scene()
    # a glass box whose top face lies in the plane y = 2 of the camera, and one whose near x face lies in the plane x = 5
    sc.cuboids.append(S.Cuboid(np.array([9.0, 0.5, -1.0], F), np.array([6.0, 3.0, 6.0], F), 1, glass(1)))
    sc.cuboids.append(S.Cuboid(np.array([7.0, 4.0, -1.0], F), np.array([4.0, 2.0, 3.0], F), 2, material(3)))
    assert sc.cuboids[1].max[1] == F(2.0) and sc.cuboids[2].min[0] == F(5.0)
    b, _, _ = _blob(sc)
    return Built(bytes(b), sc.num_spheres, sc.num_cuboids, (257, 258), remove_objects(bytes(b), sc.num_spheres, sc.num_cuboids, {257, 258}),
                 (moved_away(bytes(b), [257, 258]), sc.num_spheres, sc.num_cuboids))


# ---- F3: coincident objects
def f3_spheres(n=12):
    """1 = 0 (two identical), 3 = 4 = 5 (three identical), 7 at 6's centre with another radius, 9 = 10 at 11's x and z: every group
    lies inside a sphere run (equal x and z bits) or spans a run boundary (5 | 6)"""
    sc = padded(stage(), n)
    b, _, _ = _blob(sc)
    copy_sphere(b, 0, 1)
    copy_sphere(b, 3, 4)
    copy_sphere(b, 3, 5)
    patch_sphere(b, 7, centre=LATTICE[6], radius=0.75)
    patch_sphere(b, 8, centre=LATTICE[6], radius=1.75)
    copy_sphere(b, 9, 10)
    return b, sc


def make_f3_spheres():
    b, sc = f3_spheres()
    return _repaired(sc, b, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10])


def make_f3_cuboids():
    """two identical cuboids (materials differ); a sphere tangent to a cuboid face from outside and one from inside; a sphere whose
    front and a cuboid face at the same distance along the view axis"""
    sc = stage(spheres=3, box=False)
    M = S.Material
    sc.cuboids.append(S.Cuboid(np.array([-3.0, 1.0, -12.0], F), np.array([4.0, 4.0, 2.0], F), 2, M(albedo=S.vec3(0.9, 0.3, 0.3))))
    sc.cuboids.append(S.Cuboid(np.array([-3.0, 1.0, -12.0], F), np.array([4.0, 4.0, 2.0], F), 3, M(albedo=S.vec3(0.3, 0.3, 0.9), specular_chance=0.5)))
    sc.cuboids.append(S.Cuboid(np.array([3.5, 0.0, -13.0], F), np.array([5.0, 6.0, 2.0], F), 4, glass(0)))  # front face z = -12
    sc.spheres[0] = S.Sphere(np.array([2.5, 1.5, -10.75], F), F(1.25), 0, material(0))   # touches z = -12 from outside
    sc.spheres[1] = S.Sphere(np.array([4.5, 1.5, -13.0], F), F(1.0), 1, material(2))     # inside the box, touches both z faces
    sc.spheres[2] = S.Sphere(np.array([3.5, -1.5, -13.0], F), F(1.0), 2, glass(1))       # front at z = -12: the face's distance on the axis
    b, _, _ = _blob(sc)
    return Built(bytes(b), 3, 5, (0, 1, 2, 258, 259, 260), remove_objects(bytes(b), 3, 5, {0, 1, 2, 259}), (moved_away(bytes(b), [0, 1, 2, 259]), 3, 5))


# ---- F4: cuboids
def _f4(boxes):
    """the stage without its spheres and box, and the listed (min, max) cuboids after the floor and the wall"""
    sc = stage(spheres=0, box=False)
    for k, _ in enumerate(boxes):
        sc.cuboids.append(S.Cuboid(np.array([0.0, 0.0, -12.0], F), np.array([2.0, 2.0, 2.0], F), 2 + k, material(k)))
    b, _, _ = _blob(sc)
    for k, (mn, mx) in enumerate(boxes):
        patch_cuboid(b, 2 + k, mn=mn, mx=mx)
    return sc, b


def _benign_boxes(boxes):
    """the same boxes repaired axis by axis: ordered bounds at least 1 apart are kept, nearer or inverted ones become 2 thick around
    their centre, a non-finite bound lies 2 from the finite one (neither finite: [-1, 1])"""
    out = []
    for mn, mx in boxes:
        lo, hi = [], []
        for a, b in zip(mn, mx):
            fa, fb = np.isfinite(a), np.isfinite(b)
            if fa and fb:
                a, b = (a, b) if b - a >= 1.0 else ((a + b) / 2 - 1.0, (a + b) / 2 + 1.0)
            elif fa:
                b = a + 2.0
            elif fb:
                a = b - 2.0
            else:
                a, b = -1.0, 1.0
            lo.append(a)
            hi.append(b)
        out.append((tuple(lo), tuple(hi)))
    return out


FLAT_BOXES = [((-6.0, -2.0, -12.0), (-2.0, 2.0, -12.0)),      # plate facing the camera
              ((-1.0, 1.0, -12.0), (3.0, 1.0, -10.0)),        # plate seen edge-on from the stage camera (y == camera's would be 0; here above)
              ((4.0, -2.0, -13.0), (4.0, 3.0, -9.0)),         # plate in a plane x = const
              ((-5.0, 3.0, -11.0), (5.0, 3.0, -11.0)),        # rod
              ((0.0, -2.0, -11.0), (0.0, -2.0, -11.0))]       # point
INVERTED_BOXES = [((-6.0, -2.0, -11.0), (-2.0, 2.0, -13.0)),  # min > max in z only
                  ((3.0, -2.0, -13.0), (1.0, 2.0, -11.0)),    # ... in x only
                  ((6.5, 2.0, -11.0), (3.5, -2.0, -13.0)),    # ... on all axes
                  ((-1.0, 4.5, -11.0), (-3.5, 2.5, -13.0))]   # ... on all axes
TINY_BOXES = [((-3.0, 0.0, -10.0), (-3.0 + 1e-6, 1e-6, -10.0 + 1e-6)), ((-2.0, -2.0, -12.0), (2.0, 2.0, -12.0 + 1e-6)),
              ((3.0, -3.0, -13.0), (3.0 + 1e-6, 3.0, -9.0))]
EPS_BOXES = [((-6.0, -3.0, -12.0), (6.0, 3.0, -12.0 + 1e-3)),  # 1e-3 thick, facing the camera
             ((-7.0, 3.5, -13.0), (7.0, 3.5 + 1e-3, -9.0)),    # ... seen from below
             ((-7.5, -4.0, -13.0), (-7.5 + 1e-3, 4.0, -9.0))]  # ... in a plane x = const


def make_f4(boxes, removed=False):
    def make():
        sc, b = _f4(boxes)
        bad = [258 + k for k in range(len(boxes))]
        sc2, b2 = _f4(_benign_boxes(boxes))
        fixed = (bytes(b2), sc2.num_spheres, sc2.num_cuboids)
        if removed:
            return Built(bytes(b), 0, sc.num_cuboids, tuple(bad), remove_objects(bytes(b), 0, sc.num_cuboids, set(bad)), fixed)
        return Built(bytes(b), 0, sc.num_cuboids, tuple(bad), fixed)
    return make


def make_f4_room(scale):
    """the default room times `scale` (the camera with it): hit points are further than EPSILON from every face in binary32"""
    def make():
        sc = S.Scene()
        sc.cuboids = S.default_cuboids()
        b, _, _ = _blob(sc)
        base = bytes(b)
        for j, c in enumerate(sc.cuboids):
            patch_cuboid(b, j, mn=tuple(float(F(v) * F(scale)) for v in c.min), mx=tuple(float(F(v) * F(scale)) for v in c.max))
        return Built(bytes(b), 0, 7, tuple(256 + j for j in range(7)), (base, 0, 7))
    return make


ROOM_LOOK = (-70.0, -20.0)


def room_camera(scale):
    return tuple(float(F(v) * F(scale)) for v in (-3.3, 1.7, -6.1))


# ---- F5: materials (the twelve spheres and the box are glass: refraction chance 0.9, roughness 0 and 0.5)
BOX_PATCHES = (0, 2, 3, 4, 6)  # the entries of a 12-entry material list that the five glass boxes (cuboids 2 .. 6) receive
MAT_BAD = list(range(12)) + [258, 259, 260, 261, 262]


def f5(patches, n=12, cuboids=False):
    sc = padded(stage(mat=glass, boxes=5), n)
    if cuboids:
        full_cuboids(sc)
    b, _, _ = _blob(sc)
    for i, p in enumerate(patches):
        patch_sphere(b, i, **p)
    for j, k in enumerate(BOX_PATCHES):
        patch_cuboid(b, 2 + j, **patches[k])
    return b, sc


IOR = [dict(ior=v) for v in (0.0, -0.0, 1.0, 0.5, -1.5, DENORMAL, 1e30, 0.0, 1.0, 0.5, -1.5, 1e30)]
ABSORB = [dict(absorbance=v) for v in ((-0.0, -0.0, -0.0), (-0.5, -1.0, -0.25), 1e30, (0.7, 0.7, 0.7), (-0.0, 0.3, 0.0), (1e30, 0.0, 0.1),
                                       (0.2, 0.2, 0.2), (-2.0, -2.0, -2.0), (1.5, 1.5, 1.5), (0.0, -0.0, 0.0), (-0.1, 0.1, 1e30), (3.0, 3.0, 3.0))]
CHANCE = [dict(specular_chance=1.5), dict(specular_chance=-0.5), dict(refraction_chance=1.5), dict(refraction_chance=-0.5),
          dict(specular_chance=0.7, refraction_chance=0.7), dict(specular_chance=2.0, refraction_chance=2.0),
          dict(specular_roughness=1.5, specular_chance=0.6, refraction_chance=0.3), dict(specular_roughness=-0.5, specular_chance=0.6, refraction_chance=0.3),
          dict(refraction_roughness=1.5), dict(refraction_roughness=-0.5), dict(refraction_roughness=3.0, specular_roughness=3.0),
          dict(specular_chance=-1.0, refraction_chance=1.5, refraction_roughness=-1.0)]
LIGHT = [dict(emissiv=(-1.0, -0.5, -2.0)), dict(emissiv=1e38), dict(albedo=0.0), dict(albedo=(1.5, 2.0, 4.0)), dict(emissiv=(-1e38, 1e38, 0.0)),
         dict(albedo=(0.0, 1.0, 8.0)), dict(emissiv=(0.5, -0.5, 0.0), albedo=0.0), dict(albedo=(-1.0, -0.5, 2.0)),
         dict(emissiv=(1e38, 0.0, 0.0), albedo=(2.0, 2.0, 2.0)), dict(albedo=1e30), dict(emissiv=-0.0, albedo=-0.0), dict(albedo=(1e-40, 0.5, 1e38))]


def make_f5(patches):
    def make():
        b, sc = f5(patches)
        return _repaired(sc, b, MAT_BAD)
    return make


# ---- F6: the F1, F3 and F5 sets among 64, 200 and 256 spheres
def make_f6_f1_64():
    b, sc = f1_small(64)
    return _repaired(sc, b, range(12))


def make_f6_plane_64():
    """... with every centre in the plane z = -12: the grid is a few cells thick at most"""
    b, sc = f1_small(64, flat=True)
    assert len({float(s.position[2]) for s in sc.spheres}) == 1
    return _repaired(sc, b, range(12))


def make_f6_f3_200():
    b, sc = f3_spheres(200)
    return _repaired(sc, b, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10])


def make_f6_f5_256():
    b, sc = f5([dict(IOR[i], **ABSORB[i]) for i in range(12)], 256, cuboids=True)
    return _repaired(sc, b, MAT_BAD)


def make_f6_huge_64():
    """a radius of 1e19 among 64 spheres: the builder's `Rg < 1e15` refuses the grid"""
    sc = padded(stage(), 64)
    b, _, _ = _blob(sc)
    patch_sphere(b, 4, radius=1e19)
    return _repaired(sc, b, [4])


# ---- tier N
def make_n_spheres_never():
    """a NaN / +inf / -inf centre component, a NaN, +inf and -inf radius (r^2 = inf: the root is inf - inf): never hit"""
    sc = stage()
    b, _, _ = _blob(sc)
    x, y, z = (float(v) for v in LATTICE[0])
    # (0 and 1 hold the same NaN bits in x and the same z: a sphere run of the default kernels that shares NaN - o.x)
    for i, c in {0: (NAN, y, z), 1: (NAN, INF, z), 2: (x, y, -INF), 4: (-INF, INF, NAN), 6: (INF, 0.0, -12.0)}.items():
        patch_sphere(b, i, centre=c)
    for i, r in {3: NAN, 7: INF, 8: -INF, 10: NAN}.items():
        patch_sphere(b, i, radius=r)
    return _removed(sc, b, [0, 1, 2, 3, 4, 6, 7, 8, 10])


N_BOXES_HIT = [((-INF, -INF, -INF), (-2.0, 0.0, -11.0)),        # semi-infinite: all of min is -inf
               ((1.0, -2.0, -13.0), (INF, 2.0, -11.0)),         # one component of max +inf
               ((-1.5, 1.0, -INF), (0.5, 3.0, -11.0)),          # one component of min -inf
               ((INF, 2.5, -13.0), (6.0, 4.0, -11.0)),          # min.x = +inf: the slab x <= 6
               ((-1.0, -4.0, -13.0), (1.0, -INF, -11.0))]       # max.y = -inf: the slab y <= -4
# a NaN bound: the oracle's min / max return the other operand, so the slab is open on that side and the box IS hit; all of min NaN
N_BOXES_NAN = [((NAN, -3.0, -13.0), (-2.0, 2.0, -11.0)), ((1.0, -2.0, -13.0), (3.5, NAN, -11.0)), ((NAN, NAN, NAN), (6.0, 4.5, -11.0)),
               ((-1.5, -4.0, NAN), (1.5, -2.0, NAN))]
# every bound NaN: t1 = FLOAT_MIN, t2 = FLOAT_MAX for every ray; as the last object it is accepted by every ray ("inside": T = t2 =
# FLOAT_MAX), and RayTrace then reports a miss (compute.glsl:257)
N_BOX_ALL_NAN = [((-1.0, -1.0, -13.0), (1.0, 1.0, -11.0)), ((NAN, NAN, NAN), (NAN, NAN, NAN))]


def mirror(i: int):
    return S.Material(albedo=S.vec3(0.95), specular_chance=1.0, specular_roughness=0.0 if i % 2 else 0.1)


def make_n_mat(patches, behind=False):
    def make():
        sc = stage(mat=mirror, boxes=1) if behind else stage(mat=glass, boxes=5)
        if behind:  # the patched objects behind the camera, large: out of view, reached by bounces only
            for i in range(12):
                x, y, _ = LATTICE[i]
                sc.spheres.append(S.Sphere(np.array([x * 1.5, y * 1.5 + 1.0, -5.0], F), F(2.2), 12 + i, glass(i)))
        b, _, _ = _blob(sc)
        first = 12 if behind else 0
        for i, p in enumerate(patches):
            patch_sphere(b, first + i, **p)
        if not behind:
            for j, k in enumerate(BOX_PATCHES):
                patch_cuboid(b, 2 + j, **patches[k])
        return _repaired(sc, b, [first + i for i in range(len(patches))] + ([] if behind else [258, 259, 260, 261, 262]))
    return make


N_MAT_A = [dict(ior=NAN), dict(ior=INF), dict(ior=-INF), dict(absorbance=(INF, 0.0, -INF)), dict(absorbance=(INF, INF, INF)),
           dict(refraction_roughness=NAN), dict(refraction_roughness=INF), dict(specular_roughness=-INF, specular_chance=0.6),
           dict(specular_chance=NAN), dict(refraction_chance=INF), dict(specular_chance=-INF), dict(refraction_chance=NAN)]
N_MAT_B = [dict(ior=NAN), dict(absorbance=(0.0, NAN, 0.0)), dict(emissiv=(NAN, 0.0, 0.0)), dict(albedo=(1.0, NAN, 1.0)), dict(albedo=INF),
           dict(emissiv=(0.0, INF, 0.0)), dict(emissiv=(-INF, 0.0, 0.0)), dict(albedo=(-INF, 0.5, 0.5)), dict(specular_roughness=NAN, specular_chance=0.6),
           dict(absorbance=(-INF, -INF, -INF)), dict(ior=INF, refraction_roughness=INF), dict(refraction_chance=-INF)]


# out of view: ior +-inf, absorbance (inf, 0, -inf), the non-finite chances and roughnesses of N_MAT_A beside N_MAT_B's NaN absorbance,
# emissive, albedo
N_MAT_BEHIND = [N_MAT_A[k] for k in (1, 2, 3, 6, 8, 9, 10)] + [N_MAT_B[k] for k in (1, 2, 3, 5, 7)]


def make_n_boxes(boxes, removed):
    return make_f4(boxes, removed)


def make_n_behind_geometry():
    """non-finite geometry on objects behind the camera (their finite parts out of view): never hit"""
    sc = stage(mat=mirror)  # (mirrors in view: bounce rays head back past the camera)
    for i in range(4):
        sc.spheres.append(S.Sphere(np.array([-6.0 + 4.0 * i, 0.0, -4.0], F), F(1.75), 12 + i, material(i)))
    sc.cuboids.append(S.Cuboid(np.array([0.0, 4.0, -3.0], F), np.array([12.0, 3.0, 2.0], F), 3, material(1)))
    b, _, _ = _blob(sc)
    patch_sphere(b, 12, radius=NAN)
    patch_sphere(b, 13, centre=(NAN, 0.0, -4.0))
    patch_sphere(b, 14, centre=(2.0, -INF, -4.0))
    patch_sphere(b, 15, centre=(INF, INF, INF))
    patch_cuboid(b, 3, mn=(NAN, NAN, NAN))
    return _removed(sc, b, [12, 13, 14, 15, 259])


def make_past_count(word):
    def make():
        sc = full_cuboids(padded(stage(), 100))
        sc.cuboids = sc.cuboids[:40]
        blob = sc.ubo_bytes()
        return Built(fill_unused(blob, 100, 40, word), 100, 40, (), (fill_unused(blob, 100, 40, 0), 100, 40))
    return make


def make_n_grid_refused():
    sc = padded(stage(), 64)
    b, _, _ = _blob(sc)
    patch_sphere(b, 0, centre=(-4.5, NAN, -12.0))
    patch_sphere(b, 4, centre=(NAN, 0.0, -12.0))
    patch_sphere(b, 7, radius=NAN)
    patch_sphere(b, 11, centre=(4.5, 3.0, INF))
    return _removed(sc, b, [0, 4, 7, 11])


_FH = dict(first_hit=True)
CASES = [
    Case("f1_negative", "F1", make_f1_negative, "hit", **_FH),
    Case("f1_zero", "F1", make_f1_zero, "candidate", still=True, **_FH),
    Case("f1_huge_inside_1e19", "F1", make_f1_huge(1e19, (0.0, 0.0, -8.0)), "hit", **_FH),
    Case("f1_huge_outside_1e19", "F1", make_f1_huge(1e19, (0.0, 0.0, -1.05e19)), "hit", **_FH),
    Case("f1_huge_inside_1e20", "F1", make_f1_huge(1e20, (0.0, 0.0, -8.0), twin=((0.0, 0.0, -8.0), 1e19)), "candidate", still=True, width=8, height=8, **_FH),
    Case("f1_huge_outside_1e20", "F1", make_f1_huge(1e20, (0.0, 0.0, -1.05e20), twin=((0.0, 0.0, -1.05e19), 1e19)), "candidate", still=True, **_FH),
    Case("f2_centre", "F2", make_f2_centre, "hit", position=CAM2_POS, look=CAM2_LOOK, **_FH),
    Case("f2_surface", "F2", make_f2_surface, "hit", position=CAM2_POS, look=CAM2_LOOK, **_FH),
    Case("f2_face", "F2", make_f2_face, "hit", position=CAM2_POS, look=CAM2_LOOK, **_FH),
    Case("f3_spheres", "F3", make_f3_spheres, "hit", ties=True, width=75, height=43, aperture=0.14, **_FH),
    Case("f3_cuboids", "F3", make_f3_cuboids, "hit", ties=True, **_FH),
    Case("f4_flat", "F4", make_f4(FLAT_BOXES), "hit", **_FH),
    Case("f4_flat_oblique", "F4", make_f4(FLAT_BOXES), "hit", position=OBLIQUE_POS, look=OBLIQUE_LOOK, **_FH),
    Case("f4_inverted", "F4", make_f4(INVERTED_BOXES), "hit", **_FH),
    Case("f4_tiny", "F4", make_f4(TINY_BOXES), "hit", **_FH),
    Case("f4_eps_thick", "F4", make_f4(EPS_BOXES), "hit", **_FH),
    Case("f4_eps_thick_oblique", "F4", make_f4(EPS_BOXES), "hit", position=OBLIQUE_POS, look=OBLIQUE_LOOK, **_FH),
    # the 1e-3 thick box seen edge-on through a 0.03 degree lens, 2e-3 of its side face per image height: on the side face the thin
    # axis answers the step too (| |p.y - centre| - half | <= half < EPSILON everywhere on it): normals of two components
    Case("f4_eps_thick_edge", "F4", make_f4([((-2.0, 0.0, -13.0), (2.0, 1e-3, -12.0))]), "hit", q2=True, position=(0.0, 5e-4, -8.0), fov=0.03, **_FH),
    Case("f4_room_1e4", "F4", make_f4_room(1e4), "hit", nan_normals=True, position=room_camera(1e4), look=ROOM_LOOK, **_FH),
    Case("f4_room_1e6", "F4", make_f4_room(1e6), "hit", nan_normals=True, position=room_camera(1e6), look=ROOM_LOOK, **_FH),
    Case("f5_ior", "F5", make_f5(IOR), "bounce"),
    Case("f5_absorbance", "F5", make_f5(ABSORB), "bounce", env="sky_srgb_32"),
    Case("f5_chances", "F5", make_f5(CHANCE), "bounce"),
    Case("f5_light", "F5", make_f5(LIGHT), "bounce", aperture=0.14),
    Case("f6_f1_64", "F6", make_f6_f1_64, "hit", grid=True, **_FH),
    Case("f6_plane_64", "F6", make_f6_plane_64, "hit", grid=True, **_FH),
    Case("f6_f3_200", "F6", make_f6_f3_200, "hit", grid=True, ties=True, **_FH),
    Case("f6_f5_256", "F6", make_f6_f5_256, "bounce", grid=True),
    Case("f6_huge_64", "F6", make_f6_huge_64, "hit", grid=False, **_FH),
    Case("n_spheres_never", "N", make_n_spheres_never, "candidate", still=True, **_FH),
    Case("n_boxes_hit", "N", make_n_boxes(N_BOXES_HIT, False), "hit", **_FH),
    Case("n_boxes_nan", "N", make_n_boxes(N_BOXES_NAN, False), "hit", width=75, height=43, **_FH),
    Case("n_box_all_nan", "N", make_n_boxes(N_BOX_ALL_NAN, False), "hit", **_FH),
    Case("n_mat_a", "N", make_n_mat(N_MAT_A), "bounce"),
    Case("n_mat_b", "N", make_n_mat(N_MAT_B), "bounce", width=8, height=8),
    Case("n_mat_behind", "N", make_n_mat(N_MAT_BEHIND, behind=True), "bounce"),
    Case("n_behind_geometry", "N", make_n_behind_geometry, "none", still=True, **_FH),
    Case("n_past_count_nan", "N", make_past_count(0x7FC00000), "none", still=True, grid=True),
    Case("n_past_count_inf", "N", make_past_count(0xFF800000), "none", still=True, grid=True),
    Case("n_grid_refused", "N", make_n_grid_refused, "candidate", still=True, grid=False, **_FH),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
STILL = [c.name for c in CASES if c.still]  # the image must equal the base scene's exactly
TIER_F = [c for c in CASES if c.tier == "F"]
TIER_N = [c for c in CASES if c.tier == "N"]
