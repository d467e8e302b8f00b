"""Shared by tests/test_first_hit_abi.py (CPU) and tests/test_gpu_first_hit.py (GPU): the cases of the first-hit query and the ORACLE'S
OWN first-hit id per pixel, obtained from the frozen oracle without touching it.

The trick: in a copy of the scene blob object k's Emissiv becomes (k + 1, 0, 0) (bytes 32-43 of a sphere, 48-59 of a cuboid; k in the
id order of include/mi355pt.h: sphere i = i, cuboid j = PT_MAX_SPHERES + j).  One oracle frame at ray_depth 1, spp 1 onto a zeroed
image against an all-zero environment then leaves R = (k + 1) / (f + 1) in the red channel of a pixel whose first hit is object k (the
throughput is 1 at the first hit; Beer's law only applies inside an ABSORBING object, and no case puts a ray origin into one — which
the soundness test checks rather than assumes), and 0 on a miss: id = rint(R (f + 1)) - 1.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass

import numpy as np

import configs

pkg = configs.pkg
PT_MAX_SPHERES = 256
FLOAT_MAX = np.float32(3.4028235e38)
DEFAULT_POS, DEFAULT_LOOK = (-17.14, 3.53, -8.62), (-32.2, 0.8)


@dataclass(frozen=True)
class Case:
    name: str
    scene: str            # default | full | edge | empty
    width: int
    height: int
    frame: int = 0
    aperture: float = 0.14
    focal_length: float = 20.0
    position: tuple = DEFAULT_POS
    look: tuple = DEFAULT_LOOK


def full_ubo_scene():
    """Every slot of the GameObjectsUBO in use: the 256 stress spheres and 64 cuboids (the room's 7 + 57 small boxes in front of it)."""
    s = pkg.scene
    sc = s.stress_scene(256)
    for j in range(57):
        pos = s.vec3(-17.0 + 2.0 * (j % 19), -9.0 + 5.0 * (j // 19), -3.0 - 0.25 * (j % 5))
        sc.cuboids.append(s.Cuboid(pos, s.vec3(0.9, 0.7 + 0.1 * (j % 4), 0.8), len(sc.cuboids), s.Material(albedo=s.vec3(0.5))))
    assert sc.num_spheres == 256 and sc.num_cuboids == 64
    return sc


def make_scene(kind: str):
    return full_ubo_scene() if kind == "full" else configs.make_scene(kind)


# the cases of the issue: default scene 75x43 (ragged tiles), 8x8, 1x1; frames 0, 1, 977; aperture 0, 0.14, 2.0; the full UBO at 64x36;
# the `edge` scene's camera (origin inside sphere 0: the entry-distance quirk); a camera inside cuboid 6 (the room's middle box: centre
# (-15, -10.495, -15), 3 x 6 x 3); zero objects
CASES = [
    Case("default_75x43_f0", "default", 75, 43, frame=0),
    Case("default_75x43_f1", "default", 75, 43, frame=1),
    Case("default_75x43_f977", "default", 75, 43, frame=977),
    Case("default_8x8", "default", 8, 8),
    Case("default_1x1", "default", 1, 1),
    Case("default_75x43_ap0", "default", 75, 43, frame=1, aperture=0.0),
    Case("default_75x43_ap2", "default", 75, 43, frame=1, aperture=2.0),
    Case("full_64x36", "full", 64, 36, frame=3),
    Case("edge_64x36", "edge", 64, 36, frame=2),
    Case("incuboid_64x36", "default", 64, 36, frame=5, position=(-15.0, -10.0, -15.0), look=(20.0, 10.0)),
    Case("empty_16x9", "empty", 16, 9),
    # a camera whose InvView translation column equals ViewPos bit for bit (the float64 inverse of the host happens to round-trip): the
    # ray origin IS that column (compute.glsl:120), so "origin == ViewPos" can only be asked of such a blob
    Case("default_64x36_ap0_cam2", "default", 64, 36, aperture=0.0, position=(5.0, 2.0, -3.0), look=(20.0, -10.0)),
]
BY_NAME = {c.name: c for c in CASES}
REPLAY_CASES = ("default_8x8", "full_64x36")  # the full visiting-order replay (320 oracle calls per pixel at 64x36)


def inputs(case: Case):
    """-> (scene blob bytes, num_spheres, num_cuboids, basic blob bytes)"""
    sc = make_scene(case.scene)
    cam = pkg.camera.Camera(position=case.position, look_x=case.look[0], look_y=case.look[1])
    return sc.ubo_bytes(), sc.num_spheres, sc.num_cuboids, pkg.camera.basic_data_ubo(cam, case.width, case.height)


def id_emissive_blob(blob: bytes, ns: int, nc: int) -> bytes:
    b = bytearray(blob)
    for i in range(ns):
        struct.pack_into("<3f", b, 80 * i + 32, float(i + 1), 0.0, 0.0)
    for j in range(nc):
        struct.pack_into("<3f", b, 20480 + 96 * j + 48, float(PT_MAX_SPHERES + j + 1), 0.0, 0.0)
    return bytes(b)


_decoded = {}


def oracle_first_hit(oracle, case: Case):
    """-> (id (H, W) int32, residual (H, W) float64 = |R (f + 1) - rint|).  Computed once per case."""
    if case.name not in _decoded:
        blob, ns, nc, basic = inputs(case)
        img = oracle.render(case.width, case.height, basic, id_emissive_blob(blob, ns, nc), np.zeros((6, 2, 2, 4), np.float32),
                            num_spheres=ns, num_cuboids=nc, ray_depth=1, spp=1, focal_length=case.focal_length, aperture=case.aperture,
                            frame_start=case.frame, num_frames=1)
        v = img[..., 0].astype(np.float64) * (case.frame + 1)
        ids = (np.rint(v) - 1).astype(np.int32)
        ids.setflags(write=False)
        _decoded[case.name] = (ids, np.abs(v - np.rint(v)))
    return _decoded[case.name]


class Replayer:
    """The reference's RayTrace (compute.glsl:226-258) re-run in Python on the oracle's function-level ray_sphere / ray_cuboid (the calls
    of tests/test_oracle_vs_reference.py, here through preconverted pointers: a 64x36 replay of the full UBO is 737,280 of them)."""

    def __init__(self, oracle, blob: bytes, ns: int, nc: int):
        self.L, self.ns, self.nc = oracle.lib, ns, nc
        f = np.frombuffer(blob, np.float32)
        fp = C.POINTER(C.c_float)
        self._keep = []

        def ptr(a):
            a = np.ascontiguousarray(a, np.float32)
            self._keep.append(a)
            return a.ctypes.data_as(fp)
        self.sph = [ptr(f[20 * i:20 * i + 4]) for i in range(ns)]
        self.cub = [(ptr(f[5120 + 24 * j:5120 + 24 * j + 3]), ptr(f[5120 + 24 * j + 4:5120 + 24 * j + 7])) for j in range(nc)]
        self.o, self.d, self.t = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32)
        self.op, self.dp, self.tp = (a.ctypes.data_as(fp) for a in (self.o, self.d, self.t))

    def set_ray(self, o, d):
        self.o[:] = o
        self.d[:] = d

    def leaf(self, obj_id: int):
        """-> (hit, t1, t2) of object `obj_id` (first-hit id numbering) for the ray set last."""
        if obj_id < PT_MAX_SPHERES:
            hit = self.L.pto_ray_sphere(self.op, self.dp, self.sph[obj_id], self.tp)
        else:
            mn, mx = self.cub[obj_id - PT_MAX_SPHERES]
            hit = self.L.pto_ray_cuboid(self.op, self.dp, mn, mx, self.tp)
        return bool(hit), self.t[0], self.t[1]

    def trace(self):
        """-> (winner id or -1, T): every sphere, then every cuboid, with the reference's acceptance rule."""
        T, winner = FLOAT_MAX, -1
        for k in list(range(self.ns)) + [PT_MAX_SPHERES + j for j in range(self.nc)]:
            hit, t1, t2 = self.leaf(k)
            if hit and t2 > 0.0 and t1 < T:
                T = t2 if t1 < 0.0 else t1
                winner = k
        return winner, T


def make_tracer(case: Case, env=None, ray_depth: int = 1, **extra):
    """A PathTracer with the case's scene, camera and lens uploaded (no environment unless one is given)."""
    blob, ns, nc, basic = inputs(case)
    pt = pkg.PathTracer(env, case.width, case.height, ray_depth, 1, case.focal_length, case.aperture, **extra)
    objs = np.frombuffer(blob, dtype=np.uint8)
    pt.GameObjectsUBO.SubData(0, objs.nbytes, objs)
    pt._numSpheres, pt._numCuboids = ns, nc
    pt._push_params()
    pt.UploadBasicData(basic)
    return pt
