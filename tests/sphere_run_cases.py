"""Sphere layouts for the run sharing of the default kernels' in-order sphere loop (ray_trace_t<..., SHARE>, csrc/pt_device.hpp: a sphere
whose centre has the same x AND z bits as its predecessor reuses o.x - c.x, o.z - c.z, d.x * oc.x and oc.x^2), shared by
test_sphere_runs_cpu.py and test_gpu_sphere_runs.py.

A layout is a list of (x index, z level, count): `count` spheres with bit-equal x and z, stacked in y — one run of the loop, unless the
entry before it has the same x and z.  The suite's other scenes only ever have the default lattice's runs (6,6,6,6,6,6,2,2,2,2,2,2 at 48
spheres, equal z and different x at every boundary); the cases here have runs of every length from 1 to 63, boundaries of all three kinds
(x differs, z differs, both differ), counts that are no multiple of 4 (the loop takes four spheres per step and the last ns % 4 on their
own) and runs across the 32-sphere words the kernel reads the bits in.

expected_runs() is the run rule restated in plain Python; plan() asks the library which kernel a launch would take (pt_debug_plan_launch).
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402
import configs  # noqa: E402
from test_launch_plan import MULTISAMPLE, PERSISTENT, plan as plan_launch  # noqa: E402  (the structs of pt_debug_plan_launch live there)

pkg = graft.load_package()
F = np.float32
S = pkg.scene

XS = tuple(F(S.default_scene().spheres[6 * k].position[0]) for k in range(6))  # the six column x values of the default scene
ZS = (F(-5.0), F(-6.4), F(-7.8))
POSITION, LOOK, FOCAL_LENGTH, APERTURE = (-1.0, -0.5, -17.0), (90.0, 0.0), 12.0, 0.1
WIDTH, HEIGHT, DEPTH, ENV = 128, 72, 6, "sky_f32_32"


def material(i: int):
    """Varies per sphere: diffuse to mostly specular in four steps, three roughnesses, every seventh sphere absorbing glass."""
    if i % 7 == 3:
        return S.Material(albedo=S.vec3(1.0), absorbance=(S.vec3(0.3, 0.6, 0.9) * F((i % 5 + 1) / 5)).astype(F), specular_chance=0.02, ior=1.3,
                          refraction_chance=0.9, refraction_roughness=0.05)
    palette = [(0.59, 0.59, 0.99), (0.9, 0.25, 0.25), (0.3, 0.85, 0.35), (0.95, 0.9, 0.3), (0.8, 0.8, 0.8)]
    return S.Material(albedo=S.vec3(*palette[i % 5]), specular_chance=(i % 4) / 4, specular_roughness=(i % 3) / 3)


def layout(runs, xs=XS):
    """-> Scene: every (x index, z level, count) of `runs` becomes one column of `count` spheres at x = xs[x index], z = ZS[z level] — the
    same bits for the whole column —, radius 0.8 (0.33 for counts above 13), y = -11 + 2.1 r k + 0.5 z level with k = the number of spheres
    already placed at that (x, z); in the default room."""
    sc = S.Scene()
    placed = {}
    for xi, zl, count in runs:
        x, z = F(xs[xi]), ZS[zl]
        r = F(0.8) if count <= 13 else F(0.33)
        for _ in range(count):
            k = placed.get((float(x), zl), 0)  # (+0.0 and -0.0 share a slot: two columns at equal values never coincide)
            placed[(float(x), zl)] = k + 1
            y = F(-11.0) + F(2.1) * r * F(k) + F(0.5) * F(zl)
            i = len(sc.spheres)
            sc.spheres.append(S.Sphere(np.array([x, y, z], dtype=F), r, i, material(i)))
    sc.cuboids = S.default_cuboids()
    return sc


@dataclass
class Case:
    name: str
    runs: list
    xs: tuple = XS

    def scene(self):
        return layout(self.runs, self.xs)

    @property
    def num_spheres(self) -> int:
        return sum(c for _, _, c in self.runs)


def one_run(ns: int) -> Case:
    return Case(f"one_run{ns}", [(2, 1, ns)])


def tiny(ns: int) -> Case:
    return Case(f"tiny{ns}", [(3, 0, ns)])


def words_2_to_7(ns: int) -> Case:
    """ns >= 64 spheres for a renderer without sphere grid (knob no_sphere_grid): a run of 6, then runs of 12 — boundaries at 6 + 12 j, so
    that a run lies across every multiple of 32 below ns (30-42, 54-66, 90-102, 126-138, 150-162, 186-198, 222-234).  The first twelve
    boundaries alternate between "z differs, x equal" and "x differs, z equal"."""
    assert 64 <= ns <= 256
    slots = [(k // 2 + k % 2, (k // 2) % 3) if k % 2 == 0 else (k // 2, (k // 2 + 1) % 3) for k in range(12)]
    slots += [s for s in ((xi, zl) for xi in range(6) for zl in range(3)) if s not in slots]
    runs, left = [], ns
    while left > 0:
        n = min(left, 6 if not runs else 12)
        runs.append(slots[len(runs) % len(slots)] + (n,))
        left -= n
    return Case(f"words_2_to_7_n{ns}", runs)


NAMED = [
    Case("mixed47", [(0, 0, 1), (0, 1, 2), (1, 1, 3), (1, 0, 4), (2, 1, 5), (2, 2, 7), (3, 2, 8), (4, 0, 9), (4, 1, 8)]),
    Case("long63", [(1, 0, 31), (1, 1, 2), (3, 1, 30)]),
    Case("pairs19", [(0, 0, 2), (0, 1, 2), (1, 1, 2), (1, 0, 2), (2, 0, 2), (3, 1, 2), (3, 2, 2), (4, 2, 2), (5, 0, 2), (5, 1, 1)]),
    Case("cross43", [(0, 0, 30), (2, 0, 4), (2, 1, 3), (4, 2, 6)]),
    Case("n61", [(0, 0, 5), (0, 1, 9), (1, 1, 3), (2, 0, 12), (2, 1, 1), (3, 1, 1), (3, 2, 7), (4, 0, 6), (5, 0, 4), (5, 1, 13)]),
]
NO_RUNS = Case("no_runs", [(2 + i % 2, (i // 2) % 3, 1) for i in range(48)])  # x alternates every sphere
# a column at x = +0.0, then one at x = -0.0 with the same z: equal values, different bits — NOT a run
SIGNED_ZERO = Case("signed_zero", [(0, 0, 5), (1, 0, 4), (2, 1, 3), (0, 1, 2), (1, 1, 3)], xs=(F(0.0), F(-0.0), XS[1]))
ONE_RUN = [one_run(n) for n in (4, 5, 6, 7, 63)]
TINY = [tiny(n) for n in (1, 2, 3)]
WITH_BOUNDARIES = NAMED + [NO_RUNS, SIGNED_ZERO]
WITHOUT_BOUNDARIES = ONE_RUN + TINY
CASES = WITH_BOUNDARIES + WITHOUT_BOUNDARIES  # (+ the words_2_to_7 cases of the counts words_counts() finds)
BY_NAME = {c.name: c for c in CASES}


def expected_runs(blob: bytes, ns: int) -> int:
    """The run rule, restated: bit i of the 256 is CLEAR when sphere i's x and z words equal sphere i - 1's bit for bit; bit 0 and the
    bits at and beyond ns are always set."""
    w = np.frombuffer(blob, dtype=np.uint32)
    bits = (1 << 256) - 1
    for i in range(1, min(ns, 256)):
        if w[20 * i] == w[20 * (i - 1)] and w[20 * i + 2] == w[20 * (i - 1) + 2]:
            bits &= ~(1 << i)
    return bits


def boundaries(blob: bytes, ns: int) -> list:
    """The spheres after the first that start a run."""
    bits = expected_runs(blob, ns)
    return [i for i in range(1, ns) if bits >> i & 1]


def with_centre_words(blob: bytes, i: int, x=None, y=None, z=None, radius=None) -> bytes:
    """The blob with words of sphere i's float4 (centre, radius) replaced (uint32 bit patterns or float32 values)."""
    w = np.frombuffer(blob, dtype=np.uint32).copy()
    for k, v in enumerate((x, y, z, radius)):
        if v is not None:
            w[20 * i + k] = v if isinstance(v, (int, np.integer)) else np.array([v], dtype=F).view(np.uint32)[0]
    return w.tobytes()


def shares_wrongly(blob: bytes, i: int) -> bytes:
    """What a wrongly CLEARED run bit i computes: sphere i evaluated with sphere i - 1's x and z."""
    w = np.frombuffer(blob, dtype=np.uint32)
    return with_centre_words(blob, i, x=int(w[20 * (i - 1)]), z=int(w[20 * (i - 1) + 2]))


def camera_ubo(width: int = WIDTH, height: int = HEIGHT) -> bytes:
    cam = pkg.camera.Camera(position=POSITION, look_x=LOOK[0], look_y=LOOK[1])
    return pkg.camera.basic_data_ubo(cam, width, height)


def oracle_kwargs(sc, depth: int = DEPTH, spp: int = 1) -> dict:
    return dict(num_spheres=sc.num_spheres, num_cuboids=sc.num_cuboids, ray_depth=depth, spp=spp, focal_length=FOCAL_LENGTH, aperture=APERTURE)


def env():
    return configs.load_env(ENV)


# ---- which kernel a launch of these cases takes (pt_debug_plan_launch through tests/test_launch_plan.py)
# Which instantiations share runs (template argument SHARE = MATLDS && !GRID of bounce_step_t): the spp = 1 branch of the persistent kernel
# with materials in LDS and no grid (rows 0 - 5) and the multisample kernel's row 0.  The spp > 1 branch of the persistent kernel (row 10:
# the in-lane sample chain) does NOT: it runs the plain loop and never reads the run bits.
SHARING_ROWS = {(PERSISTENT, r) for r in range(6)} | {(MULTISAMPLE, 0)}
GRID_OFF = dict(noSphereGrid=1, hasGrid=1, gridBytes=1024)  # a scene the host has built a grid for, launched with the knob no_sphere_grid


def launch_forms(width: int, height: int, spp: int, frames: int):
    """The ways frames of a default-variant handle reach the GPU (choose_launch_mode, launch_striped, launch_single_stream in
    csrc/mi355pt_launch.cpp), as plan inputs without the scene: -> {name: dict}.
      striped    one frame on an idle handle that has not pipelined yet: untagged; two row stripes, each a launch of its own without drain
                 compaction — or, with fewer than 32 rows, ONE launch with drain compaction (32)
      pipelined  `frames` consecutive frames in one tagged launch over the whole image (also single frames, when the GPU is still busy
                 with the handle's earlier ones or the handle has pipelined before); no drain compaction
    All run five workgroups per CU (variant 14).  This is a restatement, tied to the host only by reading it: the GPU tests compare
    images and cannot tell which row ran."""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    common = dict(width=width, height=height, tilesX=tx, spp=spp, envFormat=0, variant=14, numCUs=256, hasStartedFlags=1,
                  parkedMax=-1, parkCapacity=-1, parkMin=40, batchPassMinTiles=16384, carryLast=1)
    stripes = 2 if height >= 32 else 1
    forms = {}
    for j in range(stripes):
        r0, r1 = (height * j // stripes) & ~7, height * (j + 1) // stripes
        if j + 1 < stripes:
            r1 &= ~7
        forms[f"striped{j}"] = dict(common, tilesY=(r1 - r0 + 7) // 8, batchFrames=1, tagged=0, queueChunk=8, drainCompaction=0 if stripes > 1 else 32)
    for n in sorted({1, frames}):
        forms[f"pipelined{n}"] = dict(common, tilesY=ty, batchFrames=n, tagged=1, queueChunk=4 if n > 1 and tx * ty < 12000 else 8, drainCompaction=0)
    return forms


def plan(lib, form: dict, num_spheres: int, num_cuboids: int = 7, **knobs) -> dict:
    """plan_launch's answer for one launch form of a scene with that many objects; knobs: batchPassMinTiles, and GRID_OFF."""
    fields = dict(dict.fromkeys(["numSpheres", "numCuboids", "tagged", "drainCompaction", "queueChunk", "gridBytes", "hasGrid", "hasTimeline", "hasStartedFlags",
                                 "hasFeed", "wantFeed", "noBatchPass", "noSphereGrid", "forceLeanLds", "gridCarry"], 0), **form)
    return plan_launch(lib, dict(fields, numSpheres=num_spheres, numCuboids=num_cuboids, **knobs))


def largest_count_with_materials_in_lds(lib, forms: dict, lo: int = 64, hi: int = 256, **knobs) -> int:
    """The largest sphere count n in [lo, hi] such that, for every count from lo to n, every one of the given launch forms still runs a
    kernel with the materials in LDS and without sphere grid when the grid is switched off (GRID_OFF).  0: none."""
    best = 0
    for ns in range(lo, hi + 1):
        for form in forms.values():
            p = plan(lib, form, ns, **GRID_OFF, **knobs)
            if not (p["error"] == 0 and p["matLds"] == 1 and p["grid"] == 0):
                return best
        best = ns
    return best


def words_counts(lib) -> dict:
    """The words_2_to_7 counts, one per way test_gpu_sphere_runs.py renders that case — each the largest count that keeps the materials
    in LDS for the launch forms THAT rendering can take:
      pipelined    four back-to-back frames at spp 1: the first goes out striped, the rest as single tagged frames or one tagged launch
      striped      four frames at spp 1 with the handle drained after each: untagged row stripes only
      batch_pass   spp 3 with batch_pass_min_tiles = 0: the multisample kernel, striped or pipelined"""
    spp1, spp3 = launch_forms(WIDTH, HEIGHT, 1, 4), launch_forms(WIDTH, HEIGHT, 3, 3)
    return {"pipelined": largest_count_with_materials_in_lds(lib, spp1),
            "striped": largest_count_with_materials_in_lds(lib, {k: v for k, v in spp1.items() if k.startswith("striped")}),
            "batch_pass": largest_count_with_materials_in_lds(lib, spp3, batchPassMinTiles=0)}
