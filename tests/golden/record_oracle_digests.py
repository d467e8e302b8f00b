"""Before/after pin of the CPU oracle: SHA-256 digests of the raw output bytes of every entry point of every oracle library.

    python tests/golden/record_oracle_digests.py --oracle-dir DIR      # DIR holds pt_oracle.py, the sources and the Makefile

records tests/golden/oracle_digests.json from the oracle under DIR; tests/test_oracle_digests.py asserts that the tree's own oracle
reproduces every digest.  The committed fixture was recorded from the oracle as it stood BEFORE oracle/pt_oracle.c was split into the
contract and the study builds (git archive <parent> oracle | tar -x -C DIR), never from the split sources: it is what "the split changes
no bit" means.  To re-record after a deliberate change of the arithmetic, run it on the tree's oracle/ and say so in the commit.

The fixture holds names and hex digests only.  One exception to "raw bytes": pto_list_close_decisions reports the SOURCE LINE of each
comparison, which moves with every edit of the file; it is digested as the ordinal of that comparison among the file's DECIDE sites.
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import hashlib
import importlib.util
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "oracle_digests.json")
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

KINDS = {"contract": {}, "truediv": dict(true_division=True), "exact": dict(exact=True), "nanmark": dict(mark_nan_env=True),
         "margins": dict(margins=True), "perturb": dict(perturb=True)}
# pto_set_base_variant: llvmpipe's two sets, then every bit and every value of the two order fields on its own
LLVMPIPE = 951   # pt_oracle.LLVMPIPE (spelled out: this script also runs against oracles from before the constant existed)
BASE_VARIANTS = (7, LLVMPIPE, 1, 2, 4, 128, 256, 512, 8, 16, 24, 32, 64)
THREADS = 4
BAND = 1e-4
TIGHT_BAND = 2e-7   # (the searches: about an ulp, so that values a few ulps apart count as different and the later stages run)

_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int)


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def workloads():
    import configs
    by_name = {w.name: w for w in configs.SMALL_FRAMES}
    rep = dataclasses.replace
    return [rep(by_name["default_64_d4"], name="default_48x27_d4", width=48, height=27, frames=2),
            rep(by_name["default_96x54_d13_spp4"], name="default_40x23_d13_spp2", width=40, height=23, spp=2, frames=2),
            rep(by_name["edge_128x72_d16"], name="edge_48x27_d16", width=48, height=27, frames=2)]


def scene_args(w):
    import configs
    _, basic, objs, env, kw = configs.inputs(w)
    return (w.width, w.height, basic, objs, env), kw


def atmosphere_case():
    import configs
    cam = configs.pkg.camera
    return 16, cam.atmospheric_data_ubo(), cam.atmosphere_light_pos(0.5), 15.0, 8, 3


def post_ramp():
    """256 values x RGBA: a ramp through negative, [0, 1] and > 1 inputs, plus NaN, infinities, zeros and denormals"""
    v = np.concatenate([np.linspace(-0.5, 1.0, 128, dtype=np.float32), np.geomspace(1e-6, 64.0, 118).astype(np.float32),
                        np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 0.0031308, 0.0031307, 1.0, 65504.0], np.float32)])
    assert v.size == 256
    img = np.stack([v, v[::-1], np.roll(v, 85), np.ones_like(v)], axis=-1)
    return np.ascontiguousarray(img, np.float32)


def render_digests(o, out, prefix, ws, atmosphere=True, post=False):
    """frames (every frame of the accumulation, with the statistics) + listed pixels of frame 1 + atmosphere (+ post-process)"""
    for w in ws:
        scene, kw = scene_args(w)
        frames, st = o.render(*scene, num_frames=w.frames, threads=THREADS, dump_each=True, want_stats=True, **kw)
        out[f"{prefix}/render_frame/{w.name}"] = sha(frames, np.array(sorted(st.items()), dtype="U32"))
        rng = np.random.default_rng(17)
        xy = np.stack([rng.integers(0, w.width, 24), rng.integers(0, w.height, 24)], axis=-1).astype(np.int32)
        last = frames[0][xy[:, 1], xy[:, 0]]
        out[f"{prefix}/render_pixels/{w.name}"] = sha(o.render_pixels(*scene, xy, frame=1, last=last, **kw))
    if atmosphere:
        size, ubo, lp, inten, i_steps, j_steps = atmosphere_case()
        out[f"{prefix}/atmosphere/16"] = sha(o.atmosphere(size, ubo, lp, inten, i_steps, j_steps, threads=THREADS))
    if post:
        out[f"{prefix}/postprocess/ramp256"] = sha(*o.postprocess(post_ramp()))


def bounce_counts(o, w):
    scene, kw = scene_args(w)
    basic, objs, env = o._inputs(*scene[2:])
    p = o._params(w.width, w.height, kw["num_spheres"], kw["num_cuboids"], kw["ray_depth"], kw["spp"], kw["focal_length"], kw["aperture"], env)
    counts = np.zeros((w.height, w.width), np.int32)
    fn = o.lib.pto_bounce_counts
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, _fp, _fp, C.c_void_p, C.c_int, _ip]
    assert fn(C.byref(p), basic.ctypes.data_as(_fp), objs.ctypes.data_as(_fp), env.ctypes.data_as(C.c_void_p), 1, counts.ctypes.data_as(_ip)) == 0
    return counts


def micro_digests(o, out, prefix):
    """the array and micro entry points on seeded arguments"""
    import configs
    rng = np.random.default_rng(23)
    f32 = np.float32
    wide = np.concatenate([(rng.standard_normal(3072) * np.exp(rng.uniform(-60, 60, 3072))).astype(f32),
                           rng.integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32).view(f32),
                           np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.17549435e-38] * 3, f32)])
    out[f"{prefix}/micro/rcp_rsqrt_sqrt"] = sha(o.rcp(wide), o.rsqrt(wide), o.sqrt(wide))
    ang = np.concatenate([rng.uniform(0, 2 * np.pi, 200), rng.uniform(-40, 40, 56)]).astype(f32)
    out[f"{prefix}/micro/sincos"] = sha(np.array([o.sincos(a) for a in ang], f32))
    xs = np.concatenate([rng.uniform(-110, 90, 250), [np.nan, np.inf, -np.inf, 0.0, 88.8, -104.5]]).astype(f32)
    out[f"{prefix}/micro/exp"] = sha(np.array([o.exp(x) for x in xs], f32))
    pos = np.abs(wide[:256])
    out[f"{prefix}/micro/log_pow5"] = sha(np.array([o.log(x) for x in pos], f32), np.array([o.pow5(x) for x in rng.uniform(-0.1, 1.1, 256).astype(f32)], f32))
    out[f"{prefix}/micro/rng"] = sha(o.rand_stream(12345, 64), o.hash_stream(777, 64), np.array([o.pixel_seed(x, y, f) for x, y, f in rng.integers(0, 4000, (32, 3))], np.uint32),
                                     np.array([o.lib.pto_srgb_to_linear(v) for v in range(256)], f32))
    unit = rng.standard_normal((96, 3)).astype(f32)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True).astype(f32)
    org = rng.uniform(-6, 6, (96, 3)).astype(f32)
    res = []
    for k in range(96):
        d = unit[k].copy()
        if k % 8 == 0:
            d[k % 3] = 0.0   # axis-parallel rays: infinite slab distances
        sph = np.array([*rng.uniform(-4, 4, 3), rng.uniform(0.2, 5.0)], f32)
        mn = rng.uniform(-5, 0, 3).astype(f32)
        mx = (mn + rng.uniform(0.1, 6, 3)).astype(f32)
        res.append([*o.ray_sphere(org[k], d, sph), *o.ray_cuboid(org[k], d, mn, mx)])
        p = (mn + (mx - mn) * rng.integers(0, 2, 3) + rng.uniform(-2e-3, 2e-3, 3) * (k % 2)).astype(f32)
        res.append([*o.cuboid_normal(mn, mx, p), 0.0, 0.0, 0.0])
    out[f"{prefix}/micro/intersect"] = sha(np.array(res, f32))
    res = []
    for k in range(96):
        i, n = unit[k], unit[95 - k]
        eta = f32(rng.choice([1.5, 1 / 1.5, 1.3, 1 / 1.3, 1.0]))
        v, s = o.cosine_sample_hemisphere(n, int(rng.integers(1, 2 ** 31)))
        res.append([*o.refract(i, n, eta), *o.reflect(i, n), *v, f32(s & 0xFFFF), *o.normalize(org[k]),
                    o.fresnel_schlick(float(abs(i @ n)), 1.0, float(eta)), o.fresnel_schlick(float(-abs(i @ n)) * 1e-7, float(eta), 1.0)])
    res.append([*o.normalize(np.zeros(3, f32))] + [0.0] * 12)
    out[f"{prefix}/micro/shading"] = sha(np.array(res, f32))
    dirs = np.concatenate([unit[:64], np.array([[1, 1, 1], [-1, 1, 1], [1, 0, 0], [0, 0, -1], [np.nan, 0, 1], [1, -1, 1e-9]], f32)])
    for key in ("tiny_2", "sky_f32_32", "sky_srgb_32"):
        env = configs.load_env(key)
        out[f"{prefix}/micro/sample_env/{key}"] = sha(np.array([o.sample_env(env, d) for d in dirs], f32))


def study_calls(o, w):
    """raw calls of the study entry points with one pixel of `w`: the values a library that does not implement them returns"""
    scene, kw = scene_args(w)
    basic, objs, env = o._inputs(*scene[2:])
    p = o._params(w.width, w.height, kw["num_spheres"], kw["num_cuboids"], kw["ray_depth"], kw["spp"], kw["focal_length"], kw["aperture"], env)
    head = (C.byref(p), basic.ctypes.data_as(_fp), objs.ctypes.data_as(_fp), env.ctypes.data_as(C.c_void_p))
    L = o.lib
    L.pto_list_close_decisions.restype = C.c_int
    L.pto_list_close_decisions.argtypes = [C.c_void_p, _fp, _fp, C.c_void_p, C.c_int, C.c_int, C.c_int, _fp, C.c_float, C.c_int, _fp]
    L.pto_llvmpipe_like.restype = C.c_int
    L.pto_llvmpipe_like.argtypes = [C.c_int, _fp, _fp, C.c_int, _fp]
    L.pto_set_ensemble.restype, L.pto_set_ensemble.argtypes = C.c_int, [C.c_uint, C.c_int]
    return head, L


def stub_digests(o, kind, out, w):
    head, L = study_calls(o, w)
    last, buf = np.zeros(4, np.float32), np.zeros(64, np.float32)
    ibuf = np.full(128, -1, np.int32)
    fp, ip = lambda a: a.ctypes.data_as(_fp), lambda a: a.ctypes.data_as(_ip)
    vals = {}
    if kind != "perturb":
        one = np.ones(4, np.float32)
        vals["set_perturbation"] = L.pto_set_perturbation(0, 1)
        vals["set_unfused"] = L.pto_set_unfused(1)
        vals["set_base_variant"] = L.pto_set_base_variant(LLVMPIPE)
        vals["llvmpipe_like"] = L.pto_llvmpipe_like(0, fp(one), fp(one), 4, fp(buf))
        vals["set_signature_alpha"] = L.pto_set_signature_alpha(1)
        vals["list_close_decisions"] = L.pto_list_close_decisions(*head, 3, 4, 0, fp(last), 1e-3, 16, fp(buf))
        vals["set_ensemble"] = L.pto_set_ensemble(5, 16)
        vals["set_nan_env"] = L.pto_set_nan_env(fp(one))
        vals["render_pixel_variant"] = L.pto_render_pixel_variant(*head, 3, 4, 0, fp(last), ip(ibuf), 0, ip(ibuf[8:]), 0, fp(buf))
        ns = C.c_int(0)
        vals["witness_search"] = L.pto_witness_search(*head, 3, 4, 0, fp(last), fp(one), BAND, 1e-6, 8, ip(ibuf), ip(ibuf[8:]), C.byref(ns), ip(ibuf[120:]), fp(buf))
        vals["study_calls_wrote"] = sha(buf, ibuf)
    if kind != "margins":
        img = np.zeros((w.height, w.width, 4), np.float32)
        m = np.full((w.height, w.width, 2), 7.0, np.float32)
        vals["render_frame_margins"] = L.pto_render_frame_margins(*head[:4], fp(img), 0, w.height, 0, THREADS, fp(m))
        vals["render_frame_margins_wrote"] = sha(img, m)
        scene, kw = scene_args(w)
        xy = np.array([[3, 4], [20, 11], [47, 26]], np.int32)
        vals["render_pixels_margins"] = sha(*o.render_pixels_margins(*scene, xy, **kw))
    out[f"{kind}/stubs"] = hashlib.sha256(json.dumps(vals, sort_keys=True).encode()).hexdigest()
    print(f"  {kind}: study entry points return {({k: v for k, v in vals.items() if isinstance(v, int)})}", file=sys.stderr)


def decide_sites(source):
    """line -> ordinal of the DECIDE call sites of the contract's source, in file order"""
    with open(source) as f:
        lines = [n + 1 for n, text in enumerate(f) if re.search(r"\bDECIDE\(", text) and not re.match(r"\s*#\s*define", text)]
    return {line: k for k, line in enumerate(lines)}


def witness_digests(o, out, ws, source):
    pre = "perturb"
    for bits in BASE_VARIANTS:
        o.set_base_variant(bits)
        render_digests(o, out, f"{pre}/base{bits}", ws, post=True)
    o.set_base_variant(0)
    o.set_unfused(True)
    render_digests(o, out, f"{pre}/unfused", ws, post=True)
    o.set_unfused(False)
    for prim in range(7):
        for ulps in (1, -1):
            o.set_perturbation(prim, ulps)
            render_digests(o, out, f"{pre}/perturbation{prim}{ulps:+d}", ws)
    o.set_perturbation(-1, 0)
    o.set_signature_alpha(True)
    render_digests(o, out, f"{pre}/signature", ws, atmosphere=False)
    for seed in (1, 2, 12345):
        o.set_ensemble(seed, 16)
        render_digests(o, out, f"{pre}/ensemble{seed}", ws)
    o.set_ensemble(0, 0)
    o.set_signature_alpha(False)
    edge = ws[-1]
    o.set_nan_env([0.25, 0.5, 0.75])
    render_digests(o, out, f"{pre}/nan_env", [edge], atmosphere=False)
    o.set_nan_env(None)

    # ---- close decisions, replays and searches: pixels of frame 0 that llvmpipe's arithmetic (base 951) renders differently
    sites = decide_sites(source)
    for w in (ws[0], edge):
        scene, kw = scene_args(w)
        contract = o.render(*scene, threads=THREADS, **kw)
        o.set_base_variant(LLVMPIPE)
        ref = o.render(*scene, threads=THREADS, **kw)
        o.set_base_variant(0)
        apart = np.nan_to_num(np.abs(contract - ref).max(-1), nan=0.0, posinf=0.0).ravel()
        far = np.argsort(-apart, kind="stable")[:5]   # the five pixels the two arithmetics render furthest apart
        xy = np.concatenate([np.stack([far % w.width, far // w.width], axis=-1), [[3, 4], [w.width - 1, w.height - 1]]]).astype(np.int32)
        head, L = study_calls(o, w)
        last = np.zeros(4, np.float32)
        close, first_close = [], []
        for x, y in xy:
            buf = np.zeros((64, 4), np.float32)
            n = L.pto_list_close_decisions(*head, int(x), int(y), 0, last.ctypes.data_as(_fp), 1e-2, 64, buf.ctypes.data_as(_fp))
            first_close.append(int(buf[np.argmin(buf[:n, 2]), 0]) if n else 0)
            buf[:n, 1] = [sites.get(int(line), -1) for line in buf[:n, 1]]
            close.append(np.concatenate([[n], buf.ravel()]).astype(np.float32))
        out[f"{pre}/close_decisions/{w.name}"] = sha(np.array(close))
        replays = []
        for (x, y), nearest in zip(xy, first_close):
            plain, nd = o.render_pixel_variant(*scene, int(x), int(y), **kw)
            flip, nf = o.render_pixel_variant(*scene, int(x), int(y), flips=(nearest, -1, -1), **kw)
            site, nt = o.render_pixel_variant(*scene, int(x), int(y), sites=[(1, 0, 2), (2, 0, -2), (0, 1, 2), (7, 3, 1), (8, 0, 1)], **kw)
            nan, nn = o.render_pixel_variant(*scene, int(x), int(y), pow_neg_nan=2, **kw)
            replays.append(np.concatenate([plain, flip, site, nan, np.array([nd, nf, nt, nn], np.float32)]))
        out[f"{pre}/pixel_variant/{w.name}"] = sha(np.array(replays))
        # searches: towards llvmpipe's value (base 951), towards the replays above (one inverted comparison, shifted calls: the search
        # has to find such a neighbour again) and, for one pixel, towards a value no neighbour reaches (every stage runs to its end)
        rp = np.array(replays, np.float32)
        targets = [("951", xy, ref[xy[:, 1], xy[:, 0], :3]), ("flip", xy, rp[:, 4:7]), ("sites", xy, rp[:, 8:11]),
                   ("none", xy[:1], contract[xy[:1, 1], xy[:1, 0], :3] + np.float32(0.37))]
        for what, pix, want in targets:
            found = o.witness_search(*scene, pix, want, TIGHT_BAND, close_gap=1e-2, max_flips=32, **kw)
            flat = [np.concatenate([[r["kind"], *r["flips"], len(r["sites"]), r["evaluated"], r["unstable_calls"], r["largest_move"], r["distance"]],
                                    np.array(r["sites"], np.float64).ravel(), r["value"].astype(np.float64)]) for r in found]
            out[f"{pre}/witness_search/{w.name}/{what}"] = sha(np.concatenate(flat))
            print(f"  witness_search {w.name} towards {what}: kinds {[r['kind'] for r in found]}", file=sys.stderr)

    # ---- llvmpipe's built-ins as restated: all six functions on 4,096 seeded arguments
    rng = np.random.default_rng(951)
    head, L = study_calls(o, ws[0])
    x = np.concatenate([rng.uniform(-100, 100, 2048), rng.standard_normal(2040) * np.exp(rng.uniform(-30, 30, 2040)),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 128.5, -127.5]]).astype(np.float32)
    y = rng.uniform(-6, 6, x.size).astype(np.float32)
    res = np.zeros((6, x.size), np.float32)
    for which in range(6):
        assert L.pto_llvmpipe_like(which, x.ctypes.data_as(_fp), y.ctypes.data_as(_fp), x.size, res[which].ctypes.data_as(_fp)) == 0
    out[f"{pre}/llvmpipe_like"] = sha(res)


def compute(po) -> dict:
    """every digest of the fixture, from the libraries of the pt_oracle module `po`"""
    out = {}
    ws = workloads()
    for kind, flags in KINDS.items():
        o = po.Oracle(**flags)
        render_digests(o, out, kind, ws, post=True)
        out[f"{kind}/bounce_counts/{ws[-1].name}"] = sha(bounce_counts(o, ws[-1]))
        micro_digests(o, out, kind)
        stub_digests(o, kind, out, ws[-1])
        if kind == "margins":
            for w in ws:
                scene, kw = scene_args(w)
                img, margin, cont = o.render_with_margins(*scene, num_frames=w.frames, threads=THREADS, dump_each=True, **kw)
                out[f"margins/planes/{w.name}"] = sha(img, margin, cont)
                xy = np.array([[3, 4], [20, 11], [w.width - 1, w.height - 1], [w.width // 2, w.height // 2]], np.int32)
                out[f"margins/pixels/{w.name}"] = sha(*o.render_pixels_margins(*scene, xy, **kw))
        if kind == "perturb":
            witness_digests(o, out, ws, os.path.join(po.HERE, "pt_oracle.c"))
    return out


def load_oracle_module(directory):
    spec = importlib.util.spec_from_file_location("pt_oracle_recorded", os.path.join(directory, "pt_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--oracle-dir", default=os.path.join(ROOT, "oracle"), help="directory with pt_oracle.py, its C sources and Makefile")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    digests = compute(load_oracle_module(os.path.abspath(args.oracle_dir)))
    with open(args.out, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {args.out}")
