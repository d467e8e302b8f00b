"""GPU tests of the shading half of a bounce: bsdf() computes ONE hemisphere direction per lane (from the normal, or from its
negative with two further draws on refracting lanes) and the winner section of ray_trace_t fetches a material staged in LDS once,
at an index selected between the sphere and the cuboid form (csrc/pt_device.hpp).  Both only change how often a wavefront issues the
code, never a lane's arithmetic or the order of its draws, so the image stays bit-identical to the oracle (compute.glsl:184-224,
:226-258).  The scenes here are built to take exactly those paths: spheres and cuboids that are all or mostly refractive, every
combination of roughness 0 / 0.5 / 1, specular chance 0 / > 0 and ior 1 / > 1 (total internal reflection included), the camera
inside a glass sphere, depth 32, 1 and 4 samples per pixel, kernel variants 0 and 1 (one wavefront per tile), a >= 64-sphere
scene (sphere grid, materials read from device memory) and the full 256 + 64-object UBO.
Run with `pytest -m gpu` on an MI355X.  Nothing here reads /root/reference."""
import numpy as np
import pytest

from test_gpu_parity import assert_bit_exact

pytestmark = pytest.mark.gpu

W, H = 104, 60  # 13 x 7.5 tiles of 8 x 8: the last tile row is half empty
DEPTH = 32
FRAMES = 2


def glass(S, rng, *, rough, spec, ior, tint=True):
    """refractive with the given roughness on both lobes; specular_chance `spec` (0: the Fresnel block is skipped), the rest refracts
    except for a small diffuse share"""
    return S.Material(albedo=0.6 + 0.4 * rng.rand(3), absorbance=(rng.rand(3) * 0.4 if tint else S.vec3(0.0)), specular_chance=spec,
                      specular_roughness=rough, ior=ior, refraction_chance=(1.0 - spec) * 0.96, refraction_roughness=rough)


def room(S, rng, material_of, *, opaque_every=0):
    """the default room with every cuboid but the light turned into `material_of()`; `opaque_every` = n keeps every n-th one"""
    cubs = S.default_cuboids()
    for i, c in enumerate(cubs):
        if i == 1 or (opaque_every and i % opaque_every == 0):  # 1 = the ceiling light (emissive): the only thing that ends paths bright
            continue
        c.material = material_of()
    return cubs


def lobe_scene(pkg, seed, *, rough, spec, ior, n=40, opaque_every=7, box=((-16, -10, -20), (16, 10, -2)), radius=(0.8, 2.2)):
    """`n` spheres (overlapping here and there: origins inside several at once) and the room's cuboids, all or mostly glass"""
    S = pkg.scene
    rng = np.random.RandomState(seed)
    sc = S.Scene()
    lo, hi = np.array(box[0], np.float32), np.array(box[1], np.float32)
    for i in range(n):
        pos = (lo + (hi - lo) * rng.rand(3).astype(np.float32)).astype(np.float32)
        if opaque_every and i % opaque_every == opaque_every - 1:
            m = S.Material(albedo=rng.rand(3), emissiv=(rng.rand(3) * 3.0 if i % 2 else S.vec3(0.0)), specular_chance=0.5 * rng.rand(),
                           specular_roughness=rng.rand())
        else:
            m = glass(S, rng, rough=rough, spec=spec, ior=ior)
        sc.spheres.append(S.Sphere(pos, np.float32(rng.uniform(*radius)), i, m))
    sc.cuboids = room(S, rng, lambda: glass(S, rng, rough=rough, spec=spec, ior=ior, tint=False), opaque_every=3 if opaque_every else 0)
    return sc


def mixed_scene(pkg, seed, ns, nc):
    """`ns` spheres + `nc` cuboids; about 70 % glass with every roughness / specular chance / ior of the matrix above mixed, the rest
    opaque, some emissive"""
    S = pkg.scene
    rng = np.random.RandomState(seed)
    sc = S.Scene()

    def material():
        if rng.rand() < 0.7:
            return glass(S, rng, rough=[0.0, 0.5, 1.0][rng.randint(3)], spec=[0.0, 0.05, 0.3][rng.randint(3)],
                         ior=[1.0, 1.3, 1.5, 2.4][rng.randint(4)], tint=rng.rand() < 0.5)
        return S.Material(albedo=rng.rand(3), emissiv=(rng.rand(3) * 2.0 if rng.rand() < 0.25 else S.vec3(0.0)),
                          specular_chance=0.6 * rng.rand(), specular_roughness=rng.rand())

    lo, hi = np.array((-18, -11, -21), np.float32), np.array((18, 11, -1), np.float32)
    for i in range(ns):
        pos = (lo + (hi - lo) * rng.rand(3).astype(np.float32)).astype(np.float32)
        sc.spheres.append(S.Sphere(pos, np.float32(rng.uniform(0.3, 1.4)), i, material()))
    sc.cuboids = room(S, rng, material, opaque_every=3)
    while len(sc.cuboids) < nc:  # boxes between the spheres
        pos = (lo + (hi - lo) * rng.rand(3).astype(np.float32)).astype(np.float32)
        dim = (0.5 + 2.5 * rng.rand(3)).astype(np.float32)
        sc.cuboids.append(S.Cuboid(pos, dim, len(sc.cuboids), material()))
    sc.cuboids = sc.cuboids[:nc]
    return sc


def check(pkg, oracle, sc, cam, what, *, spps=(1, 4), variants=(0, 1), depth=DEPTH, frames=FRAMES):
    basic = pkg.camera.basic_data_ubo(cam, W, H)
    env = pkg.envmap.synthetic_sky_rgba32f(16)
    for spp in spps:
        want = oracle.render(W, H, basic, sc.ubo_bytes(), env, num_spheres=sc.num_spheres, num_cuboids=sc.num_cuboids, ray_depth=depth,
                             spp=spp, focal_length=12.0, aperture=0.05, num_frames=frames)
        assert float(np.nan_to_num(want[..., :3], posinf=0.0).max()) > 0.0, f"{what}: the scene renders nothing"
        for variant in variants:
            pt = pkg.PathTracer(env, W, H, depth, spp, 12.0, 0.05)
            pt.SetVariant(variant)
            pt.UploadScene(sc)
            pt.UploadBasicData(basic)
            for _ in range(frames):
                pt.Render()
            got = pt.Result
            pt.Dispose()
            assert_bit_exact(got, want, f"{what}, depth {depth}, {spp} spp, variant {variant}")


def default_camera(pkg):
    return pkg.camera.Camera()


@pytest.mark.parametrize("ior", [1.0, 1.5], ids=lambda v: f"ior{v}")
@pytest.mark.parametrize("spec", [0.0, 0.3], ids=lambda v: f"spec{v}")
@pytest.mark.parametrize("rough", [0.0, 0.5, 1.0], ids=lambda v: f"rough{v}")
def test_refractive_lobes_bit_exact(pkg, native_lib, oracle, rough, spec, ior):
    """Mostly glass: nearly every wavefront of every bounce holds refracting lanes beside diffuse and specular ones.  ior 1.5 with
    roughness 0 gives total internal reflection from inside (refract() = 0, a NaN direction downstream: compute.glsl:210-214)."""
    seed = 100 + int(rough * 2) * 4 + (2 if spec else 0) + (1 if ior > 1.0 else 0)
    sc = lobe_scene(pkg, seed, rough=rough, spec=spec, ior=ior)
    check(pkg, oracle, sc, default_camera(pkg), f"glass rough {rough} spec {spec} ior {ior}")


@pytest.mark.parametrize("rough", [0.0, 0.5, 1.0], ids=lambda v: f"rough{v}")
def test_all_refractive_bit_exact(pkg, native_lib, oracle, rough):
    """Every sphere and every cuboid but the light refracts (no opaque object, no specular share: the roll never takes the specular lobe)."""
    sc = lobe_scene(pkg, 200 + int(rough * 2), rough=rough, spec=0.0, ior=1.3, opaque_every=0)
    check(pkg, oracle, sc, default_camera(pkg), f"all glass, rough {rough}")


def test_camera_inside_a_glass_sphere(pkg, native_lib, oracle):
    """Every primary ray starts inside glass (fromInside at the first hit: Beer's law, the flipped normal, ior / 1 the other way round);
    ior 2.4 reflects most of them back inside."""
    S = pkg.scene
    for ior, rough in ((1.5, 0.0), (2.4, 0.5)):
        sc = lobe_scene(pkg, 300, rough=rough, spec=0.05, ior=ior)
        cam = default_camera(pkg)
        rng = np.random.RandomState(5)
        sc.spheres[0] = S.Sphere(np.asarray(cam.position, np.float32) + np.float32(0.4), np.float32(3.0), 0,
                                 glass(S, rng, rough=rough, spec=0.05, ior=ior))
        check(pkg, oracle, sc, cam, f"camera inside glass, ior {ior}, rough {rough}")


def test_large_scene_with_glass(pkg, native_lib, oracle):
    """96 spheres: the generic bounce walks the sphere grid and the materials are read from the UBO in device memory (sphere form
    5 * i + 1, cuboid form 1280 + 6 * i + 2)."""
    sc = mixed_scene(pkg, 400, 96, 12)
    check(pkg, oracle, sc, default_camera(pkg), "96 spheres + 12 cuboids, 70 % glass")


def test_full_ubo_with_glass(pkg, native_lib, oracle):
    """256 spheres + 64 cuboids: the last material of either array is reachable."""
    sc = mixed_scene(pkg, 500, 256, 64)
    check(pkg, oracle, sc, default_camera(pkg), "256 spheres + 64 cuboids, 70 % glass")
