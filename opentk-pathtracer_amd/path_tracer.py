"""Host-side mirror of the reference's renderer classes over the C ABI (harness glue for tests and bench).

  PathTracer            /root/reference/OpenTK-PathTracer/src/Render/PathTracer.cs:9-141
  AtmosphericScatterer  /root/reference/OpenTK-PathTracer/src/Render/AtmosphericScatterer.cs:9-119
  BufferObject.SubData  /root/reference/OpenTK-PathTracer/src/Render/Objects/BufferObject.cs:37-48

Member names and argument meaning follow the C# classes (NumSpheres, RayDepth, SPP, Render(), SetSize(),
ResetRenderer(), Samples, Result ...), so the call sequence of the reference's MainWindow can be replayed as is.
Every method is a thin call into libmi355pt.so; there is no Python or CPU implementation of the integrator here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native
from .native import check


# one record of pt_first_hit_read / pt_pick (include/mi355pt.h): 32 bytes
FIRST_HIT_DTYPE = np.dtype([("origin", np.float32, 3), ("t", np.float32), ("dir", np.float32, 3), ("id", np.int32)])
assert FIRST_HIT_DTYPE.itemsize == 32
# one guide record of pt_denoise_read_guides (include/mi355pt.h): 32 bytes; id and t as in FIRST_HIT_DTYPE
GUIDE_DTYPE = np.dtype([("pos", np.float32, 3), ("id", np.int32), ("normal", np.float32, 3), ("t", np.float32)])
assert GUIDE_DTYPE.itemsize == 32
# an entry of the object map (pt_denoise_read_object_map): history point = a * P + b per component, state = PT_TRACK_KEEP / MOVED / DROP
OBJECT_MAP_DTYPE = np.dtype([("a", np.float32, 3), ("state", np.int32), ("b", np.float32, 3), ("zero", np.int32)])
assert OBJECT_MAP_DTYPE.itemsize == 32
# a tile record of pt_adaptive_read_tiles: samples held, the count the statistics started at, the tile's noise estimate, in-image pixels
ADAPTIVE_TILE_DTYPE = np.dtype([("k", np.int32), ("k0", np.int32), ("err", np.float32), ("n", np.int32)])
assert ADAPTIVE_TILE_DTYPE.itemsize == 16


class EnvironmentMap:
    """A cube texture as the host would hand it to GL: 6 faces (+X,-X,+Y,-Y,+Z,-Z), RGBA32F or SRGB8_A8
    (MainWindow.cs:177-187)."""

    def __init__(self, faces: np.ndarray):
        faces = np.ascontiguousarray(faces)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 4:
            raise ValueError("faces must have shape (6, S, S, 4)")
        if faces.dtype == np.float32:
            self.format = native.PT_ENV_RGBA32F
        elif faces.dtype == np.uint8:
            self.format = native.PT_ENV_SRGB8_A8
        else:
            raise ValueError("faces must be float32 (RGBA32F) or uint8 (SRGB8_A8)")
        self.faces = faces
        self.size = faces.shape[1]


class UniformBuffer:
    """BufferObject bound as UBO 0 (BasicDataUBO) or UBO 1 (GameObjectsUBO): SubData(offset, size, data)."""

    def __init__(self, tracer: "PathTracer", which: str):
        self._t, self._which = tracer, which

    def SubData(self, offset: int, size: int, data) -> None:
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray))
                                   else np.asarray(data))
        if buf.nbytes < size:
            raise ValueError("data shorter than size")
        fn = self._t._lib.pt_upload_basic_data if self._which == "basic" else self._t._lib.pt_upload_game_objects
        check(fn(self._t._h, offset, size, buf.ctypes.data_as(C.c_void_p)), self._t._h)


class PathTracer:
    def __init__(self, environmentMap, width: int, height: int, rayDepth: int, spp: int, focalLength: float,
                 apertureDiamater: float, device: int = 0, devices=None):
        """`devices` = list of HIP device ids: ONE renderer row-tiled over those GPUs inside the library
        (pt_create_multi; the gather over xGMI happens inside Result / Present).  Otherwise one GPU (`device`)."""
        self._lib = native.load()
        h = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*devices)
            check(self._lib.pt_create_multi(ids, len(devices), width, height, C.byref(h)))
        else:
            check(self._lib.pt_create(device, width, height, C.byref(h)))
        self._h = h
        self.devices = list(devices) if devices is not None else [device]
        self.band_rows, self.band_world, self.band_rank = 0, 1, 0
        self.Width, self.Height = width, height
        self._numSpheres = self._numCuboids = 0
        self._rayDepth, self._spp = rayDepth, spp
        self._focalLength, self._apertureDiameter = focalLength, apertureDiamater
        self._push_params()
        self._adaptive = (1e-4, 8, 1024)  # the last SetAdaptive values (the library's defaults; the ABI has no getter)
        self._env = None
        self.BasicDataUBO = UniformBuffer(self, "basic")       # MainWindow.cs:195-197
        self.GameObjectsUBO = UniformBuffer(self, "objects")   # MainWindow.cs:199-201
        self.y0, self.rows = 0, height
        if environmentMap is not None:
            self.EnvironmentMap = environmentMap

    # -- the six uniform-setting properties, PathTracer.cs:11-83
    def _push_params(self):
        check(self._lib.pt_set_params(self._h, self._numSpheres, self._numCuboids, self._rayDepth, self._spp,
                                      self._focalLength, self._apertureDiameter), self._h)

    def _prop(name):  # noqa: N805
        def get(self):
            return getattr(self, name)

        def set_(self, v):
            setattr(self, name, v)
            self._push_params()
        return property(get, set_)

    NumSpheres = _prop("_numSpheres")
    NumCuboids = _prop("_numCuboids")
    RayDepth = _prop("_rayDepth")
    SPP = _prop("_spp")
    FocalLength = _prop("_focalLength")
    ApertureDiameter = _prop("_apertureDiameter")
    del _prop

    @property
    def EnvironmentMap(self):  # PathTracer.cs:85
        return self._env

    @EnvironmentMap.setter
    def EnvironmentMap(self, env):
        if isinstance(env, AtmosphericScatterer):
            env._select(self)
        else:
            if not isinstance(env, EnvironmentMap):
                env = EnvironmentMap(env)
            ptrs = (C.c_void_p * 6)(*[env.faces[f].ctypes.data_as(C.c_void_p) for f in range(6)])
            check(self._lib.pt_set_environment(self._h, env.size, env.format, ptrs), self._h)
        self._env = env

    @property
    def Samples(self) -> int:  # PathTracer.cs:112
        return self.FrameIndex * self._spp

    @property
    def FrameIndex(self) -> int:
        v = C.c_int()
        check(self._lib.pt_get_frame_index(self._h, C.byref(v)), self._h)
        return v.value

    def Render(self) -> int:  # PathTracer.cs:114-129
        total = C.c_int()
        check(self._lib.pt_render(self._h, C.byref(total)), self._h)
        return total.value

    def SetSize(self, width: int, height: int) -> None:  # PathTracer.cs:131-135
        check(self._lib.pt_set_size(self._h, width, height), self._h)
        self.Width, self.Height = width, height
        self.y0, self.rows = 0, height
        self.band_rows, self.band_world, self.band_rank = 0, 1, 0

    def ResetRenderer(self) -> None:  # PathTracer.cs:137-140
        check(self._lib.pt_reset(self._h), self._h)

    # -- multi-GPU tiling + plumbing (no reference counterpart)
    def SetTile(self, y0: int, rows: int) -> None:
        check(self._lib.pt_set_tile(self._h, y0, rows), self._h)
        self.y0, self.rows = y0, rows
        self.band_rows, self.band_world, self.band_rank = 0, 1, 0

    def SetInterleavedTile(self, rank: int, world: int, band_rows: int) -> None:
        check(self._lib.pt_set_interleaved_tile(self._h, rank, world, band_rows), self._h)
        from .distributed import interleaved_rows
        self.y0, self.rows = 0, len(interleaved_rows(self.Height, rank, world, band_rows))
        self.band_rows, self.band_world, self.band_rank = band_rows, world, rank

    # -- persistence (the reference only has the screenshot button, Gui.cs:28-33)
    def SaveCheckpoint(self, path) -> None:
        from . import checkpoint
        checkpoint.save_checkpoint(path, self)

    def LoadCheckpoint(self, path, strict: bool = True) -> dict:
        from . import checkpoint
        return checkpoint.load_checkpoint(path, self, strict)

    def SaveScreenshot(self, path) -> None:  # Gui.cs:28-33 -> Framebuffer.cs:67-82
        from . import checkpoint
        checkpoint.save_screenshot(path, self)

    @property
    def Result(self) -> np.ndarray:
        """The RGBA32F `Result` image of this tile, read back to the host: (rows, Width, 4), row 0 = image row y0."""
        out = np.empty((self.rows, self.Width, 4), dtype=np.float32)
        check(self._lib.pt_read_result(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def ReadInto(self, out: np.ndarray) -> np.ndarray:
        assert out.dtype == np.float32 and out.shape == (self.rows, self.Width, 4) and out.flags.c_contiguous
        check(self._lib.pt_read_result(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def PresentInto(self, out: np.ndarray) -> np.ndarray:
        assert out.dtype == np.uint8 and out.shape == (self.rows, self.Width, 4) and out.flags.c_contiguous
        check(self._lib.pt_present_rgba8(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), 0), self._h)
        return out

    def Present(self) -> np.ndarray:
        """ScreenEffect.Render(PathTracer.Result) (ScreenEffect.cs:29-37, PostProcessing/fragment.glsl): the tone-mapped
        RGBA8 image of this tile, (rows, Width, 4) uint8, row 0 = image row y0."""
        out = np.empty((self.rows, self.Width, 4), dtype=np.uint8)
        check(self._lib.pt_present_rgba8(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), 0), self._h)
        return out

    def PresentAsync(self, slot: int) -> None:
        """Non-blocking present (pt_present_rgba8_async): tone map + device-to-host copy of the image as it is now into
        the library's pinned slot; Render() calls that follow overlap the copy."""
        check(self._lib.pt_present_rgba8_async(self._h, slot), self._h)

    def PresentWait(self, slot: int):
        """-> (image, frame_index): (rows, Width, 4) uint8 VIEW of the slot's pinned host image (valid until the next
        PresentAsync on that slot) and the number of frames it shows."""
        st = self.__dict__.setdefault("_present_state", {})
        if "args" not in st:
            st["args"] = (C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_int())
            st["views"] = {}
        ptr, pitch, frame = st["args"]
        rc = self._lib.pt_present_wait(self._h, slot, C.byref(ptr), C.byref(pitch), C.byref(frame))
        if rc:
            check(rc, self._h)
        if not ptr:  # a slot bound to caller-owned device memory (BindPresentImage): the image is there, nothing came to the host
            return None, frame.value
        key = (slot, C.addressof(ptr.contents), self.rows, self.Width)
        img = st["views"].get(key)
        if img is None:  # one numpy view per pinned slot image (building it costs more than the call itself)
            assert pitch.value == self.Width * 4
            img = st["views"][key] = np.ctypeslib.as_array(ptr, shape=(self.rows, self.Width, 4))
        return img, frame.value

    def BindPresentImage(self, slot: int, device_ptr, nbytes: int = 0) -> None:
        """pt_present_bind_device_image: present slot `slot` tone-maps into caller-owned device memory (interop-style); None restores."""
        check(self._lib.pt_present_bind_device_image(self._h, slot, C.c_void_p(device_ptr) if device_ptr else None, nbytes), self._h)

    def SetPartition(self, band_rows: int) -> None:
        """Group handles: block-cyclic bands of `band_rows` image rows per device (0 = contiguous row blocks)."""
        check(self._lib.pt_multi_set_partition(self._h, band_rows), self._h)

    @property
    def GatherIsDirect(self) -> bool:
        """Group handles: True when every gather copy goes over a direct peer link (pt_multi_gather_is_direct); a staged group must not
        be the source of a scaling number."""
        v = C.c_int()
        check(self._lib.pt_multi_gather_is_direct(self._h, C.byref(v)), self._h)
        return bool(v.value)

    def PostProcessDevice(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self._lib.pt_postprocess_device(self._h, C.byref(p), C.byref(n)), self._h)
        return p.value, n.value

    def WriteResult(self, image: np.ndarray, frame_index: int) -> None:
        img = np.ascontiguousarray(image, dtype=np.float32)
        assert img.shape == (self.rows, self.Width, 4)
        check(self._lib.pt_write_result(self._h, img.ctypes.data_as(C.POINTER(C.c_float)), 0, frame_index), self._h)

    def Synchronize(self) -> None:
        check(self._lib.pt_synchronize(self._h), self._h)

    def ResultDevicePtr(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self._lib.pt_result_device_ptr(self._h, C.byref(p), C.byref(n)), self._h)
        return p.value, n.value

    def BindResultBuffer(self, device_ptr: int | None, nbytes: int = 0) -> None:
        check(self._lib.pt_bind_result_buffer(self._h, C.c_void_p(device_ptr), nbytes), self._h)

    def SetStream(self, hip_stream: int | None) -> None:
        check(self._lib.pt_set_stream(self._h, C.c_void_p(hip_stream)), self._h)

    def SetVariant(self, variant: int) -> None:
        check(self._lib.pt_set_variant(self._h, variant), self._h)

    def SetArithmetic(self, mode: int) -> None:
        """native.PT_ARITH_CONTRACT (default, fastest) or native.PT_ARITH_REFERENCE (the GL reference's own arithmetic: bit-identical to
        it in ~98.6 % of pixels, slower).  Frames rendered before keep their arithmetic; the accumulation is not reset."""
        check(self._lib.pt_set_arithmetic(self._h, mode), self._h)

    def SetPresentArithmetic(self, mode: int) -> None:
        """Arithmetic of the tone map of the presents that follow (Present, PostProcessDevice, PresentAsync; pt_present_set_arithmetic):
        native.PT_ARITH_CONTRACT (default) or native.PT_ARITH_REFERENCE (the GL reference's own arithmetic: its float colour bit for bit on
        the reference's fixture).  Independent of SetArithmetic and AtmosphericScatterer.SetArithmetic; the image is not touched."""
        if mode not in (native.PT_ARITH_CONTRACT, native.PT_ARITH_REFERENCE):
            raise ValueError("mode must be native.PT_ARITH_CONTRACT or native.PT_ARITH_REFERENCE")
        check(self._lib.pt_present_set_arithmetic(self._h, mode), self._h)

    # -- first-hit query (replaces the CPU ray caster of Gui.cs:223-233 -> MainWindow.RayTrace, MainWindow.cs:302-318)
    def FirstHit(self, frame: int = 0) -> np.ndarray:
        """pt_first_hit_render + pt_first_hit_read: per pixel the primary ray of sample 0 of `frame` and what it meets first, as a
        (rows, Width) structured array (FIRST_HIT_DTYPE): origin (3,), t (+inf on a miss), dir (3,), id (-1 miss, sphere i = i,
        cuboid j = native.PT_MAX_SPHERES + j).  Row 0 = image row y0.  Touches neither the image nor the frame counter."""
        check(self._lib.pt_first_hit_render(self._h, frame), self._h)
        out = np.empty((self.rows, self.Width), dtype=FIRST_HIT_DTYPE)
        check(self._lib.pt_first_hit_read(self._h, out.ctypes.data_as(C.c_void_p), 0), self._h)
        return out

    def SetFirstHitRay(self, mode: int) -> None:
        """pt_first_hit_set_ray: the ray of the FirstHit and Pick calls that follow — native.PT_RAY_SAMPLE0 (sample 0 of `frame`, lens and
        sub-pixel draws included; the default) or native.PT_RAY_PINHOLE (the pinhole ray through the pixel's centre: the same answer for
        every frame, focal length and aperture)."""
        check(self._lib.pt_first_hit_set_ray(self._h, mode), self._h)

    def Pick(self, x: int, y: int, frame: int = 0):
        """pt_pick: -> (id, t, origin (3,), dir (3,)) of image pixel (x, y) (y = 0 is the bottom row) for sample 0 of `frame`."""
        i, t = C.c_int(), C.c_float()
        o, d = np.empty(3, np.float32), np.empty(3, np.float32)
        fp = C.POINTER(C.c_float)
        check(self._lib.pt_pick(self._h, x, y, frame, C.byref(i), C.byref(t), o.ctypes.data_as(fp), d.ctypes.data_as(fp)), self._h)
        return i.value, t.value, o, d

    # -- preview denoiser (the image of MainWindow.cs:49-56 filtered for display)
    def SetDenoise(self, iterations: int = 5, sigma_color: float = 0.5, sigma_plane: float = 0.02, normal_log2_power: int = 5) -> None:
        """pt_denoise_set_params: a-trous passes (0..6), luminance and plane-distance edge-stops (> 0), log2 of the normal weight's power (0..7)."""
        check(self._lib.pt_denoise_set_params(self._h, iterations, sigma_color, sigma_plane, normal_log2_power), self._h)

    def Denoise(self, frame: int = 0) -> np.ndarray:
        """pt_denoise_render + pt_denoise_read: the image as it stands, filtered with guides from sample 0 of `frame`, as (rows, Width, 4)
        float32 (alpha = 1).  Touches neither the image nor the frame counter.  Single-GPU handles that own the whole image."""
        check(self._lib.pt_denoise_render(self._h, frame), self._h)
        out = np.empty((self.rows, self.Width, 4), dtype=np.float32)
        check(self._lib.pt_denoise_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def DenoiseGuides(self) -> np.ndarray:
        """pt_denoise_read_guides: the guide records of the last Denoise as a (rows, Width) structured array (GUIDE_DTYPE): pos (3,), id,
        normal (3,), t; a miss has id -1, t +inf, pos = normal = 0."""
        out = np.empty((self.rows, self.Width), dtype=GUIDE_DTYPE)
        check(self._lib.pt_denoise_read_guides(self._h, out.ctypes.data_as(C.c_void_p), 0), self._h)
        return out

    def SetDenoiseMode(self, mode: int, sigma_variance: float = 6.0) -> None:
        """pt_denoise_set_mode: PT_DENOISE_FIXED (sigma_color, halved every pass) or PT_DENOISE_VARIANCE (the luminance stop is
        sigma_variance standard deviations of each pixel's own noise, estimated from the image) for the Denoise calls that follow."""
        check(self._lib.pt_denoise_set_mode(self._h, mode, sigma_variance), self._h)

    def DenoiseVariance(self) -> np.ndarray:
        """pt_denoise_read_variance: the variance estimate V0 of the last Denoise in PT_DENOISE_VARIANCE as (rows, Width) float32."""
        out = np.empty((self.rows, self.Width), dtype=np.float32)
        check(self._lib.pt_denoise_read_variance(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def SetDenoiseTemporal(self, enable: bool = True, max_history: int = 32) -> None:
        """pt_denoise_set_temporal: the Denoise calls that follow carry the previous view's result across a ResetRenderer by reprojecting
        it through the guides and blending by sample counts; max_history (1..65535) caps the count a history pixel brings along."""
        check(self._lib.pt_denoise_set_temporal(self._h, int(enable), max_history), self._h)

    def ClearDenoiseHistory(self) -> None:
        """pt_denoise_history_clear: forget what the temporal stage integrated (after a scene, material or environment edit)."""
        check(self._lib.pt_denoise_history_clear(self._h), self._h)

    def DenoiseIntegrated(self) -> np.ndarray:
        """pt_denoise_read_integrated: the integrated image of the last Denoise with the temporal stage on as (rows, Width, 4) float32;
        alpha = the per-pixel sample count."""
        out = np.empty((self.rows, self.Width, 4), dtype=np.float32)
        check(self._lib.pt_denoise_read_integrated(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def DenoiseHistory(self):
        """pt_denoise_read_history: the history set the last temporal Denoise used -> (image (rows, Width, 4) float32, guides (rows, Width)
        GUIDE_DTYPE, B (3, 3) float32, O (3,) float32): B (P - O) = lambda (ndc x, ndc y, 1) for a point P that view saw."""
        image = np.empty((self.rows, self.Width, 4), dtype=np.float32)
        guides = np.empty((self.rows, self.Width), dtype=GUIDE_DTYPE)
        B, O = np.empty((3, 3), dtype=np.float32), np.empty(3, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        check(self._lib.pt_denoise_read_history(self._h, image.ctypes.data_as(fp), guides.ctypes.data_as(C.c_void_p), B.ctypes.data_as(fp),
                                                O.ctypes.data_as(fp)), self._h)
        return image, guides, B, O

    def SetDenoiseTracking(self, enable: bool = True, edit_max_history: int = 0) -> None:
        """pt_denoise_set_object_tracking: the temporal Denoise calls that follow compare the scene with the one their history was made of —
        the history of an object that moved or was resized is found through that object's own motion, that of an object whose material
        changed is dropped for that object only; edit_max_history (0..65535, 0 = max_history) caps the history count after such an edit."""
        check(self._lib.pt_denoise_set_object_tracking(self._h, int(enable), edit_max_history), self._h)

    def DenoiseObjectMap(self):
        """pt_denoise_read_object_map: -> (the object map of the last Denoise as 320 entries of OBJECT_MAP_DTYPE, indexed by guide id;
        tracked: True if the scene differed from the history's and the tracked kernel ran)."""
        out = np.empty(native.PT_MAX_SPHERES + native.PT_MAX_CUBOIDS, dtype=OBJECT_MAP_DTYPE)
        tracked = C.c_int()
        check(self._lib.pt_denoise_read_object_map(self._h, out.ctypes.data_as(C.c_void_p), C.byref(tracked)), self._h)
        return out, bool(tracked.value)

    def SetDenoiseLens(self, enable: bool = True, coc_scale: float = 1.0) -> None:
        """pt_denoise_set_lens: the Denoise calls that follow take their guides from the pinhole ray through the pixel's centre instead
        of sample 0, and relax the id, normal and plane stops of a tap that lies within coc_scale times the lens's blur radius of both
        its ends (coc_scale 0: pinhole guides, the usual tap rules).  For a host that renders with the lens open."""
        check(self._lib.pt_denoise_set_lens(self._h, int(enable), coc_scale), self._h)

    def SetDenoiseMoments(self, enable: bool = True, prior_samples: int = 32) -> None:
        """pt_denoise_set_moments: the Denoise calls that follow observe the image and keep per-pixel moments across frames; from the
        second observation on, PT_DENOISE_VARIANCE blends the variance measured that way with the spatial estimate, which counts as
        prior_samples (1..65535) observations."""
        check(self._lib.pt_denoise_set_moments(self._h, int(enable), prior_samples), self._h)

    def DenoiseNoise(self) -> np.ndarray:
        """pt_denoise_read_noise: the noise map Vm of the last Denoise with the moments on (variance of the tone-compressed luminance of
        the image as it stands, measured across frames) as (rows, Width) float32; needs two observations."""
        out = np.empty((self.rows, self.Width), dtype=np.float32)
        check(self._lib.pt_denoise_read_noise(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def DenoiseNoiseLevel(self):
        """pt_denoise_noise_level: -> (the mean of Vm over the pixels with id >= 0, the observation count K, that pixel count): the
        convergence figure a host compares with a threshold."""
        mean, k, hit = C.c_float(), C.c_int(), C.c_int()
        check(self._lib.pt_denoise_noise_level(self._h, C.byref(mean), C.byref(k), C.byref(hit)), self._h)
        return float(mean.value), int(k.value), int(hit.value)

    # -- adaptive sampling (per-tile sample counts driven by measured noise)
    def SetAdaptive(self, threshold: float = 1e-4, min_samples: int = 8, max_samples: int = 1024) -> None:
        """pt_adaptive_set_params: a tile stays active while it holds fewer than max_samples samples and either fewer than min_samples
        since its statistics started or a noise estimate (variance of the tone-compressed luminance) above threshold."""
        check(self._lib.pt_adaptive_set_params(self._h, threshold, min_samples, max_samples), self._h)
        self._adaptive = (float(np.float32(threshold)), int(min_samples), int(max_samples))

    @property
    def AdaptiveParams(self) -> tuple:
        """(threshold, min_samples, max_samples) as the last successful SetAdaptive left them (the defaults before the first)."""
        return self._adaptive

    def RenderAdaptive(self, passes: int = 1) -> None:
        """pt_adaptive_render: `passes` passes, each one more sample per pixel of every tile still active.  Asynchronous.  The first call
        starts an adaptive state from the frames rendered so far; until ResetRenderer, Render raises and FrameIndex stays."""
        check(self._lib.pt_adaptive_render(self._h, passes), self._h)

    def AdaptiveStatus(self) -> dict:
        """pt_adaptive_status: -> active_tiles, tiles, pixel_samples (sum over pixels of sample count x spp), min_count, max_count."""
        a, t, lo, hi, s = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        check(self._lib.pt_adaptive_status(self._h, C.byref(a), C.byref(t), C.byref(s), C.byref(lo), C.byref(hi)), self._h)
        return {"active_tiles": a.value, "tiles": t.value, "pixel_samples": s.value, "min_count": lo.value, "max_count": hi.value}

    def AdaptiveTiles(self) -> np.ndarray:
        """pt_adaptive_read_tiles: the tile records as a (ceil(rows / 8), ceil(Width / 8)) structured array (ADAPTIVE_TILE_DTYPE)."""
        out = np.empty(((self.rows + 7) // 8, (self.Width + 7) // 8), dtype=ADAPTIVE_TILE_DTYPE)
        check(self._lib.pt_adaptive_read_tiles(self._h, out.ctypes.data_as(C.c_void_p)), self._h)
        return out

    def AdaptiveNoise(self) -> np.ndarray:
        """pt_adaptive_read_noise: the per-pixel noise estimate e as (rows, Width) float32."""
        out = np.empty((self.rows, self.Width), dtype=np.float32)
        check(self._lib.pt_adaptive_read_noise(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def AdaptiveM2(self) -> np.ndarray:
        """pt_adaptive_read_m2: the per-pixel Welford sum M2 as (rows, Width) float32."""
        out = np.empty((self.rows, self.Width), dtype=np.float32)
        check(self._lib.pt_adaptive_read_m2(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    @property
    def AdaptiveLive(self) -> bool:
        """Whether an adaptive state is live (pt_adaptive_status with every pointer NULL returns PT_OK).  Never raises."""
        return self._lib.pt_adaptive_status(self._h, None, None, None, None, None) == native.PT_OK

    def AdaptiveState(self) -> dict:
        """The whole of a live state: frame_index (the F it started from), image, tiles (ADAPTIVE_TILE_DTYPE), m2.  The per-pixel
        estimate and the tiles' err are functions of these; RestoreAdaptive rebuilds them."""
        return {"frame_index": self.FrameIndex, "image": self.Result, "tiles": self.AdaptiveTiles(), "m2": self.AdaptiveM2()}

    def RestoreAdaptive(self, image: np.ndarray, frame_index: int, tiles: np.ndarray, m2: np.ndarray) -> None:
        """pt_adaptive_write_state: installs a live state as AdaptiveState returned it; every read-out and every later pass then equals
        those of the tracer the state was read from.  A refused call changes nothing."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        rec = np.ascontiguousarray(tiles, dtype=ADAPTIVE_TILE_DTYPE)
        sums = np.ascontiguousarray(m2, dtype=np.float32)
        assert img.shape == (self.rows, self.Width, 4) and sums.shape == (self.rows, self.Width)
        assert rec.shape == ((self.rows + 7) // 8, (self.Width + 7) // 8)
        fp = C.POINTER(C.c_float)
        check(self._lib.pt_adaptive_write_state(self._h, img.ctypes.data_as(fp), 0, frame_index, rec.ctypes.data_as(C.c_void_p),
                                                sums.ctypes.data_as(fp), 0), self._h)

    def EndAdaptive(self) -> int:
        """pt_adaptive_end: levels every tile to the largest count and leaves the adaptive state; the image then equals that many Render
        calls bit for bit and Render is accepted again.  -> the new frame index."""
        v = C.c_int()
        check(self._lib.pt_adaptive_end(self._h, C.byref(v)), self._h)
        return v.value

    def SetDenoiseAdaptiveNoise(self, enable: bool = True, prior_samples: int = 8) -> None:
        """pt_denoise_set_adaptive_noise: on a live adaptive state the Denoise calls that follow form pass 0's variance in
        PT_DENOISE_VARIANCE from the sampler's own per-pixel estimate e and the tile counts, blended with the spatial estimate, which
        counts as prior_samples (1..65535) samples.  Without a live state nothing changes."""
        check(self._lib.pt_denoise_set_adaptive_noise(self._h, int(enable), prior_samples), self._h)

    def DenoiseVarianceUsed(self) -> np.ndarray:
        """pt_denoise_read_variance_used: var_0, the variance pass 0 of the last Denoise read in place of V0 (formed from the adaptive
        state or from the moments), as (rows, Width) float32; raises when that Denoise blended nothing."""
        out = np.empty((self.rows, self.Width), dtype=np.float32)
        check(self._lib.pt_denoise_read_variance_used(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), 0), self._h)
        return out

    def PresentDenoised(self) -> np.ndarray:
        """pt_denoise_present_rgba8: the result of the last Denoise through the tone map Present applies, as (rows, Width, 4) uint8."""
        out = np.empty((self.rows, self.Width, 4), dtype=np.uint8)
        check(self._lib.pt_denoise_present_rgba8(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), 0), self._h)
        return out

    def SetFrameBatch(self, max_frames: int) -> None:
        """Largest number of consecutive Render() calls one launch pipelines (1 = launch every frame at once)."""
        check(self._lib.pt_set_frame_batch(self._h, max_frames), self._h)

    def TimerBegin(self) -> None:
        check(self._lib.pt_timer_begin(self._h), self._h)

    def TimerEnd(self) -> float:
        ms = C.c_float()
        check(self._lib.pt_timer_end(self._h, C.byref(ms)), self._h)
        return ms.value

    def ReadEnvironment(self) -> np.ndarray:
        s = C.c_int()
        check(self._lib.pt_read_environment(self._h, None, C.byref(s)), self._h)
        out = np.empty((6, s.value, s.value, 4), dtype=np.float32)
        check(self._lib.pt_read_environment(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(s)), self._h)
        return out

    # -- convenience: replay the host's upload sequence for a whole scene + camera
    def UploadScene(self, scene) -> None:
        """LoadScene()'s upload loop (MainWindow.cs:265-266): one SubData per object, then the counts."""
        for obj in scene.objects():
            d = obj.gpu_data()
            self.GameObjectsUBO.SubData(obj.buffer_offset, d.nbytes, d)
        self._numSpheres, self._numCuboids = scene.num_spheres, scene.num_cuboids
        self._push_params()

    def UploadBasicData(self, blob: bytes) -> None:
        """The three SubData calls of MainWindow.cs:131-132,279 (InvProjection, InvView, ViewPos)."""
        self.BasicDataUBO.SubData(0, 64, blob[0:64])
        self.BasicDataUBO.SubData(64, 64, blob[64:128])
        self.BasicDataUBO.SubData(128, 16, blob[128:144])

    def Dispose(self) -> None:
        if getattr(self, "_h", None):
            self._lib.pt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


class AtmosphericScatterer:
    """AtmosphericScatterer.cs:9-119 — precomputes the sky cube on the GPU of the PathTracer it is attached to."""

    def __init__(self, size: int, atmo_ubo: bytes, light_pos, tracer: PathTracer | None = None):
        self.Size = size
        self.ISteps, self.JSteps = 50, 15          # AtmosphericScatterer.cs:92-93
        self.LightIntensity = 15.0                 # :94
        self.LightPos = np.asarray(light_pos, dtype=np.float32)  # from Time, :41
        self._ubo = bytes(atmo_ubo)
        self._tracer = tracer
        self._arithmetic = native.PT_ARITH_CONTRACT

    def SetSize(self, size: int) -> None:  # :115-118
        self.Size = size

    def SetArithmetic(self, mode: int) -> None:
        """native.PT_ARITH_CONTRACT (default) or native.PT_ARITH_REFERENCE (the GL reference's own arithmetic: every texel within 1e-4
        of its cube, at about the same speed) for the Render() calls that follow.  Remembered on this object and applied before each Render(), so it
        survives re-attachment to another tracer; independent of PathTracer.SetArithmetic."""
        if mode not in (native.PT_ARITH_CONTRACT, native.PT_ARITH_REFERENCE):
            raise ValueError("mode must be PT_ARITH_CONTRACT or PT_ARITH_REFERENCE")
        self._arithmetic = mode

    def _select(self, tracer: PathTracer) -> None:
        self._tracer = tracer
        self.Render()

    def Render(self) -> None:  # :102-113
        t = self._tracer
        if t is None:
            raise RuntimeError("AtmosphericScatterer is not attached to a PathTracer")
        buf = np.frombuffer(self._ubo, dtype=np.uint8)
        check(t._lib.pt_atmosphere_upload_data(t._h, 0, buf.nbytes, buf.ctypes.data_as(C.c_void_p)), t._h)
        lp = np.ascontiguousarray(self.LightPos, dtype=np.float32)
        check(t._lib.pt_atmosphere_set_arithmetic(t._h, self._arithmetic), t._h)
        check(t._lib.pt_atmosphere_render(t._h, self.Size, self.ISteps, self.JSteps,
                                          lp.ctypes.data_as(C.POINTER(C.c_float)), max(self.LightIntensity, 0.0)), t._h)

    @property
    def Result(self) -> np.ndarray:
        return self._tracer.ReadEnvironment()
