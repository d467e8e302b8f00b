/*
 * mi355pt.h — C ABI of libmi355pt.so: the MI355X (gfx950) replacement for the reference's path-tracing
 * compute dispatch.  Plain C, cdecl, blittable arguments only, so the reference's C# host can bind every
 * entry point with [DllImport("mi355pt")] (binding shown in INTEGRATION.md).
 *
 * The reference has NO plugin/FFI interface for this path: the hot path is hard-wired GL calls inside the
 * C# class PathTracer.  Each entry point below therefore replaces one thing the host does to the shader
 * today; citations are relative to /root/reference/OpenTK-PathTracer/.
 *
 * Conventions
 *   - every function returns PT_OK (0) or a negative PT_E_* code; nothing throws across the boundary
 *     (reference: C# exceptions + console prints, src/Render/Objects/ShaderProgram.cs:25-27,70-74);
 *     pt_last_error() returns a human-readable message for the last failure on that handle
 *     (or for the last failed pt_create when handle == NULL);
 *   - the host owns every source/destination array for the duration of the call only (as with
 *     GL.NamedBufferSubData, src/Render/Objects/BufferObject.cs:37-48); the library owns all device memory;
 *   - one handle = one renderer on one GPU (pt_create) or on a GROUP of GPUs (pt_create_multi: the image is
 *     row-tiled across the devices inside the library and gathered over xGMI only when it is read or presented),
 *     callable from one thread at a time (the reference calls everything from the GameWindow thread,
 *     src/MainWindow.cs:40,72,146).  Work is enqueued on the handle's HIP stream: pt_upload_*, pt_set_* and
 *     pt_render are stream-ordered; only pt_read_*, pt_present_rgba8, pt_present_wait, pt_synchronize,
 *     pt_timer_end and pt_destroy block;
 *   - limits (PT_E_OUT_OF_RANGE beyond them): width, height <= PT_MAX_IMAGE_DIM; ray_depth <= PT_MAX_RAY_DEPTH;
 *     spp <= PT_MAX_SPP (the reference GUI offers rayDepth 1..50 and SPP 1..10, src/Render/Gui.cs:40,48);
 *   - image rows: row 0 is the BOTTOM of the image (NDC y = -1), as in the GL image the reference writes
 *     (res/shaders/PathTracing/compute.glsl:104,114); pixels are RGBA32F, alpha = 1.
 */
#ifndef MI355PT_H
#define MI355PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define PT_API __declspec(dllexport)
#else
#define PT_API __attribute__((visibility("default")))
#endif

typedef struct pt_renderer *pt_handle;

enum {
    PT_OK = 0,
    PT_E_BAD_HANDLE = -1,
    PT_E_BAD_ARGUMENT = -2,  /* NULL pointer, bad dimensions, bad enum */
    PT_E_OUT_OF_RANGE = -3,  /* byteOffset/size outside the 144 B / 26,624 B / 464 B blobs (GL would raise INVALID_VALUE) */
    PT_E_NO_ENVIRONMENT = -4,/* pt_render before any environment map was set */
    PT_E_HIP = -5,           /* a HIP runtime call failed; message has the hipError string */
    PT_E_NO_DEVICE = -6,     /* no usable gfx950 device: the library has NO CPU fallback */
    PT_E_OUT_OF_MEMORY = -7
};

enum { PT_ENV_RGBA32F = 0, PT_ENV_SRGB8_A8 = 1 };

#define PT_BASIC_DATA_UBO_SIZE 144      /* src/MainWindow.cs:195-197 ; compute.glsl:59-64  */
#define PT_GAME_OBJECTS_UBO_SIZE 26624  /* src/MainWindow.cs:17,199-201 ; compute.glsl:66-70 */
#define PT_ATMOSPHERE_UBO_SIZE 464      /* src/Render/AtmosphericScatterer.cs:72 ; AtmosphericScattering/compute.glsl:11-15 */
#define PT_MAX_SPHERES 256
#define PT_MAX_CUBOIDS 64
#define PT_MAX_IMAGE_DIM 32767   /* pixel coordinates travel in 16-bit fields inside the kernels */
#define PT_MAX_RAY_DEPTH 4095    /* bounce counters travel in 12-bit fields */
#define PT_MAX_SPP 4095
#define PT_MAX_GROUP_DEVICES 16
#define PT_PRESENT_SLOTS 3       /* pinned host images of the non-blocking present path */

/* ---- lifetime -------------------------------------------------------------------------------------------- */

/* new PathTracer(env, width, height, ...) — src/Render/PathTracer.cs:95-110 — on HIP device `device_id`.
 * Allocates the RGBA32F accumulation image (the reference's `Result` texture, PathTracer.cs:97-99) ZEROED
 * (the reference leaves it undefined, src/Render/Objects/Texture.cs:169-197; frame 0 multiplies it by 0). */
PT_API int pt_create(int device_id, int width, int height, pt_handle *out);
PT_API int pt_destroy(pt_handle h);

/* The same renderer on n_devices GPUs of this process (no reference counterpart, the reference
 * owns one GL context): the image is tiled across device_ids[0..n) in block-cyclic bands of 8 rows = single tile rows (balanced: rows
 * near the floor cost ~2x sky rows; pt_multi_set_partition changes the band height or selects contiguous row
 * blocks), every device keeps its rows resident and renders them with global pixel coordinates, so the image is
 * bit-identical to the single-GPU one.  Nothing is exchanged per frame.  Every entry point accepts the group handle:
 * uploads / parameters / environment are replicated to all devices, pt_render enqueues on all of them, and
 * pt_read_result / pt_present_rgba8 / pt_present_rgba8_async GATHER the rows on device_ids[0] with peer copies over
 * xGMI (hipMemcpyPeerAsync; each peer has its own link to the root) before the single device-to-host copy.
 * device_ids may name the same device more than once (used to test the group path on a one-GPU box).
 * Not available on a group handle (PT_E_BAD_ARGUMENT): pt_set_tile, pt_set_interleaved_tile, pt_bind_result_buffer,
 * pt_set_stream, pt_postprocess_device.
 * Peer access: the gather wants hipDeviceCanAccessPeer == 1 in both directions between device_ids[0] and every other
 * device.  Where it is 0 (no xGMI / P2P disabled) the group is still created and renders the same bits, but its gather
 * is staged through host memory by the HIP runtime; pt_multi_gather_is_direct reports which one the handle got, and a
 * scaling measurement must refuse a staged group (bench.py and tools/multi_gpu_check.sh do). */
PT_API int pt_create_multi(const int *device_ids, int n_devices, int width, int height, pt_handle *out);
/* *out_direct = 1 when every gather copy of this handle goes over a direct peer link (always 1 for a one-GPU handle), 0 when the
 * runtime stages it through the host (see pt_create_multi). */
PT_API int pt_multi_gather_is_direct(pt_handle h, int *out_direct);
/* band_rows = 0: contiguous row blocks (device g owns rows [g*H/G, (g+1)*H/G)); else a multiple of 8: block-cyclic
 * bands of that many rows (default 8).  Resets the frame counter and zeroes, like pt_set_tile. */
PT_API int pt_multi_set_partition(pt_handle h, int band_rows);
/* Number of devices behind the handle (1 for pt_create handles). */
PT_API int pt_device_count_of(pt_handle h, int *out_n_devices);

/* PathTracer.SetSize — PathTracer.cs:131-135: frame counter = 0, image reallocated (and zeroed). The tile is
 * reset to the whole image. */
PT_API int pt_set_size(pt_handle h, int width, int height);

/* Multi-GPU row-block tiling (no reference counterpart: the reference is single-GPU).  This handle renders
 * and stores only rows [y0, y0+rows) of the width x height image; seeds and NDC still use global pixel
 * coordinates, so tiled and untiled renders are bit-identical.  Resets the frame counter and zeroes. */
PT_API int pt_set_tile(pt_handle h, int y0, int rows);

/* Block-cyclic variant of pt_set_tile for load balance across GPUs (rows near the floor cost ~2x sky rows): this handle
 * owns the bands rank, rank + world, rank + 2*world, ... of band_rows image rows each (band_rows a multiple of 8) and
 * stores them compactly, band after band.  Same bit-identical pixels; resets the frame counter and zeroes. */
PT_API int pt_set_interleaved_tile(pt_handle h, int rank, int world, int band_rows);

/* PathTracer.ResetRenderer — PathTracer.cs:137-140: frame counter = 0 (image contents are irrelevant then). */
PT_API int pt_reset(pt_handle h);

/* ---- inputs ------------------------------------------------------------------------------------------------ */

/* The six property setters NumSpheres/NumCuboids/RayDepth/SPP/FocalLength/ApertureDiameter —
 * PathTracer.cs:11-83 (GLSL uniforms compute.glsl:88-94). */
PT_API int pt_set_params(pt_handle h, int num_spheres, int num_cuboids, int ray_depth, int spp,
                         float focal_length, float aperture_diameter);

/* BasicDataUBO.SubData(offset, size, data) — src/MainWindow.cs:131-132,278-279: InvProjection@0, InvView@64,
 * ViewPos@128 (OpenTK row-major bytes, consumed as GLSL column-major). 0 <= offset, offset+size <= 144. */
PT_API int pt_upload_basic_data(pt_handle h, int byte_offset, int size, const void *src);

/* GameObjectsUBO.SubData(BufferOffset, size, data) — src/BaseSTD140Compatible.cs:12-16: std140 Spheres[256]@0
 * (80 B each), Cuboids[64]@20480 (96 B each). 0 <= offset, offset+size <= 26,624.  (The library shadows the block on the
 * host: scenes with >= 64 spheres get a sphere grid for their secondary rays, rebuilt before the next launch; results are
 * bit-identical to the reference's loop over all spheres.) */
PT_API int pt_upload_game_objects(pt_handle h, int byte_offset, int size, const void *src);

/* PathTracer.EnvironmentMap = <cube texture> — PathTracer.cs:85,118; cube creation src/MainWindow.cs:177-187,
 * src/Helper.cs:41-48.  faces[0..5] = +X,-X,+Y,-Y,+Z,-Z, each face_size^2 tightly packed RGBA texels
 * (float32 x4 for PT_ENV_RGBA32F, uint8 x4 sRGB-encoded for PT_ENV_SRGB8_A8), row 0 = t 0 as uploaded by
 * glTextureSubImage3D.  Sampling = GL LINEAR magnification with seamless cube edges (MainWindow.cs:168,178). */
PT_API int pt_set_environment(pt_handle h, int face_size, int format, const void *const faces[6]);

/* ---- the hot path ------------------------------------------------------------------------------------------ */

/* PathTracer.Render() — PathTracer.cs:114-123: enqueue one dispatch of the integrator with the current frame
 * index, then post-increment it. Asynchronous. *out_total_samples (optional) = frames * SPP after this call
 * (PathTracer.Samples, PathTracer.cs:112).
 * An upload / pt_set_params that repeats what the renderer already holds is NOT "something in between" (the reference re-uploads the
 * camera on every update, MainWindow.cs:131-132): it returns at once and changes nothing.
 * Frames of consecutive pt_render calls with nothing in between are launched as ONE pipelined kernel (up to
 * pt_set_frame_batch frames).  A frame is only held back while earlier frames of this handle are still running on the GPU
 * (so deferral never idles the device); the launch happens when the GPU has drained, when the batch is full, or at the next call of any other entry point
 * (uploads and parameter changes apply to LATER frames only, exactly as with one launch per call; every read,
 * pt_synchronize and pt_timer_* first launch what is pending).  The image is bit-identical either way.
 * Back-pressure: consecutive launches overlap on two internal streams (the second moves into the wavefront slots the first one's
 * drain frees), which needs the first one resident.  pt_render does not wait for that: a full batch whose predecessor is not resident
 * yet simply stays pending (the GPU has two launches queued, nothing idles) and is launched by a later call; only a host that runs
 * more than 16 launches ahead is held, for at most 2 ms per call.  Calls that block anyway (pt_synchronize, reads, presents) launch
 * what is pending and may wait for residency in between.  A single frame is launched that way too whenever the GPU still runs the
 * previous one.
 * pt_render cannot fail for a reason of the frame pipelining (PathTracer.cs:114-123 cannot either): a launch whose hand-over of a
 * pixel between two frames does not complete in time (a GPU shared with other work) abandons itself instead of producing a wrong
 * pixel, and the library re-renders exactly what is missing behind it before anything can observe the image. */
PT_API int pt_render(pt_handle h, int *out_total_samples);
/* Largest number of frames one launch may pipeline (1..64; 0 = back to automatic).  1 = NO deferral: every pt_render hands its frame to the
 * GPU at once (lowest latency: the interactive setting).  Since round 6 that does not mean one launch per frame: the first such
 * pt_render starts a FRAME-FED launch with room for 32 frames, and the calls that follow publish their frame into it (one store to a
 * host-mapped word; the resident wavefronts begin it as soon as they run out of earlier work), so frames of a host that renders faster
 * than the GPU pipeline like a batch (0.114 instead of 0.137 ms per 1080p frame).  Only full-size images of scenes whose kernel has a fed
 * instantiation (one sample per pixel, materials in LDS, no sphere grid) take that path; anything that changes an input or observes the
 * image closes the launch first, and a launch that waits 150 us for its next frame ends itself (the GPU is never held by a host that
 * has stopped rendering).  A handle on which this
 * was never called (or was last called with 0) pipelines up to 64 frames per launch — and up to 256 when it owns fewer than 12,000
 * tiles (a 1/8 share of a 1080p image: the fixed cost of a launch is 7 % of a 64-frame launch there); a limit set here is kept
 * exactly as given. */
PT_API int pt_set_frame_batch(pt_handle h, int max_frames);

/* What ScreenEffect.Render reads (src/MainWindow.cs:51): blocks until the stream is idle and copies this
 * handle's rows [y0, y0+rows) into dst (row_pitch_bytes >= width*16; 0 means tightly packed). */
PT_API int pt_read_result(pt_handle h, float *dst_rgba32f, size_t row_pitch_bytes);

/* The step right after the path ("next" row 1): ScreenEffect.Render(PathTracer.Result) —
 * src/Render/ScreenEffect.cs:29-37 with res/shaders/PostProcessing/fragment.glsl:17-44 — ACES tone map + gamma 2.4 into
 * an RGBA8 image (alpha 255), fused with the read-back: 4 B/pixel cross PCIe instead of 16.  Blocks like pt_read_result;
 * row_pitch_bytes >= width*4 (0 = tight).  pt_postprocess_device runs the same pass and returns the device copy (stream-
 * ordered, no host copy) so that a multi-GPU harness can gather RGBA8 rows instead of RGBA32F. */
PT_API int pt_present_rgba8(pt_handle h, uint8_t *dst_rgba8, size_t row_pitch_bytes);
PT_API int pt_postprocess_device(pt_handle h, void **out_device_ptr, size_t *out_bytes);

/* Non-blocking present for the reference's per-frame loop (src/MainWindow.cs:49-56: Render() -> PostProcesser.Render
 * (PathTracer.Result) -> blit, every frame).  pt_present_rgba8_async snapshots the image as it is after the frames
 * rendered so far: tone map (ACES + gamma, as pt_present_rgba8) into a device-side RGBA8 image of slot `slot`
 * (0 <= slot < PT_PRESENT_SLOTS), stream-ordered behind those frames, then a device-to-host copy into the library-owned
 * PINNED host image of that slot on a separate copy stream.  It returns at once; later pt_render calls only wait for
 * the (microseconds-long) tone-map pass, so frame f+1 renders while frame f's 4 B/pixel cross PCIe.
 * pt_present_wait blocks until the slot's copy has landed and returns the pinned image (tightly packed rows, row 0 =
 * bottom, valid until the next pt_present_rgba8_async on the same slot or pt_set_size/pt_destroy) and the frame index
 * (= number of accumulated frames) it shows.  Typical loop: render; present_async(f % 2); present_wait((f + 1) % 2) ->
 * upload to the GL texture -> swap.  Works on group handles (the gather of the RGBA8 rows happens on the copy stream).
 * On a single-GPU handle the presented frame comes from a SNAPSHOT that the integrator launch writes while it resolves that
 * frame's pixels, so the next pt_render does not wait for the tone map; once a host is seen to present every frame, pt_render
 * launches each frame with the snapshot attached (the image is unchanged; three internal buffers of width x rows x 16 bytes). */
PT_API int pt_present_rgba8_async(pt_handle h, int slot);
PT_API int pt_present_wait(pt_handle h, int slot, const uint8_t **out_host_rgba8, size_t *out_row_pitch_bytes,
                           int *out_frame_index);
/* Interop-style present (the library side of SURVEY section 8f row 4; no reference counterpart — the reference samples its GL
 * texture in place, src/Render/ScreenEffect.cs:29-37): make caller-owned DEVICE memory (>= rows*width*4 bytes, e.g. a GL buffer
 * registered with hipGraphicsGLRegisterBuffer and mapped) the image of present slot `slot`; NULL restores the library's own images.
 * pt_present_rgba8_async(slot) then tone-maps the frame straight into that memory and copies nothing to the host — the 8.3 MB
 * that a 1080p frame otherwise sends over PCIe; pt_present_wait(slot) returns once the image is complete there (out_host_rgba8
 * receives NULL, the frame index as usual).  Single-GPU handles only. */
PT_API int pt_present_bind_device_image(pt_handle h, int slot, void *device_rgba8, size_t bytes);

/* Resume support (no reference counterpart; the reference discards accumulation on every event): replace the
 * accumulation image of this tile and set the frame counter.  Alpha is stored as 1 whatever the source holds (the
 * reference always stores 1, compute.glsl:129; inside a pipelined launch the library uses alpha as a frame tag). */
PT_API int pt_write_result(pt_handle h, const float *src_rgba32f, size_t row_pitch_bytes, int frame_index);

PT_API int pt_get_frame_index(pt_handle h, int *out_frame_index);
/* Launch what is pending and wait for the handle's stream.  (A pipelined launch that abandoned a frame hand-over — see pt_render — has
 * been repaired when this returns: the image is the one an undisturbed run leaves; no error is reported for it.) */
PT_API int pt_synchronize(pt_handle h);

/* ---- atmosphere environment (secondary kernel) ------------------------------------------------------------- */

/* AtmosphericScatterer: UBO upload (src/Render/AtmosphericScatterer.cs:72-89: InvProjection@0 + 6 InvView@64),
 * the four uniforms (:11-57: ISteps, JSteps, lightPos from Time, LightIntensity) and Render() (:102-113),
 * into a size^2 x 6 RGBA32F cube that then becomes the environment (MainWindow.cs:189). */
PT_API int pt_atmosphere_upload_data(pt_handle h, int byte_offset, int size, const void *src);
PT_API int pt_atmosphere_render(pt_handle h, int size, int i_steps, int j_steps, const float light_pos[3],
                                float light_intensity);

/* Read back the current environment cube as RGBA32F (6 * face_size^2 * 4 floats), e.g. the atmosphere result
 * (the GUI shows / the tests check it).  sRGB environments are returned linearised. */
PT_API int pt_read_environment(pt_handle h, float *dst_rgba32f, int *out_face_size);

/* ---- plumbing for harnesses (torch.distributed, benchmarking); not part of the reference surface ----------- */

/* Device pointer + byte size of this tile's accumulation image (for zero-copy wrapping, e.g. the RCCL gather at
 * present time in multi-GPU runs). */
PT_API int pt_result_device_ptr(pt_handle h, void **out_device_ptr, size_t *out_bytes);
/* Render into caller-owned device memory (>= rows*width*16 bytes) instead of the internal image; NULL restores.
 * The buffer's RGB contents are taken as the accumulation so far (zero them for a fresh render: frame 0 multiplies
 * them by 0, and 0 * NaN is NaN as in the reference); its alpha channel is set to 1 at bind time (stream-ordered).
 * On the library's own stream the buffer must be observed through the library: while pt_render calls are outstanding its
 * alpha channel carries the frame tags of the pipelined launches, and pt_synchronize / pt_read_result /
 * pt_result_device_ptr restore alpha = 1 (the value the reference stores, compute.glsl:129) before they return.  On a
 * caller-owned stream (pt_set_stream) every frame stores alpha = 1 and stream order alone is enough. */
PT_API int pt_bind_result_buffer(pt_handle h, void *device_ptr, size_t bytes);
/* Use an existing hipStream_t (passed as void*) instead of the handle's own stream; NULL restores.  With a caller
 * stream every pt_render is enqueued on THAT stream before it returns (one launch per frame, no deferral, no
 * internal helper streams), so synchronising the stream is enough to observe the image. */
PT_API int pt_set_stream(pt_handle h, void *hip_stream);
/* hipEvent pair recorded on the handle's stream: elapsed GPU milliseconds between begin and end. */
PT_API int pt_timer_begin(pt_handle h);
PT_API int pt_timer_end(pt_handle h, float *out_milliseconds);
/* Kernel variant selector for A/B measurements; all variants produce bit-identical images.
 * 0 = default (persistent queue kernel), 1 = one wavefront per 8x8 tile, 2..6 = wave-local pools, 10+k = persistent
 * kernel with k+1 workgroups per CU. */
PT_API int pt_set_variant(pt_handle h, int variant);

enum { PT_ARITH_CONTRACT = 0, PT_ARITH_REFERENCE = 1 };
/* Arithmetic of the frames rendered after this call.  CONTRACT (default): the pt-f32 contract, fastest.
 * REFERENCE: the GL reference's own choices (never fused, correctly rounded / and sqrt, its summation orders
 * and built-ins) — bit-identical to the reference in ~98.6 % of pixels, several times slower (see DESIGN).
 * Frames issued before the call keep the arithmetic they were issued under; the accumulation is not reset (call
 * pt_reset for a clean image).  REFERENCE frames are plain single launches: no frame pipelining, no present
 * snapshots.  The atmosphere precompute has a switch of its own (pt_atmosphere_set_arithmetic) and is not affected
 * by this one, and so has the post-process tone map (pt_present_set_arithmetic): this switch does not select it.
 * Any other mode: PT_E_BAD_ARGUMENT. */
PT_API int pt_set_arithmetic(pt_handle h, int mode);
/* Arithmetic of the pt_atmosphere_render calls that follow (the reference's AtmosphericScatterer is an object of its
 * own, so is this switch): PT_ARITH_CONTRACT (default) or PT_ARITH_REFERENCE — the GL reference's own choices, within
 * 1e-4 of its cubes on every texel, at about the same speed (see DESIGN).  The current environment is not touched, nor is
 * pt_set_arithmetic's mode.  Everything else about pt_atmosphere_render is the same in both modes.  Any other
 * mode: PT_E_BAD_ARGUMENT, and the previous mode stays in force. */
PT_API int pt_atmosphere_set_arithmetic(pt_handle h, int mode);
/* Arithmetic of the tone map (res/shaders/PostProcessing/fragment.glsl:17-44, ScreenEffect.Render) of every present that
 * follows: pt_present_rgba8, pt_postprocess_device, every path of pt_present_rgba8_async (snapshot, row stripes,
 * accumulation image; slots bound with pt_present_bind_device_image included) and the per-device pass of a group handle
 * before its gather.  PT_ARITH_CONTRACT (default) or PT_ARITH_REFERENCE — the GL reference's own choices: multiply-adds
 * with two roundings, a true division, IEEE min / max for the clamp, its pow with the exponent (float)(1 / 2.4), and the
 * final mix(.., lessThan(..)) as a SELECT between v * 12.92 and the power branch; the float colour is then bit-identical
 * to the reference's on all 18,432 values of its fixture (see DESIGN).  The same in both modes: float -> unorm8 is
 * round-half-up of clamp(v, 0, 1) * 255 (the reference's fixture holds the shader's float colour only), a NaN colour is
 * clamped by IEEE minNum / maxNum and so becomes 0 (as do NaN and +-inf inputs; the reference's data holds none), alpha
 * is 255.  A switch of its own: it touches neither pt_set_arithmetic's nor pt_atmosphere_set_arithmetic's mode, nor the
 * accumulation image, the frame counter or the environment, and it fans out to every part of a group handle.  A call
 * that CHANGES the mode first launches what is pending and closes an open frame-fed launch (a call with the mode in
 * force does nothing and costs nothing, so a host may make it every frame); a present already in flight keeps the
 * arithmetic it was issued under.  While the mode is REFERENCE, a host that presents every frame into bound device images gets
 * snapshot or per-frame presents instead of the display fused into the frame-fed launch (that one is the contract's tone
 * map).  Any other mode: PT_E_BAD_ARGUMENT, and the previous mode stays in force. */
PT_API int pt_present_set_arithmetic(pt_handle h, int mode);

/* ---- first-hit query: "what is under this pixel?" ------------------------------------------------------------- */

/* The reference answers this on the CPU, with a second ray caster: src/Render/Gui.cs:223-233 -> MainWindow.RayTrace,
 * src/MainWindow.cs:302-318 (Sphere.IntersectsRay / Cuboid.IntersectsRay on a pinhole ray through the cursor: other formulas, no lens,
 * no sub-pixel offset, not the shader's entry-distance acceptance rule, compute.glsl:234,247 — so a click can select another object
 * than the one the rendered pixel shows, most often inside or near glass).  These calls replace it with the integrator's own ray:
 * for pixel (x, y) the record describes the first intersection of the ray of SAMPLE 0 OF FRAME frame_index, exactly as pt_render
 * traces it for that pixel and frame — seed from (x, y, frame), the two sub-pixel draws, GetWorldSpaceRay, the two lens draws with
 * the handle's current focal length and aperture, RayTrace over spheres 0..Ns-1 then cuboids 0..Nc-1 with the reference's
 * acceptance rule and visiting order — in the CONTRACT arithmetic, whatever the three arithmetic switches say.
 * Record = 32 bytes = 8 words, rows like the image (row 0 = bottom, global pixel coordinates under tiling):
 *   words 0-2 ray origin; word 3 t = the T RayTrace leaves (the smallest positive root: the EXIT distance when the origin lies inside
 *   the winner), +inf on a miss; words 4-6 ray direction; word 7 id as int32 bits: -1 miss, i = sphere i, PT_MAX_SPHERES + j = cuboid j.
 * Read: the current camera blob, scene blob and parameters.  Neither read nor written: the accumulation image, the frame counter, the
 * environment (none is needed), the three arithmetic switches.
 * With aperture > 0 that ray is one lens sample: near an out-of-focus silhouette the answer changes with frame_index.  That holds for
 * the default, PT_RAY_SAMPLE0, only: under PT_RAY_PINHOLE (pt_first_hit_set_ray) the record describes a stable ray, whatever the lens. */

/* Which ray the records describe (pt_first_hit_set_ray).  SAMPLE0: sample 0 of frame frame_index, as above.  PINHOLE: the pinhole ray
 * through the pixel's centre — what MainWindow.cs:302-318 aims at, a stable ray through the cursor, traced with the shader's own
 * RayTrace: the NDC point of compute.glsl:113-115 with both sub-pixel draws replaced by 0.5, GetWorldSpaceRay (:352-357), normalised;
 * origin = InvView's translation column (the origin of :120 at aperture 0, bit for bit); no lens, no RNG draw: frame_index, focal length
 * and aperture do not enter the result. */
enum { PT_RAY_SAMPLE0 = 0, PT_RAY_PINHOLE = 1 };
/* The ray of the pt_first_hit_render and pt_pick calls that follow (the click of Gui.cs:223-233 -> MainWindow.cs:302-318); what is
 * queued already keeps the ray it was issued under.  Default PT_RAY_SAMPLE0.  The record layout does not change, frame_index is still
 * validated, and nothing is read or written that the query did not touch before.  Any other mode: PT_E_BAD_ARGUMENT, and the previous
 * mode stays in force.  Works under pt_set_tile / pt_set_interleaved_tile; group handles: every device takes the mode. */
PT_API int pt_first_hit_set_ray(pt_handle h, int mode);

/* Gui.cs:223-233 / MainWindow.cs:302-318 for EVERY pixel of this handle's rows (an id / depth image for an outline or denoising
 * pass): stream-ordered and asynchronous; launches what is pending first.  The rows x width x 32-byte device buffer is allocated by
 * the first call after pt_set_size / pt_set_tile / pt_set_interleaved_tile, which free it (never by pt_render).
 * frame_index < 0: PT_E_BAD_ARGUMENT.  Group handles: every device renders its rows. */
PT_API int pt_first_hit_render(pt_handle h, int frame_index);
/* The records of the last pt_first_hit_render (Gui.cs:223-233 / MainWindow.cs:302-318 read their answer on the host as well): blocks,
 * copies this handle's rows into dst; row_pitch_bytes >= width*32, 0 = tightly packed.  Group handles gather the rows of all devices.
 * PT_E_BAD_ARGUMENT when nothing was rendered since the last pt_set_size / pt_set_tile / pt_set_interleaved_tile. */
PT_API int pt_first_hit_read(pt_handle h, void *dst, size_t row_pitch_bytes);
/* Device pointer + byte size of those records (stream-ordered behind the pt_first_hit_render that wrote them; valid until the next
 * resize / re-tiling), for a device-side consumer of the id / depth image — no counterpart in Gui.cs:223-233 / MainWindow.cs:302-318,
 * whose answer lives on the host.  Single-GPU handles only, like pt_postprocess_device. */
PT_API int pt_first_hit_device_ptr(pt_handle h, void **out, size_t *bytes);
/* MainWindow.RayTrace for one pixel — the call Gui.cs:223-233 makes on a click (MainWindow.cs:302-318): blocks; one 8x8-tile launch and
 * a 32-byte copy; the records of pt_first_hit_render are not touched.  *out_id as word 7 above; out_t, out_origin, out_dir may be
 * NULL (out_t: e.g. the FocalLength that focuses the lens on the object).  x / y outside the image, or — on a tiled handle — a row
 * the handle does not own: PT_E_OUT_OF_RANGE; out_id == NULL or frame_index < 0: PT_E_BAD_ARGUMENT.  Group handles: the device that
 * owns the row answers. */
PT_API int pt_pick(pt_handle h, int x, int y, int frame_index, int *out_id, float *out_t, float out_origin[3], float out_dir[3]);

/* ---- preview denoiser: guide buffers + an edge-avoiding a-trous filter ------------------------------------------ */

/* The reference shows the raw accumulation image (src/MainWindow.cs:49-56 -> src/Render/ScreenEffect.cs:29-37), and resets it on
 * every camera move, GUI edit and pick (MainWindow.cs:58-63): most of the time the user looks at frames 1..16, the noisiest images the
 * renderer makes.  These calls filter the image for display WITHOUT touching it: pt_denoise_render writes, into buffers of the
 * library, (1) a guide record per pixel from the integrator's own primary ray — 32 bytes = 8 words, rows like the image: words 0-2 hit
 * position P = origin + direction * t (two roundings per component), word 3 id as int32 bits, words 4-6 shading normal N as RayTrace
 * leaves it (not flipped when the origin lies inside the object; NaN on a cuboid's edges, as in the reference), word 7 t; id and t as
 * in the first-hit record; miss: id -1, t +inf, P = N = 0 — and (2) `iterations` passes of a 5x5 a-trous wavelet filter (Dammertz et
 * al. 2010) over the image's RGB, pass i with step 2^i, edge-stopping on id, normal, plane distance and tone-compressed luminance.
 * The definition, operation by operation (it is reproducible bit for bit in binary32), is DESIGN.md section 3.5.
 * SCOPE: single-GPU handles that own the whole image.  A group handle, or a handle under pt_set_tile (other than all rows) /
 * pt_set_interleaved_tile, gets PT_E_BAD_ARGUMENT from all of these calls: the filter reads up to 62 rows beyond a pixel's own.  With
 * aperture > 0 and the default switches the guides are lens-jittered like the first-hit record of PT_RAY_SAMPLE0: the filter is
 * specified, but its guides describe one lens sample of a pixel that shows the mean of many.  pt_denoise_set_lens is for that case. */

/* Filter parameters of the pt_denoise_render calls that follow — a GUI slider's setter, like those MainWindow.cs:49-63 drives; the result
 * is shown through ScreenEffect.cs:29-37.  iterations 0..6 (0 = the image is copied), sigma_color > 0 (luminance edge-stop; halves every
 * pass), sigma_plane > 0 (plane-distance edge-stop, relative to the pixel's t), normal_log2_power 0..7 (the normal weight is max(0, Np.Nq)
 * to the power 2^that).  Defaults 5, 0.5, 0.02, 5.  A non-finite sigma: PT_E_BAD_ARGUMENT; anything else outside its range:
 * PT_E_OUT_OF_RANGE; the previous values stay in force then. */
PT_API int pt_denoise_set_params(pt_handle h, int iterations, float sigma_color, float sigma_plane, int normal_log2_power);
/* Denoise the image as it stands, for the present of MainWindow.cs:49-63 / ScreenEffect.cs:29-37: stream-ordered and asynchronous.
 * Observes the image exactly as pt_postprocess_device does (pending frames are launched, an open frame-fed launch is closed, an
 * abandoned hand-over is repaired first) and reads its RGB only; renders the guides for sample 0 of frame guide_frame_index in the
 * CONTRACT arithmetic, then runs the passes.  Neither read nor written: the frame counter, the environment, the three arithmetic
 * switches; never written: the accumulation image.  The buffers (rows x width x 64 bytes) are allocated by the first call after
 * pt_set_size / pt_set_tile / pt_set_interleaved_tile, which free them (never by pt_render).  guide_frame_index < 0: PT_E_BAD_ARGUMENT. */
PT_API int pt_denoise_render(pt_handle h, int guide_frame_index);
/* The denoised image of the last pt_denoise_render as RGBA32F (alpha = 1), what MainWindow.cs:49-63 would hand to ScreenEffect.cs:29-37:
 * blocks; row_pitch_bytes >= width*16, 0 = tightly packed.  PT_E_BAD_ARGUMENT when nothing was rendered since the last (re)size / (re)tiling. */
PT_API int pt_denoise_read(pt_handle h, float *dst, size_t row_pitch_bytes);
/* The guide records of the last pt_denoise_render (no counterpart in MainWindow.cs:49-63 / ScreenEffect.cs:29-37: the reference has no
 * geometry buffers): blocks; 32 bytes per pixel, row_pitch_bytes >= width*32, 0 = tightly packed.  PT_E_BAD_ARGUMENT before the first render. */
PT_API int pt_denoise_read_guides(pt_handle h, void *dst, size_t row_pitch_bytes);
/* Device pointer + byte size of the denoised RGBA32F image (stream-ordered behind the pt_denoise_render that wrote it; valid until the
 * next pt_denoise_render, resize or re-tiling), for a device-side present in place of MainWindow.cs:49-63 / ScreenEffect.cs:29-37.
 * PT_E_BAD_ARGUMENT before the first render. */
PT_API int pt_denoise_device_ptr(pt_handle h, void **out, size_t *bytes);
/* pt_present_rgba8 of the denoised image: ScreenEffect.cs:29-37 (ACES + gamma, in the present arithmetic in force) over the result of
 * the last pt_denoise_render instead of the raw image of MainWindow.cs:49-63; blocks; row_pitch_bytes >= width*4, 0 = tightly packed.
 * PT_E_BAD_ARGUMENT before the first render. */
PT_API int pt_denoise_present_rgba8(pt_handle h, uint8_t *dst, size_t row_pitch_bytes);

/* Modes of the luminance edge-stop (pt_denoise_set_mode).  FIXED: one width for the whole image, sigma_color, halved every pass — the
 * filter above, bit for bit.  VARIANCE: the stop of every pixel is sigma_variance standard deviations of that pixel's own noise (the
 * variance-guided edge stop of Schied et al. 2017, SVGF), estimated spatially from the image itself; DESIGN.md section 3.5. */
enum { PT_DENOISE_FIXED = 0, PT_DENOISE_VARIANCE = 1 };
/* Mode of the pt_denoise_render calls that follow — a GUI toggle's setter, like those MainWindow.cs:49-63 drives; the result is shown
 * through ScreenEffect.cs:29-37; what is queued already keeps the mode it was issued under.  sigma_variance > 0: the width of the
 * luminance stop in standard deviations, stored in both modes.  Defaults PT_DENOISE_FIXED, 6.  In PT_DENOISE_VARIANCE a stage in front
 * of the passes estimates a variance per pixel (half the mean squared first difference of the tone-compressed luminance over the
 * pixels of the same id in a 7x7 window), the passes filter it along with the colour, and iterations, sigma_plane and
 * normal_log2_power of pt_denoise_set_params apply; sigma_color is not read, and nothing halves.  A non-finite sigma_variance or a mode
 * other than the two: PT_E_BAD_ARGUMENT; sigma_variance <= 0: PT_E_OUT_OF_RANGE; the previous values stay in force then.  Scope as for
 * pt_denoise_set_params. */
PT_API int pt_denoise_set_mode(pt_handle h, int mode, float sigma_variance);
/* The variance estimate of the last pt_denoise_render — the noise the filter saw in the image of MainWindow.cs:49-63 before it went to
 * ScreenEffect.cs:29-37, one float per pixel (variance of the tone-compressed luminance; 0 on a miss), rows like the image: blocks;
 * row_pitch_bytes >= width*4, 0 = tightly packed.  It doubles as a noise map: a host can stop showing the denoised image once the map
 * is flat.  PT_E_BAD_ARGUMENT when nothing was rendered since the last (re)size / (re)tiling, when the last render ran in
 * PT_DENOISE_FIXED, or with iterations = 0 (no estimate is made for a copy). */
PT_API int pt_denoise_read_variance(pt_handle h, float *dst, size_t row_pitch_bytes);

/* The temporal stage (the temporal half of SVGF, Schied et al. 2017): in front of the passes, the result of the
 * previous view is reprojected through the guide records and blended with the image by sample counts, so that the first frames after
 * the reset a camera move causes show tens of samples per pixel instead of one.  The handle keeps two SETS — an integrated image I
 * (RGBA32F: rgb, alpha = the per-pixel sample count), its guide records and its camera — the CURRENT one and the HISTORY, and counts
 * RESET EPOCHS: pt_reset, pt_write_result, pt_set_size, pt_set_tile and pt_set_interleaved_tile each begin a new one.  A temporal
 * pt_denoise_render whose current set is of an earlier epoch first makes it the history (a pointer swap); then it renders the guides,
 * integrates I(p) = ((n C + m' Hc) / (n + m'), n + m') — C the image, n = frame index * spp, Hc and m the history's colour and count
 * found at p's reprojected position among the pixels of p's id, m' = min(m, max_history) — or I(p) = (C, n) where nothing is found,
 * and filters I in the mode in force in place of the image.  Within one epoch repeated calls reuse the same history and integrate
 * afresh: nothing is counted twice.  n = 0 (a reset with no frame rendered yet) shows the old view warped to the new camera.  With
 * the stage off (the default) pt_denoise_render neither reads nor writes either set and its results are bit for bit what they were. */

/* Switch of the pt_denoise_render calls that follow — a GUI toggle's setter, like those MainWindow.cs:49-63 drives; the result is shown
 * through ScreenEffect.cs:29-37; what is queued already keeps the values it was issued under.  enable: 0 or 1, anything else
 * PT_E_BAD_ARGUMENT; max_history 1..65535 (the cap of the count a history pixel brings along: the smaller, the faster stale lighting
 * fades), outside that PT_E_OUT_OF_RANGE; the previous values stay in force then.  Defaults 0, 32.  Scope as for pt_denoise_set_params. */
PT_API int pt_denoise_set_temporal(pt_handle h, int enable, int max_history);
/* Forgets both sets: the next temporal pt_denoise_render finds no history (I = (C, n)) — what a host calls after a scene, material or
 * environment edit (the GUI edits beside the camera moves of MainWindow.cs:49-63, shown through ScreenEffect.cs:29-37), which changes
 * the colours the history holds, not only where they are seen from.  With pt_denoise_set_object_tracking on, an edit of the objects
 * (position, size, material, the counts) needs no clear: the stage follows or drops the edited object's history by itself.  An
 * environment edit, a pt_set_params change other than the counts (ray depth, spp, lens) and anything else the scene blob does not hold
 * still do.  Frees nothing.  Scope as for pt_denoise_set_params. */
PT_API int pt_denoise_history_clear(pt_handle h);
/* The integrated image I of the last pt_denoise_render made with the temporal stage on — the input of the passes in place of the image
 * of MainWindow.cs:49-63, before the filter and ScreenEffect.cs:29-37 — RGBA32F, alpha = the per-pixel sample count (it doubles as a
 * history-length map), rows like the image; row_pitch_bytes >= width*16, 0 = tightly packed.  PT_E_BAD_ARGUMENT when the last render
 * ran with the stage off, or when nothing was rendered since the last (re)size / (re)tiling. */
PT_API int pt_denoise_read_integrated(pt_handle h, float *dst, size_t row_pitch_bytes);
/* The history set the last temporal pt_denoise_render used (the previous view of MainWindow.cs:49-63, as it went to
 * ScreenEffect.cs:29-37's input): image = its I (width*height RGBA32F), guides = its 32-byte guide records (as pt_denoise_read_guides),
 * both tightly packed; out_B = the inverse of its camera's ray matrix, row-major, out_O = its ray origin (the InvView translation):
 * out_B (P - out_O) = lambda (ndc x, ndc y, 1) for a point P seen by that camera.  Every pointer may be NULL.  PT_E_BAD_ARGUMENT when
 * that render had no history (or none was made since the last (re)size / (re)tiling / pt_denoise_history_clear). */
PT_API int pt_denoise_read_history(pt_handle h, float *image, void *guides, float out_B[9], float out_O[3]);

/* Object tracking of the temporal stage, for the other everyday reset: the object-properties window,
 * Gui.cs:154-218 (Position drag :163-168, material fields :170-210, Upload + reset :212-216), MainWindow.cs:58-63.  Every temporal
 * pt_denoise_render keeps, with its set, a copy of the scene blob and the object counts.  With tracking on, a render with a valid history
 * compares that copy with the scene in force, object by object (guide ids are object indices), into an OBJECT MAP of 320 entries of 32
 * bytes, indexed by guide id (sphere i at i, cuboid j at PT_MAX_SPHERES + j): words 0-2 a.xyz, word 3 the state as int32 bits, words 4-6
 * b.xyz, word 7 zero.  PT_TRACK_DROP: the id is beyond either scene's count of its kind, or one of its 64 material bytes differs — its
 * pixels take no history (I = (C, n)).  PT_TRACK_KEEP (a = 1, b = 0): its geometry floats are bit-equal.  PT_TRACK_MOVED: they differ —
 * a translation or a resize, the edits of Gui.cs:163-168 / Cuboid.cs:23-24 — and history point = a * P + b per component carries the
 * object as it is onto the object as the history saw it (sphere: a = r_h / r_c; cuboid, per axis: a = extent_h / extent_c; in double,
 * rounded once; a radius or extent <= 0 or anything not finite: DROP): the history of a pixel is sought at that point instead of at P,
 * among the pixels of its id.  If every object that exists is KEEP and the counts are equal, the render is bit for bit what it is with
 * tracking off; otherwise the count a history pixel brings along is capped by min(max_history, edit_max_history) (edit_max_history 0:
 * by max_history), since the edit also changed the light that falls on everything else.  Through ScreenEffect.cs:29-37 as before. */
enum { PT_TRACK_KEEP = 0, PT_TRACK_MOVED = 1, PT_TRACK_DROP = 2 };
/* Switch of the pt_denoise_render calls that follow — what a host sets once, so that the Upload + reset of Gui.cs:154-218 (Position drag
 * :163-168, material fields :170-210, Upload + reset :212-216; the reset of MainWindow.cs:58-63) needs no pt_denoise_history_clear; the
 * result is shown through ScreenEffect.cs:29-37; what is queued already keeps the values it was issued under.  enable: 0 or 1, anything
 * else PT_E_BAD_ARGUMENT; edit_max_history 0..65535, outside that PT_E_OUT_OF_RANGE; the previous values stay in force then.  Defaults
 * 0, 0.  No effect unless pt_denoise_set_temporal is on.  Scope as for pt_denoise_set_params. */
PT_API int pt_denoise_set_object_tracking(pt_handle h, int enable, int edit_max_history);
/* The object map the last pt_denoise_render built for the edit of Gui.cs:154-218 (Position drag :163-168, material fields :170-210,
 * Upload + reset :212-216) that the reset of MainWindow.cs:58-63 followed, before its result went to ScreenEffect.cs:29-37: 320 entries of
 * 32 bytes as above into dst_320x32_bytes; *out_tracked = 1 if the scene differed and the tracked kernel ran, 0 if it was unchanged (all
 * KEEP).  Either pointer may be NULL.  PT_E_BAD_ARGUMENT when the last render ran with the temporal stage or this switch off, when it had
 * no valid history, or when nothing was rendered since the last (re)size / (re)tiling / pt_denoise_history_clear. */
PT_API int pt_denoise_read_object_map(pt_handle h, void *dst_320x32_bytes, int *out_tracked);

/* Lens mode of the pt_denoise_render calls that follow, for a host that renders with the lens open (the reference's own start:
 * new PathTracer(env, W, H, 13, 1, 20f, 0.14f), MainWindow.cs:189, shown through MainWindow.cs:49-63 / ScreenEffect.cs:29-37); what is
 * queued already keeps the values it was issued under.  enable = 1 changes two things.  (a) The guide records
 * come from the pinhole ray of PT_RAY_PINHOLE instead of sample 0 — same 32 bytes, same fields, the same rules; guide_frame_index is
 * validated and does not enter; stage V, the temporal stage and its sets consume them unchanged, and the temporal reprojection, which
 * always went through a pinhole camera, now meets guides of that camera.  (b) Every pixel gets a blur radius in pixels from its guide t,
 * c = (cocK |t - F|) / t, c = cocK on a miss, where cocK = coc_scale (A / 2) / F H / (2 |InvProjection[5]|) with the handle's aperture
 * A, focal length F and image height H (0 when A <= 0, F <= 0 or not finite).  A tap at Chebyshev distance r = step max(|dx|, |dy|)
 * from its centre p with r <= c(p) and r <= c(q) lies inside what the lens has already blurred at both ends: its id is not compared
 * and its normal and plane weights are 1; the luminance stop of the mode in force still applies.  Every other tap follows the rules
 * above, and a miss pixel still passes through.  coc_scale = 0: pinhole guides under the old tap rules.
 * enable other than 0 or 1, or a non-finite coc_scale: PT_E_BAD_ARGUMENT; coc_scale < 0: PT_E_OUT_OF_RANGE; the previous values stay in
 * force then.  Defaults 0, 1.  With enable = 0 pt_denoise_render is bit for bit what it was.  Scope as for pt_denoise_set_params. */
PT_API int pt_denoise_set_lens(pt_handle h, int enable, float coc_scale);

/* Temporal moments (the temporal-moments half of SVGF, Schied et al. 2017): a per-pixel noise estimate measured
 * ACROSS frames instead of across neighbours, for a host that keeps the denoised image on screen while the image of MainWindow.cs:49-63
 * converges behind it.  The spatial estimate V0 of PT_DENOISE_VARIANCE counts image detail inside one id (reflections, refractions) as
 * noise, so it stops falling while the true noise still does.  With the switch on, every pt_denoise_render OBSERVES the image: the
 * handle keeps a MOMENT SET — per pixel the luminance of the last observation and the running sum of squares M2, per handle the
 * observation count K and the sample count of the last observation — updated by the weighted Welford rule from the image alone (the
 * samples since the last look enter as their block mean, so a host may look every frame or every few), and forgotten (K = 0) when the
 * reset epoch or spp changes, the frame index goes back, or the handle is resized or re-tiled.  A render that finds the image as the
 * last observation saw it (or empty) counts nothing twice.  Vm = the variance of the tone-compressed luminance of the image as it
 * stands, M2 / (K - 1) / n carried through the tone curve; 0 on a miss and while K < 2.  In PT_DENOISE_VARIANCE with iterations > 0, the
 * temporal stage off and K >= 2, pass 0 reads var_0 = ((K - 1) Vt + prior_samples V0) / (K - 1 + prior_samples) in place of V0, Vt = the
 * mean of Vm over the pixels of the same id in the 3x3 window; pt_denoise_read_variance still returns V0.  In every other case the
 * filter's result is bit for bit what it is with the switch off, and the observations and the two read-outs below work all the same.
 * Limit: with the temporal stage on the passes filter the integrated image, whose noise is not the accumulation image's, so Vm is
 * measured and not used.  Reads the image's RGB only; touches neither the image, the frame counter nor anything pt_render reads. */

/* Switch of the pt_denoise_render calls that follow — a GUI toggle's setter, like those MainWindow.cs:49-63 drives; the result is shown
 * through ScreenEffect.cs:29-37; what is queued already keeps the values it was issued under.  enable: 0 or 1, anything else
 * PT_E_BAD_ARGUMENT; prior_samples 1..65535 (how many observations the spatial estimate is worth in the blend), outside that
 * PT_E_OUT_OF_RANGE; the previous values stay in force then.  Defaults 0, 32.  With enable = 0 pt_denoise_render is bit for bit what it
 * was, observes nothing and allocates nothing; the moment set stays as it is.  Scope as for pt_denoise_set_params. */
PT_API int pt_denoise_set_moments(pt_handle h, int enable, int prior_samples);
/* The noise map Vm of the last pt_denoise_render — how far the image of MainWindow.cs:49-63 still is from converged, before it goes to
 * ScreenEffect.cs:29-37 — one float per pixel (0 on a miss), rows like the image: blocks; row_pitch_bytes >= width*4, 0 = tightly
 * packed.  Unlike pt_denoise_read_variance's map this one does become flat where the image has detail.  PT_E_BAD_ARGUMENT when the last
 * render ran with the switch off, when fewer than two observations exist, when nothing was rendered since the last (re)size /
 * (re)tiling, for dst == NULL or a pitch smaller than a row. */
PT_API int pt_denoise_read_noise(pt_handle h, float *dst, size_t row_pitch_bytes);
/* The convergence figure of the image of MainWindow.cs:49-63 (what a host compares with a threshold to stop denoising, or rendering,
 * instead of showing ScreenEffect.cs:29-37 a filtered image for ever): *out_mean_variance = the mean of Vm over the pixels with id >= 0
 * (0 if there is none), *out_observations = K, *out_hit_pixels = that pixel count.  A device reduction forms one binary32 sum and one
 * count per 256 pixels; the host adds them in index order in double.  Blocks.  Any pointer may be NULL.  PT_E_BAD_ARGUMENT in the first
 * three cases of pt_denoise_read_noise. */
PT_API int pt_denoise_noise_level(pt_handle h, float *out_mean_variance, int *out_observations, int *out_hit_pixels);

/* The adaptive sampler's noise as the denoiser's, for a host that shows the denoised image of MainWindow.cs:49-63
 * while pt_adaptive_render (below) converges it.  An adaptively sampled image changes its noise level at every 8x8 tile border, and the
 * moments above are refused on it; but every pixel of a live adaptive state carries an exact estimate e of its own noise, in Vm's unit.
 * With the switch on, a pt_denoise_render in PT_DENOISE_VARIANCE with iterations > 0 on a live state reads, in pass 0, in place of V0:
 * var_0 = ((k - k0) Et + prior_samples V0) / (k - k0 + prior_samples), where (k, k0) is the record of the pixel's own tile, Et = S / k
 * and S = the mean of e(q) k_q over the pixels q of the same id in the 3x3 window, each with the count of its own tile — the window's
 * per-sample variance, carried to the pixel's own count; var_0 = V0 on a miss and where k - k0 <= 0.  pt_denoise_read_variance still
 * returns V0.  In every other case — no live state, PT_DENOISE_FIXED, iterations = 0 — the result is bit for bit what it is with the
 * switch off.  Stream-ordered behind the passes already queued; reads the adaptive state and writes neither it nor the image.  The
 * temporal stage and the moments stay refused on a live state. */

/* Switch of the pt_denoise_render calls that follow — a GUI toggle's setter, like those MainWindow.cs:49-63 drives; the result is shown
 * through ScreenEffect.cs:29-37; what is queued already keeps the values it was issued under.  enable: 0 or 1, anything else
 * PT_E_BAD_ARGUMENT; prior_samples 1..65535 (how many samples the spatial estimate is worth in the blend), outside that
 * PT_E_OUT_OF_RANGE; the previous values stay in force then.  Defaults 0, 8.  With enable = 0 pt_denoise_render is bit for bit what it
 * was and allocates nothing.  Scope as for pt_denoise_set_params. */
PT_API int pt_denoise_set_adaptive_noise(pt_handle h, int enable, int prior_samples);
/* var_0 of the last pt_denoise_render — the variance its pass 0 read in place of V0, how noisy the filter took the image of
 * MainWindow.cs:49-63 to be before the result went to ScreenEffect.cs:29-37, whether the switch above or pt_denoise_set_moments formed
 * it — one float per pixel, rows like the image: blocks; row_pitch_bytes >= width*4, 0 = tightly packed.  PT_E_BAD_ARGUMENT when the last render blended nothing (pass 0 read V0: pt_denoise_read_variance), when
 * nothing was rendered since the last (re)size / (re)tiling, for dst == NULL or a pitch smaller than a row. */
PT_API int pt_denoise_read_variance_used(pt_handle h, float *dst, size_t row_pitch_bytes);

/* ---- Adaptive sampling: per-tile sample counts driven by measured noise.  The reference spends every frame on every pixel
 * (PathTracer.cs:114-129); these entry points stop where the image is done and keep sampling where it is not.  The image is divided into
 * 8x8 tiles of the handle's own rows; every tile carries a record (k, k0, err, n): the samples its pixels hold, the count the statistics
 * started at, the tile's noise estimate and its in-image pixel count.  One PASS gives every ACTIVE tile — k < max_samples and
 * (k - k0 < min_samples - 1 or err > threshold), re-evaluated from the stored record at the start of every pass — one more frame with the
 * tile's own frame index k.  A pixel's sample for frame index k depends on (x, y, k) and the inputs only, so a pixel that has received k
 * samples holds bit for bit what k pt_render frames leave there.  err = the mean over the tile's pixels of e = M2 / ((k - k0) k) /
 * (1 + l)^4, the variance of the pixel's mean carried to the tone-compressed luminance u = l / (1 + l) — pt_denoise_noise_level's unit —
 * with M2 the Welford sum recovered from the running mean before and after each fold (the definition: DESIGN.md section 3.5).
 * While an adaptive state is LIVE — from the pt_adaptive_render that initialises it until pt_reset, pt_write_result, pt_set_size,
 * pt_set_tile, pt_set_interleaved_tile or pt_bind_result_buffer — pixels hold different sample counts: pt_get_frame_index keeps returning
 * the frame index F the state started from, pt_render and a pt_denoise_render with the temporal stage or the moments on return
 * PT_E_BAD_ARGUMENT and touch nothing, until pt_reset or pt_adaptive_end; everything that only reads the image works unchanged.  A live
 * state can be saved and restored (pt_adaptive_read_m2, pt_adaptive_write_state) and left without losing the image (pt_adaptive_end).  A
 * host that never calls
 * pt_adaptive_render is not affected in any way.  Single-GPU handles, under pt_set_tile / pt_set_interleaved_tile too; a group handle:
 * PT_E_BAD_ARGUMENT. */

/* threshold: a variance of u, finite and >= 0 (else PT_E_BAD_ARGUMENT); min_samples 2..65535, max_samples min_samples..65535 (else
 * PT_E_OUT_OF_RANGE); the previous values stay in force on an error.  Defaults 1e-4f (a standard deviation of 0.01, about 2.5 of the 255
 * display levels before gamma), 8, 1024.  Read by the passes enqueued after the call. */
PT_API int pt_adaptive_set_params(pt_handle h, float threshold, int min_samples, int max_samples);
/* Enqueues `passes` passes (1..65535, else PT_E_OUT_OF_RANGE) on the stream in force: asynchronous, stream-ordered.  Pending pt_render
 * frames are launched first.  Without a live state one is initialised from the frame index F: every tile k = F, k0 = max(F, 1),
 * statistics zero — so a host may render its first frames with pt_render and go on adaptively, or start from frame 0.  The buffers (16
 * bytes per tile, 8 per pixel) are allocated by the first call after a (re)size or (re)tiling.  PT_E_BAD_ARGUMENT under
 * pt_set_arithmetic(PT_ARITH_REFERENCE); PT_E_NO_ENVIRONMENT without an environment. */
PT_API int pt_adaptive_render(pt_handle h, int passes);
/* Blocks.  *out_active_tiles = the tiles still active under the parameters in force, *out_tiles = the tile count, *out_pixel_samples =
 * the sum over the pixels of their sample counts x spp, *out_min_count / *out_max_count = the smallest and largest k.  Any pointer may be
 * NULL.  PT_E_BAD_ARGUMENT without a live state. */
PT_API int pt_adaptive_status(pt_handle h, int *out_active_tiles, int *out_tiles, int64_t *out_pixel_samples, int *out_min_count,
                              int *out_max_count);
/* Blocks.  ceil(width / 8) x ceil(rows / 8) records of 16 bytes, row-major, tile row 0 = the handle's rows 0..7: (int32 k, int32 k0,
 * float err, int32 n).  PT_E_BAD_ARGUMENT without a live state or for dst == NULL. */
PT_API int pt_adaptive_read_tiles(pt_handle h, void *dst_16_bytes_per_tile);
/* Blocks.  The per-pixel estimate e (the heat map a GUI would show), one float per pixel, rows like the image; row_pitch_bytes >=
 * width*4, 0 = tightly packed.  PT_E_BAD_ARGUMENT without a live state, for dst == NULL or a pitch smaller than a row. */
PT_API int pt_adaptive_read_noise(pt_handle h, float *dst, size_t row_pitch_bytes);
/* Blocks.  The per-pixel Welford sum M2, laid out like pt_adaptive_read_noise's map, with the same refusals.  With pt_read_result,
 * pt_get_frame_index (F) and pt_adaptive_read_tiles this is the whole state: e and err are functions of these. */
PT_API int pt_adaptive_read_m2(pt_handle h, float *dst, size_t row_pitch_bytes);
/* Blocks.  Installs a live state: the image and frame index F as pt_write_result(image, F) installs them (alpha forced to 1, a new reset
 * epoch), the records' (k, k0, n) and M2 as given, e and err rebuilt from them bit for bit as the pass that left the state wrote them.
 * From here every read-out and every later pass equals those of the handle the state was read from, given the same inputs.  Everything
 * is checked first, and a refused call touches nothing — not the image, the frame index, the reset epoch nor a live state:
 * PT_E_BAD_ARGUMENT for a NULL pointer, a pitch smaller than a row (0 = tightly packed) or frame_index < 0; PT_E_OUT_OF_RANGE unless
 * every record has n = the tile's in-image pixel count, k0 = max(frame_index, 1) and frame_index <= k <= 65535.  err in the records is
 * not read; M2 is taken as bits (any float).  Needs neither an environment nor the contract arithmetic: the next pt_adaptive_render
 * makes its own checks.  The buffers are allocated if the handle has none. */
PT_API int pt_adaptive_write_state(pt_handle h, const float *image_rgba32f, size_t image_pitch_bytes, int frame_index,
                                   const void *tiles_16_bytes_per_tile, const float *m2, size_t m2_pitch_bytes);
/* Levels and leaves: with kmax / kmin the largest / smallest k of the records, enqueues kmax - kmin passes in which exactly the tiles
 * with k < kmax are active (the pt_adaptive_set_params values are neither read nor changed), ends the state as pt_bind_result_buffer ends
 * it — no new reset epoch: the accumulation continues — and sets the frame index to kmax (*out_frame_index, may be NULL).  The image then
 * equals kmax pt_render frames bit for bit; pt_render, the temporal stage and the moments are accepted again.  Blocks only to fetch the
 * records.  PT_E_BAD_ARGUMENT without a live state; when passes are needed (kmin < kmax) pt_adaptive_render's preconditions apply with
 * its error codes, and a refused call touches nothing.  A state that never diverged ends without a launch. */
PT_API int pt_adaptive_end(pt_handle h, int *out_frame_index);

PT_API const char *pt_last_error(pt_handle h);
PT_API const char *pt_version(void);
PT_API int pt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_H */
