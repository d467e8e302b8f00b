"""Accumulation checkpoints and screenshots.

The reference has no restartable renders; its only persistence is the GUI's screenshot button (Gui.cs:28-33 ->
Framebuffer.cs:67-82: read the displayed RGBA8 image back, flip it vertically because GL rows are bottom-up, write a
PNG).  On top of pt_read_result / pt_write_result this module adds
  * save_checkpoint / load_checkpoint: the raw RGBA32F accumulation image + frame index + the parameters the image is
    only valid for, so that a long progressive render continues bit-identically after a restart;
  * save_screenshot: the tone-mapped RGBA8 image (pt_present_rgba8) as a PNG, flipped like the reference's.
File format, version 1 (little endian): 8-byte magic "PTCKPT1\\0", int32 x 8 (width, image height, y0, rows, band_rows, band_world,
band_rank, frame index), int32 x 2 (ray depth, spp), float32 x 2 (focal length, aperture), then rows*width*4 float32.
Version 2, written for a tracer whose adaptive state is live (PathTracer.AdaptiveLive) — pixels then hold
different sample counts and the frame index alone does not describe the image: 8-byte magic "PTCKPT2\\0", the version 1 header fields
unchanged (frame index = the F the state started from), float32 threshold, int32 min_samples, int32 max_samples, int32 tiles_y,
int32 tiles_x (= ceil(rows / 8), ceil(width / 8)), the image as in version 1, tiles_y*tiles_x records of 16 bytes (int32 k, int32 k0,
float32 err, int32 n), then the per-pixel Welford sums M2 as rows*width float32.  Loading it restores a live state
(PathTracer.RestoreAdaptive, which rebuilds the per-pixel estimate and the tiles' err) and the parameters (SetAdaptive).  Without a
live state save_checkpoint writes version 1; both versions load.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

MAGIC = b"PTCKPT1\0"
MAGIC_V2 = b"PTCKPT2\0"
_HEADER = struct.Struct("<8s8i2i2f")
_ADAPTIVE = struct.Struct("<f4i")  # threshold, min_samples, max_samples, tiles_y, tiles_x
TILE_DTYPE = np.dtype([("k", "<i4"), ("k0", "<i4"), ("err", "<f4"), ("n", "<i4")])


class CheckpointError(ValueError):
    pass


def write_checkpoint_file(path, image: np.ndarray, *, width, height, y0, rows, band_rows=0, band_world=1, band_rank=0,
                          frame_index, ray_depth, spp, focal_length, aperture) -> None:
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.shape != (rows, width, 4):
        raise CheckpointError(f"image shape {img.shape} does not match rows x width x 4 = {(rows, width, 4)}")
    with open(path, "wb") as f:
        f.write(_HEADER.pack(MAGIC, width, height, y0, rows, band_rows, band_world, band_rank, frame_index, ray_depth, spp,
                             float(focal_length), float(aperture)))
        f.write(img.tobytes())


def write_adaptive_checkpoint_file(path, image: np.ndarray, tiles: np.ndarray, m2: np.ndarray, *, width, height, y0, rows, band_rows=0,
                                   band_world=1, band_rank=0, frame_index, ray_depth, spp, focal_length, aperture, threshold, min_samples,
                                   max_samples) -> None:
    """Version 2: a live adaptive state (the image, the tile records and the per-pixel M2) with the sampler's parameters."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.shape != (rows, width, 4):
        raise CheckpointError(f"image shape {img.shape} does not match rows x width x 4 = {(rows, width, 4)}")
    tiles_y, tiles_x = (rows + 7) // 8, (width + 7) // 8
    rec = np.ascontiguousarray(tiles)
    if rec.shape != (tiles_y, tiles_x) or rec.dtype.itemsize != 16:
        raise CheckpointError(f"tile records {rec.shape} do not match ceil(rows / 8) x ceil(width / 8) = {(tiles_y, tiles_x)} records of 16 bytes")
    sums = np.ascontiguousarray(m2, dtype=np.float32)
    if sums.shape != (rows, width):
        raise CheckpointError(f"M2 shape {sums.shape} does not match rows x width = {(rows, width)}")
    with open(path, "wb") as f:
        f.write(_HEADER.pack(MAGIC_V2, width, height, y0, rows, band_rows, band_world, band_rank, frame_index, ray_depth, spp,
                             float(focal_length), float(aperture)))
        f.write(_ADAPTIVE.pack(float(threshold), int(min_samples), int(max_samples), tiles_y, tiles_x))
        f.write(img.tobytes())
        f.write(rec.tobytes())
        f.write(sums.tobytes())


def read_checkpoint_file(path):
    """-> (header dict, (rows, width, 4) float32 image).  The header says which `version` the file is; a version 2 header also carries
    threshold, min_samples, max_samples, tiles ((tiles_y, tiles_x) records, TILE_DTYPE) and m2 ((rows, width) float32)."""
    with open(path, "rb") as f:
        raw = f.read(_HEADER.size)
        if len(raw) != _HEADER.size:
            raise CheckpointError("truncated checkpoint header")
        magic, width, height, y0, rows, band_rows, band_world, band_rank, frame, depth, spp, focal, aperture = _HEADER.unpack(raw)
        if magic not in (MAGIC, MAGIC_V2):
            raise CheckpointError("not a mi355pt checkpoint (bad magic)")
        if width <= 0 or rows < 0 or frame < 0:
            raise CheckpointError("corrupt checkpoint header")
        hdr = dict(version=1 if magic == MAGIC else 2, width=width, height=height, y0=y0, rows=rows, band_rows=band_rows, band_world=band_world,
                   band_rank=band_rank, frame_index=frame, ray_depth=depth, spp=spp, focal_length=focal, aperture=aperture)
        tiles = 0
        if magic == MAGIC_V2:
            raw = f.read(_ADAPTIVE.size)
            if len(raw) != _ADAPTIVE.size:
                raise CheckpointError("truncated checkpoint header")
            threshold, min_samples, max_samples, tiles_y, tiles_x = _ADAPTIVE.unpack(raw)
            if (tiles_y, tiles_x) != ((rows + 7) // 8, (width + 7) // 8):
                raise CheckpointError(f"checkpoint tile grid {tiles_y} x {tiles_x} does not match rows = {rows}, width = {width}")
            if not (threshold >= 0.0 and threshold != float("inf")) or not 2 <= min_samples <= max_samples <= 65535:
                raise CheckpointError("corrupt checkpoint header (adaptive parameters)")
            hdr.update(threshold=threshold, min_samples=min_samples, max_samples=max_samples)
            tiles = tiles_y * tiles_x
        data = f.read()
    pixels = rows * width
    want = pixels * 16 + (tiles * 16 + pixels * 4 if magic == MAGIC_V2 else 0)
    if len(data) != want:
        raise CheckpointError(f"checkpoint payload is {len(data)} bytes, expected {want}")
    if magic == MAGIC_V2:
        hdr["tiles"] = np.frombuffer(data, dtype=TILE_DTYPE, count=tiles, offset=pixels * 16).reshape(tiles_y, tiles_x).copy()
        hdr["m2"] = np.frombuffer(data, dtype=np.float32, count=pixels, offset=pixels * 16 + tiles * 16).reshape(rows, width).copy()
    return hdr, np.frombuffer(data, dtype=np.float32, count=pixels * 4).reshape(rows, width, 4).copy()


def save_checkpoint(path, tracer) -> None:
    """Dump `tracer`'s tile (all of the image on one GPU) with everything needed to validate a later load: version 2 with the adaptive
    state while one is live, version 1 otherwise."""
    common = dict(width=tracer.Width, height=tracer.Height, y0=tracer.y0, rows=tracer.rows,
                  band_rows=tracer.band_rows, band_world=tracer.band_world, band_rank=tracer.band_rank,
                  ray_depth=tracer.RayDepth, spp=tracer.SPP, focal_length=tracer.FocalLength,
                  aperture=tracer.ApertureDiameter)
    if getattr(tracer, "AdaptiveLive", False):
        state = tracer.AdaptiveState()
        threshold, min_samples, max_samples = tracer.AdaptiveParams
        write_adaptive_checkpoint_file(path, state["image"], state["tiles"], state["m2"], frame_index=state["frame_index"], threshold=threshold,
                                       min_samples=min_samples, max_samples=max_samples, **common)
        return
    write_checkpoint_file(path, tracer.Result, frame_index=tracer.FrameIndex, **common)


def load_checkpoint(path, tracer, strict: bool = True) -> dict:
    """Restore image + frame index into `tracer`.  The tile geometry must match; with `strict` the integrator parameters
    must match too (an image accumulated with other parameters is not a sample of the same estimator)."""
    hdr, img = read_checkpoint_file(path)
    # the whole tile geometry must match: under block-cyclic ownership every rank has y0 = 0 and often the same row
    # count, so band height / world size / rank are what tell one rank's rows from another's
    geo = dict(width=tracer.Width, height=tracer.Height, y0=tracer.y0, rows=tracer.rows, band_rows=tracer.band_rows)
    if tracer.band_rows:
        geo.update(band_world=tracer.band_world, band_rank=tracer.band_rank)
    for k, v in geo.items():
        if hdr[k] != v:
            raise CheckpointError(f"checkpoint {k} = {hdr[k]} but the renderer has {v}")
    if strict:
        par = dict(ray_depth=tracer.RayDepth, spp=tracer.SPP)
        for k, v in par.items():
            if hdr[k] != v:
                raise CheckpointError(f"checkpoint {k} = {hdr[k]} but the renderer has {v} (pass strict=False to override)")
        if np.float32(hdr["focal_length"]) != np.float32(tracer.FocalLength) or np.float32(hdr["aperture"]) != np.float32(tracer.ApertureDiameter):
            raise CheckpointError("checkpoint lens parameters differ from the renderer's (pass strict=False to override)")
    if hdr["version"] == 2:
        # the records must describe this geometry and this frame index (what pt_adaptive_write_state would refuse)
        rec, frame = hdr["tiles"], hdr["frame_index"]
        h = np.minimum(8, hdr["rows"] - 8 * np.arange(rec.shape[0]))
        w = np.minimum(8, hdr["width"] - 8 * np.arange(rec.shape[1]))
        if (rec["n"] != h[:, None] * w[None, :]).any() or (rec["k0"] != max(frame, 1)).any() or (rec["k"] < frame).any() or (rec["k"] > 65535).any():
            raise CheckpointError("checkpoint tile records are inconsistent with the geometry or the frame index")
        if not hasattr(tracer, "RestoreAdaptive"):
            raise CheckpointError("the checkpoint holds an adaptive state, which this renderer cannot restore")
        tracer.RestoreAdaptive(img, frame, rec, hdr["m2"])
        tracer.SetAdaptive(hdr["threshold"], hdr["min_samples"], hdr["max_samples"])
        return hdr
    tracer.WriteResult(img, hdr["frame_index"])
    return hdr


def encode_png(rgba8: np.ndarray, flip_vertically: bool = True) -> bytes:
    """Minimal PNG (8-bit RGB, no alpha: the reference saves the opaque displayed image).  `rgba8` is (H, W, 3|4) uint8 with
    row 0 = bottom of the image (GL order); flip_vertically=True writes it top-down like Framebuffer.cs:79."""
    img = np.ascontiguousarray(rgba8[..., :3], dtype=np.uint8)
    if flip_vertically:
        img = img[::-1]
    h, w = img.shape[:2]
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def decode_png_rgb8(data: bytes) -> np.ndarray:
    """Inverse of encode_png for the files it writes (filter type 0 only) — used by the tests."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(tag + body) & 0xFFFFFFFF), "PNG chunk CRC"
        if tag == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert (depth, ctype) == (8, 2)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3).copy()


def save_screenshot(path, tracer) -> None:
    """Gui.cs:28-33 screenshot: the displayed (tone-mapped) image as PNG, flipped vertically (Framebuffer.cs:67-82)."""
    with open(path, "wb") as f:
        f.write(encode_png(tracer.Present(), flip_vertically=True))
