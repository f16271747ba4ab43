"""Python plumbing over libdsrt_hip.so (tests, bench and the multi-GPU launcher use it).

The product is the shared library and its C ABI (include/dsrt.h); this package only moves pointers and sizes across
that boundary.  It is imported as `dsrt_amd` (see dsrt_amd.py at the repository root: the directory name mandated for
the package contains hyphens and cannot be written in an import statement).
"""
import ctypes as C

import numpy as np

try:
    # PyTorch-ROCm ships its own libamdhip64.so.7; two HIP runtimes in one process cannot both see the GPU.  Importing torch
    # first makes the dynamic loader bind libdsrt_hip.so to that same runtime (same SONAME).  torch is plumbing only
    # (device buffers, streams, torch.distributed in bench.py); the library itself has no torch dependency.
    import torch as _torch  # noqa: F401
except ImportError:  # pragma: no cover
    _torch = None

from . import capi
from .capi import (DsrtAccum, DsrtFrame, DsrtGBuffer, DsrtPose, DsrtRayHits, DsrtRays, DsrtRenderDesc, DsrtStats, GPUCamera, GPUScene)

lib = capi.load()


class DsrtError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib.dsrt_last_error()
        super().__init__(f"{where} failed with {code}: {msg.decode() if msg else ''}")


def _check(rc, where):
    if rc != 0:
        raise DsrtError(rc, where)


def _f3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


def _poses(poses):
    p = np.ascontiguousarray(poses, dtype=np.float32)
    if p.size % 12:
        raise ValueError("poses: 12 floats per body")
    return p.reshape(-1, 12)


class HostScene:
    """Flattened scene + BVH on the host (DsrtHostScene)."""

    def __init__(self):
        self._h = lib.dsrt_host_scene_create()
        self._built = False

    def close(self):
        if self._h and lib is not None:
            lib.dsrt_host_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def add_obj(self, path, scale=1.0):
        _check(lib.dsrt_host_scene_add_obj(self._h, str(path).encode(), float(scale)), "dsrt_host_scene_add_obj")
        self._built = False
        return self

    def add_world_file(self, path):
        _check(lib.dsrt_host_scene_add_world_file(self._h, str(path).encode()), "dsrt_host_scene_add_world_file")
        self._built = False
        return self

    def add_arrays(self, tris=None, spheres=None, mats=None):
        def arr(a, dt):
            a = np.ascontiguousarray(a if a is not None else np.zeros(0, dt), dtype=dt)
            return a, (a.ctypes.data if a.size else None), int(a.size)
        t, tp, tn = arr(tris, capi.TRI_DTYPE)
        s, sp, sn = arr(spheres, capi.SPHERE_DTYPE)
        m, mp, mn = arr(mats, capi.MAT_DTYPE)
        _check(lib.dsrt_host_scene_add_arrays(self._h, tp, tn, sp, sn, mp, mn), "dsrt_host_scene_add_arrays")
        self._built = False
        return self

    def add_texture_file(self, path, flip_vertically=True):
        """Texture slot of an image file (decoded into the scene's pool as the reference's builder decodes map_Kd files); the id a triangle added with
        add_arrays carries in albedo_tex.  flip_vertically: the state of the reference's global stb flag (True once any MTL named a map)."""
        slot = lib.dsrt_host_scene_add_texture_file(self._h, str(path).encode(), 1 if flip_vertically else 0)
        if slot < 0:
            _check(slot, "dsrt_host_scene_add_texture_file")
        return slot

    def build_bvh(self, kind="median"):
        """kind "median": the reference's tree (parity); "sah": binned-SAH tree, "lbvh": linear BVH built on the GPU -- non-parity fast modes."""
        if kind == "median":
            _check(lib.dsrt_host_scene_build_bvh(self._h), "dsrt_host_scene_build_bvh")
        elif kind == "sah":
            _check(lib.dsrt_host_scene_build_bvh_sah(self._h), "dsrt_host_scene_build_bvh_sah")
        elif kind == "bodies":                       # one subtree per body under a chain of top nodes (include/dsrt.h, MOVABLE RIGID BODIES)
            _check(lib.dsrt_host_scene_build_bvh_bodies(self._h), "dsrt_host_scene_build_bvh_bodies")
        elif kind == "lbvh":                         # built on the GPU (device 0 unless set_lbvh_device says otherwise)
            ms, tot = C.c_float(), C.c_float()
            _check(lib.dsrt_host_scene_build_bvh_gpu(self._h, int(getattr(self, "lbvh_device", 0)), C.byref(ms), C.byref(tot)), "dsrt_host_scene_build_bvh_gpu")
            self.lbvh_build_ms, self.lbvh_total_ms = ms.value, tot.value
        else:
            raise ValueError("build_bvh kind must be 'median', 'sah', 'lbvh' or 'bodies'")
        self._built = True
        return self

    def begin_body(self):
        """Start a movable body (dsrt_host_scene_begin_body): triangles added from now on belong to it.  Returns its index, 1 .. 15."""
        b = lib.dsrt_host_scene_begin_body(self._h)
        if b < 0:
            _check(b, "dsrt_host_scene_begin_body")
        return b

    @property
    def body_count(self):
        return lib.dsrt_host_scene_body_count(self._h)

    def body_range(self, body):
        """(first triangle, number of triangles) of a body."""
        first, n = C.c_int(), C.c_int()
        _check(lib.dsrt_host_scene_body_range(self._h, int(body), C.byref(first), C.byref(n)), "dsrt_host_scene_body_range")
        return first.value, n.value

    def build_bvh_bodies(self):
        return self.build_bvh("bodies")

    def set_body_poses(self, first_body, poses):
        """The CPU statement of Context.set_body_poses: `poses` is (count, 12) float32, row-major 3x4 [R | t], applied to the REST pose."""
        p = _poses(poses)
        _check(lib.dsrt_host_scene_set_body_poses(self._h, int(first_body), int(p.shape[0]), p.ctypes.data if p.size else None), "dsrt_host_scene_set_body_poses")
        return self

    @property
    def texture_failures(self):
        """Paths of texture maps that could not be decoded (their texel is the reference's 1x1 white fallback)."""
        buf = C.create_string_buffer(1 << 16)
        n = lib.dsrt_host_scene_texture_failures(self._h, buf, len(buf))
        return [p for p in buf.value.decode(errors="replace").split("\n") if p][:n] if n else []

    @property
    def stack_need(self):
        return lib.dsrt_host_scene_bvh_stack_need(self._h)

    def view(self, camera=None, sun_dir=None):
        """GPUScene with HOST pointers (valid while this object lives and is not modified)."""
        if not self._built:
            self.build_bvh()
        s = GPUScene()
        _check(lib.dsrt_host_scene_view(self._h, C.byref(s)), "dsrt_host_scene_view")
        if camera is not None:
            lib.dsrt_scene_set_frame(C.byref(s), C.byref(camera), _f3(sun_dir if sun_dir is not None else (0.0, -1.0, 0.0)))
        return s

    def arrays(self):
        """numpy copies of the flattened arrays, in the reference layouts."""
        s = self.view()

        def grab(ptr, n, dt):
            if not ptr or n == 0:
                return np.zeros(0, dt)
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt).copy()
        return {
            "tris": grab(s.triangles, s.num_triangles, capi.TRI_DTYPE),
            "spheres": grab(s.spheres, s.num_spheres, capi.SPHERE_DTYPE),
            "mats": grab(s.materials, s.num_materials, capi.MAT_DTYPE),
            "idx": grab(s.tri_indices, s.num_triangles if s.tri_indices else 0, np.dtype("<i4")),
            "nodes": grab(s.bvh_nodes, s.num_bvh_nodes, capi.NODE_DTYPE),
            "texhdr": grab(s.textures, s.num_textures, capi.TEXHDR_DTYPE),
            "texpool": grab(s.texture_pool, s.texture_pool_floats, np.dtype("<f4")),
        }


def read_pose_file(path):
    n = C.c_int(0)
    rc = lib.dsrt_read_pose_file(str(path).encode(), None, 0, C.byref(n))
    _check(rc, "dsrt_read_pose_file")
    poses = (DsrtPose * n.value)()
    _check(lib.dsrt_read_pose_file(str(path).encode(), poses, n.value, C.byref(n)), "dsrt_read_pose_file")
    return list(poses)


def pose_to_frame(pose):
    f = DsrtFrame()
    _check(lib.dsrt_pose_to_frame(C.byref(pose), C.byref(f)), "dsrt_pose_to_frame")
    return f


def pose_to_model(pose, xyz, direction=False):
    """World-frame points (or, with direction=True, directions) of a pose's epoch into the model frame the scene lives in (dsrt_pose_points_to_model /
    dsrt_pose_dirs_to_model): `xyz` of shape (3,) or (N, 3), computed in float64 as the pose file holds it; returns float32 of the same shape."""
    a = np.ascontiguousarray(xyz, dtype=np.float64)
    if a.ndim not in (1, 2) or a.shape[-1] != 3:
        raise ValueError(f"pose_to_model: xyz must have shape (3,) or (N, 3), not {a.shape}")
    flat = a.reshape(-1, 3)
    out = np.empty(flat.shape, np.float32)
    fn = lib.dsrt_pose_dirs_to_model if direction else lib.dsrt_pose_points_to_model
    _check(fn(C.byref(pose), int(flat.shape[0]), flat.ctypes.data, out.ctypes.data), fn.__name__)
    return out.reshape(a.shape)


def camera_look_at(lookfrom, lookat, vfov, width, height, spp, max_depth):
    cam = GPUCamera()
    _check(lib.dsrt_camera_look_at(C.byref(cam), _f3(lookfrom), _f3(lookat), float(vfov), int(width), int(height), int(spp), int(max_depth)),
           "dsrt_camera_look_at")
    return cam


def frame_camera(frame, vfov, width, height, spp, max_depth):
    """Camera for one pose frame: at cam_in_model, looking at the model origin (src/main.cpp:399)."""
    return camera_look_at(tuple(frame.cam_in_model), (0.0, 0.0, 0.0), vfov, width, height, spp, max_depth)


def decode_image_file(path, flip_vertically=False):
    """The builder's texture decoder on one file -> H x W x 3 uint8 (dsrt_decode_image_file)."""
    w, h = C.c_int(), C.c_int()
    _check(lib.dsrt_decode_image_file(str(path).encode(), int(bool(flip_vertically)), C.byref(w), C.byref(h), None, 0), "dsrt_decode_image_file")
    out = np.zeros((h.value, w.value, 3), np.uint8)
    _check(lib.dsrt_decode_image_file(str(path).encode(), int(bool(flip_vertically)), C.byref(w), C.byref(h), out.ctypes.data, out.size), "dsrt_decode_image_file")
    return out


def write_ppm(path, rgb, width, height):
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    _check(lib.dsrt_write_ppm(str(path).encode(), rgb.ctypes.data, int(width), int(height)), "dsrt_write_ppm")


def write_png(path, rgb, width, height):
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    _check(lib.dsrt_write_png(str(path).encode(), rgb.ctypes.data, int(width), int(height)), "dsrt_write_png")


def write_pfm(path, data):
    """Portable float map of an (H, W) or (H, W, 3) float array in image order (top row first); dsrt_write_pfm stores it bottom-up."""
    a = np.ascontiguousarray(data, dtype=np.float32)
    ch = 1 if a.ndim == 2 else a.shape[2]
    _check(lib.dsrt_write_pfm(str(path).encode(), a.ctypes.data, int(a.shape[1]), int(a.shape[0]), int(ch)), "dsrt_write_pfm")


def make_desc(width, height, spp, max_depth=50, gamma=2.0, seed=1337, tile_size=0, shard_rank=0, shard_count=0,
              collect_counters=0, checked=0, stack_entries=0, tune=(0, 0, 0, 0), rng_mode=0, math_mode=0):
    d = DsrtRenderDesc()
    d.width, d.height, d.spp, d.max_depth, d.gamma, d.seed = int(width), int(height), int(spp), int(max_depth), float(gamma), int(seed)
    d.rng_mode = int(rng_mode)
    d.math_mode = int(math_mode)
    d.tile_size, d.shard_rank, d.shard_count = int(tile_size), int(shard_rank), int(shard_count)
    d.collect_counters, d.checked, d.stack_entries = int(collect_counters), int(checked), int(stack_entries)
    for i, v in enumerate(tuple(tune) + (0,) * (4 - len(tune))):
        d.tune[i] = int(v)
    return d


DENOISE_GUIDES = ("normal", "position", "albedo", "range")            # DsrtDenoiseGuides' channels: G-buffer channels of those names (capi.GBUFFER_CHANNELS)


def _defaults(struct, fill, changes):
    """A `struct` as the library's `fill` function leaves it, with `changes` = {field: value} applied."""
    p = struct()
    fill(C.byref(p))
    for k, v in changes.items():
        if k not in dict(struct._fields_):
            raise ValueError(f"{struct.__name__} has no field {k!r}")
        setattr(p, k, v)
    return p


def denoise_defaults(**changes):
    """dsrt_denoise_defaults: the DsrtDenoise the library fills (iterations, normal_power_log2, sigma_l, sigma_z, sigma_a), with `changes` applied."""
    return _defaults(capi.DsrtDenoise, lib.dsrt_denoise_defaults, changes)


def coverage_desc(pattern=None, samples=None):
    """A DsrtCoverageDesc (include/dsrt.h, COVERAGE): dsrt_coverage_defaults' (DIAGONAL, 64) with `pattern` ("grid" / "diag" or capi.COVERAGE_*) and `samples`
    (S of an S x S grid, or the n of the diagonal) applied.  A string "grid:S" / "diag:N" sets both."""
    d = capi.DsrtCoverageDesc()
    lib.dsrt_coverage_defaults(C.byref(d))
    if isinstance(pattern, str) and ":" in pattern:
        pattern, samples = pattern.split(":", 1)
    if pattern is not None:
        names = {"grid": capi.COVERAGE_GRID, "diag": capi.COVERAGE_DIAGONAL, "diagonal": capi.COVERAGE_DIAGONAL}
        if isinstance(pattern, str) and pattern not in names:
            raise ValueError(f"unknown coverage pattern {pattern!r}; known: {sorted(names)}")
        d.pattern = names[pattern] if isinstance(pattern, str) else int(pattern)
    if samples is not None:
        d.samples = int(samples)
    return d


def coverage_classes(ranges):
    """A DsrtCoverageClasses of up to 16 triangle ranges [(first, num), ...], e.g. HostScene.body_range(b) per body."""
    ranges = list(ranges)
    if len(ranges) > 16:
        raise ValueError("at most 16 classes")
    cl = capi.DsrtCoverageClasses()
    cl.count = len(ranges)
    for c, (first, num) in enumerate(ranges):
        cl.first[c], cl.num[c] = int(first), int(num)
    return cl


def coverage_alpha_min():
    """dsrt_denoise_coverage_alpha_min: the default alpha_min of the coverage-aware denoiser."""
    return float(lib.dsrt_denoise_coverage_alpha_min())


def temporal_defaults(**changes):
    """dsrt_temporal_defaults: the DsrtTemporal the library fills (alpha_min, normal_cos_min, plane_tol, min_support), with `changes` applied."""
    return _defaults(capi.DsrtTemporal, lib.dsrt_temporal_defaults, changes)


def temporal_shading(flags_ptr, edge_guard=1):
    """A DsrtTemporalShading (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING): flags_ptr the address of the current G-buffer's flags channel (a device
    address for the device form, a host address for the host form: an int, a ctypes.c_void_p or None), edge_guard 0 or 1."""
    return capi.DsrtTemporalShading(flags_ptr, int(edge_guard))


UPSCALE_GUIDES = DENOISE_GUIDES + ("flags",)                         # DsrtUpscaleGuides' channels; "flags" (uint8) is the optional one


def upscale_coverage_alpha_min():
    """dsrt_upscale_coverage_alpha_min: the default alpha_min of the coverage-aware upscaler and of the denoiser in front of it."""
    return float(lib.dsrt_upscale_coverage_alpha_min())


def upscale_defaults(**changes):
    """dsrt_upscale_defaults: the DsrtUpscale the library fills (normal_power_log2, sigma_z, sigma_a, use_sun), with `changes` applied."""
    return _defaults(capi.DsrtUpscale, lib.dsrt_upscale_defaults, changes)


def sensor_psf_gaussian(sigma, size):
    """dsrt_sensor_psf_gaussian: a normalised size x size Gaussian PSF (float32, row-major) for sensor_defaults(psf=...)."""
    taps = np.zeros((int(size), int(size)), np.float32)
    _check(lib.dsrt_sensor_psf_gaussian(float(sigma), int(size), taps.ctypes.data), "dsrt_sensor_psf_gaussian")
    return taps


def sensor_defaults(psf=None, **changes):
    """dsrt_sensor_defaults (include/dsrt.h, SENSOR MODEL): the DsrtSensor the library fills, with `changes` applied.  psf: a square float32 array of odd size
    (1 .. 33), kept alive by the struct it is set in; None = no blur."""
    p = _defaults(capi.DsrtSensor, lib.dsrt_sensor_defaults, changes)
    if psf is not None:
        taps = np.ascontiguousarray(psf, np.float32)
        if taps.ndim != 2 or taps.shape[0] != taps.shape[1]:
            raise ValueError(f"psf must be a square 2-D array, not {taps.shape}")
        p.psf, p.psf_size = taps.ctypes.data, taps.shape[0]
        p._keep_psf = taps
    return p


def write_pnm16(path, dn, bits):
    """dsrt_write_pnm16: a raw frame (H, W) or (H, W, 3) of uint16 DN from a `bits`-bit ADC as P5 / P6 with maxval 2^bits - 1."""
    a = np.ascontiguousarray(dn, dtype=np.uint16)
    ch = 1 if a.ndim == 2 else a.shape[2]
    _check(lib.dsrt_write_pnm16(str(path).encode(), a.ctypes.data, int(a.shape[1]), int(a.shape[0]), int(ch), (1 << int(bits)) - 1), "dsrt_write_pnm16")


def stars_from_catalog(ra_deg, dec_deg, mag, flux_mag0=(1.0, 1.0, 1.0)):
    """dsrt_stars_from_catalog (include/dsrt.h, POINT SOURCES): a catalogue of right ascensions, declinations (degrees) and magnitudes as (dirs, flux) -- float64 (N, 3)
    unit directions in the catalogue's frame (pose_to_model(pose, dirs, direction=True) brings them into the model frame) and float32 (N, 3) fluxes,
    flux_mag0 * 10^(-0.4 mag) per channel."""
    ra, dec, m = (np.ascontiguousarray(x, np.float64).reshape(-1) for x in (ra_deg, dec_deg, mag))
    if not (ra.size == dec.size == m.size):
        raise ValueError(f"stars_from_catalog: {ra.size} right ascensions, {dec.size} declinations, {m.size} magnitudes")
    f0 = np.ascontiguousarray(flux_mag0, np.float32).reshape(3)
    dirs, flux = np.zeros((ra.size, 3), np.float64), np.zeros((ra.size, 3), np.float32)
    _check(lib.dsrt_stars_from_catalog(int(ra.size), ra.ctypes.data, dec.ctypes.data, m.ctypes.data, f0.ctypes.data, dirs.ctypes.data, flux.ctypes.data), "dsrt_stars_from_catalog")
    return dirs, flux


def synthetic_star_catalog(seed, count, mag_min=0.0, mag_max=6.5):
    """dsrt_stars_synthetic_catalog: (ra_deg, dec_deg, mag), float64 (count,) each -- uniform on the sphere, magnitudes in [mag_min, mag_max] with N(< m) ~ 10^(0.5 m)."""
    ra, dec, m = (np.zeros(int(count), np.float64) for _ in range(3))
    _check(lib.dsrt_stars_synthetic_catalog(int(seed), int(count), float(mag_min), float(mag_max), ra.ctypes.data, dec.ctypes.data, m.ctypes.data), "dsrt_stars_synthetic_catalog")
    return ra, dec, m


def lens_defaults(**changes):
    """dsrt_lens_defaults (include/dsrt.h, LENS MODEL): the DsrtLens the library fills -- filter 2 (Catmull-Rom), channels 3, clamp_zero 1, everything else 0 -- with
    `changes` applied.  The caller sets the two frames: src_width, src_height, src_fx .. src_cy and fx .. cy (lens_intrinsics_from_camera gives the library's own)."""
    return _defaults(capi.DsrtLens, lib.dsrt_lens_defaults, changes)


def lens_distort_points(params, xy):
    """dsrt_lens_distort_points: positions `xy` (N, 2) in the SOURCE frame, in pixels -- star centroids, prev_xy, keypoints -- through the forward model of `params`
    (a DsrtLens) into the distorted frame.  Returns (xy_out float32 (N, 2), ok uint8 (N,)); a point that is not finite has ok 0 and comes out as (0, 0)."""
    src = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out, ok = np.zeros_like(src), np.zeros(len(src), np.uint8)
    _check(lib.dsrt_lens_distort_points(C.byref(params), len(src), src.ctypes.data, out.ctypes.data, ok.ctypes.data), "dsrt_lens_distort_points")
    return out, ok


def lens_intrinsics_from_camera(cam, width, height):
    """dsrt_lens_intrinsics_from_camera: (fx, fy, cx, cy) of the library's own pinhole for the GPUCamera `cam` at width x height, as Python floats (float32 values)."""
    out = np.zeros(4, np.float32)
    _check(lib.dsrt_lens_intrinsics_from_camera(C.byref(cam), int(width), int(height), out.ctypes.data), "dsrt_lens_intrinsics_from_camera")
    return tuple(float(v) for v in out)


def aligned_zeros(count, dtype=np.float32, align=64):
    """A zeroed numpy array of `count` elements whose data starts on an `align`-byte boundary (a host history buffer must be 16-byte aligned)."""
    raw = np.zeros(count * np.dtype(dtype).itemsize + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + count * np.dtype(dtype).itemsize].view(dtype)


def shard_layout(desc):
    total, mine, padded, nbytes = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    _check(lib.dsrt_shard_layout(C.byref(desc), C.byref(total), C.byref(mine), C.byref(padded), C.byref(nbytes)), "dsrt_shard_layout")
    return {"tiles_total": total.value, "tiles_this_shard": mine.value, "tiles_per_shard_padded": padded.value, "rgb8_bytes_padded": nbytes.value}


def selftest_rccl_gather(device=0, nbytes=1 << 20):
    """dsrt_selftest_rccl_gather: a one-rank RCCL communicator and one checked ncclGather on `device`."""
    _check(lib.dsrt_selftest_rccl_gather(int(device), int(nbytes)), "dsrt_selftest_rccl_gather")


def set_experiment(word):
    """Development switches of the A/B tools (include/dsrt.h, dsrt_dev_set_experiment): process-wide, undefined bits refused."""
    _check(lib.dsrt_dev_set_experiment(int(word) & 0xFFFFFFFF), "dsrt_dev_set_experiment")


def microbench_copy(nbytes=2 << 30, blocks_per_cu=8, reps=8, device=0, mode=0):
    """HBM streaming calibration (include/dsrt.h): float4 grid-stride kernel; mode 0 copy (GB/s counts bytes read + written), 1 read only, 2 write only, 3 non-temporal copy."""
    ms, moved = C.c_float(), C.c_double()
    _check(lib.dsrt_microbench_copy(int(device), int(mode), int(nbytes), int(blocks_per_cu), int(reps), C.byref(ms), C.byref(moved)), "dsrt_microbench_copy")
    return {"mode": ("copy", "read only", "write only", "non-temporal copy")[mode], "bytes_per_buffer": int(nbytes), "blocks_per_cu": blocks_per_cu, "reps": reps, "ms": ms.value,
            "GBps": moved.value / ms.value / 1e6}


def microbench_gather(mode=0, dependent=False, live_lanes=64, pad_valu=0, table_bytes=19 << 20, iters=2000, device=0):
    """Gather-rate calibration kernel (include/dsrt.h): returns {"ms", "records", "Grecords_per_s"}."""
    ms, rec = C.c_float(), C.c_double()
    _check(lib.dsrt_microbench_gather(int(device), int(mode), int(bool(dependent)), int(live_lanes), int(pad_valu), int(table_bytes), int(iters),
                                      C.byref(ms), C.byref(rec)), "dsrt_microbench_gather")
    return {"mode": mode, "dependent": bool(dependent), "live_lanes": live_lanes, "pad_valu": pad_valu, "table_MB": table_bytes / 2**20, "iters": iters,
            "ms": ms.value, "records": rec.value, "Grecords_per_s": rec.value / ms.value / 1e6}


VALU_KINDS = tuple(lib.dsrt_microbench_valu_kind_name(k).decode() for k in range(lib.dsrt_microbench_valu_kinds()))


def microbench_valu(kind=0, waves_per_simd=8, iters=20000, lane_mask=(1 << 64) - 1, pattern=0, device=0, simds=1024):
    """VALU issue-cost calibration (include/dsrt.h).  `kind`: index or name (VALU_KINDS).  cycles_per_instruction_per_simd is for the stream as issued:
    with pattern 1 or 2 half of the instructions are v_add_f32."""
    if isinstance(kind, str):
        kind = VALU_KINDS.index(kind)
    ms, n, ghz = C.c_float(), C.c_double(), C.c_double()
    _check(lib.dsrt_microbench_valu(int(device), int(kind), int(pattern), int(waves_per_simd), int(iters), int(lane_mask), C.byref(ms), C.byref(n), C.byref(ghz)),
           "dsrt_microbench_valu")
    gips = n.value / ms.value / 1e6
    return {"kind": VALU_KINDS[kind], "pattern": ("x32", "alternating with v_add_f32", "pairs between pairs of v_add_f32", "x16 then v_add_f32 x16", "alternating with v_pk_mul_f32", "x16 then v_pk_mul_f32 x16")[pattern], "waves_per_simd": waves_per_simd, "iters": iters,
            "lanes": bin(lane_mask).count("1"), "ms": ms.value, "wave_instructions": n.value, "G_wave_instructions_per_s": gips, "shader_clock_GHz": ghz.value,
            "cycles_per_instruction_per_simd": simds * ghz.value / gips}


def _body_motion(first_tri, num_tris, poses_prev, poses_cur, prim_id_ptr):
    """(DsrtBodyMotion, the arrays that keep its HOST pointers alive) of the bodies' triangle ranges (HostScene.body_range) and two sets of poses, (bodies, 12) or
    (bodies, 3, 4) each, entry 0 ignored; prim_id_ptr: the G-buffer channel, wherever the form has its buffers."""
    first, num = np.ascontiguousarray(first_tri, np.int32).reshape(-1), np.ascontiguousarray(num_tris, np.int32).reshape(-1)
    pp, pc = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (poses_prev, poses_cur))
    if not (len(first) == len(num) and pp.size == pc.size == 12 * len(first)):
        raise ValueError(f"body motion: {len(first)} first_tri, {len(num)} num_tris, {pp.size} and {pc.size} pose floats do not describe one set of bodies")
    m = capi.DsrtBodyMotion(len(first), first.ctypes.data, num.ctypes.data, pp.ctypes.data, pc.ctypes.data, prim_id_ptr)
    return m, (first, num, pp, pc)


def body_motion_host(first_tri, num_tris, poses_prev, poses_cur, prim_id, normal, position):
    """dsrt_body_motion_host: the CPU statement of the motion rule (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES) over n points: prim_id int32 (n,), normal and
    position float32 (n, 3).  Returns (prev_normal, prev_position) = (N', X'), float32 (n, 3)."""
    prim = np.ascontiguousarray(prim_id, np.int32).reshape(-1)
    N, X = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (normal, position))
    if not len(prim) == len(N) == len(X):
        raise ValueError("prim_id, normal and position must describe the same points")
    m, keep = _body_motion(first_tri, num_tris, poses_prev, poses_cur, prim.ctypes.data)
    n2, x2 = np.zeros_like(N), np.zeros_like(X)
    _check(lib.dsrt_body_motion_host(C.byref(m), len(prim), _array_ptr(N), _array_ptr(X), _array_ptr(n2), _array_ptr(x2)), "dsrt_body_motion_host")
    return n2, x2


def stats_dict(st):
    return {name: getattr(st, name) for name, _ in DsrtStats._fields_}


def _tensor_ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _array_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


_OUTPUTS = {"rgb8": (np.uint8, (3,)), "f32": (np.float32, (3,)), "linear": (np.float32, (3,)), "var": (np.float32, (3,)), "prev_xy": (np.float32, (2,)),
            "weight": (np.float32, ()), "support": (np.float32, ()), "prev_position": (np.float32, (3,)), "status": (np.uint8, ()),
            "level": (np.uint8, ())}


def _outputs(desc, wants, device=None):
    """The outputs of a sample-set frame that `wants` = {name of _OUTPUTS: asked for?} names, in its order, None for one not asked for: torch tensors on `device`
    (uninitialised), or zeroed numpy arrays where there is none."""
    out = []
    for name, want in wants.items():
        dt, tail = _OUTPUTS[name]
        shape = (desc.height, desc.width) + tail
        out.append(None if not want else np.zeros(shape, dt) if device is None else _torch.empty(shape, dtype=getattr(_torch, np.dtype(dt).name), device=device))
    return tuple(out)


class Context:
    """One GPU: resident scene in traversal layout + render launches (DsrtContext)."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib.dsrt_ctx_create(int(device), C.byref(h)), "dsrt_ctx_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.dsrt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def clone(self):
        """A second context on the same device sharing this one's resident scene (dsrt_ctx_clone)."""
        h = C.c_void_p()
        _check(lib.dsrt_ctx_clone(self._h, C.byref(h)), "dsrt_ctx_clone")
        other = Context.__new__(Context)
        other._h, other.device = h, self.device
        return other

    def set_certified_tree(self, on=True):
        """The next upload also builds the certified second tree (include/dsrt.h): rays walk a SAH tree, the kernel certifies every answer against the reference tree."""
        _check(lib.dsrt_ctx_set_certified_tree(self._h, 1 if on else 0), "dsrt_ctx_set_certified_tree")
        return self

    @property
    def has_certified_tree(self):
        return bool(lib.dsrt_ctx_has_certified_tree(self._h))

    def upload(self, scene_host_view):
        _check(lib.dsrt_scene_upload(self._h, C.byref(scene_host_view)), "dsrt_scene_upload")

    def upload_device(self, scene_device_view):
        _check(lib.dsrt_scene_upload_device(self._h, C.byref(scene_device_view)), "dsrt_scene_upload_device")

    def upload_bodies(self, host_scene, frame):
        """Upload a HostScene that carries the bodies tree and keep resident what set_body_poses needs (dsrt_scene_upload_bodies); `frame` is a GPUScene that
        supplies camera, params and Sun (e.g. host_scene.view(camera, sun))."""
        _check(lib.dsrt_scene_upload_bodies(self._h, host_scene._h, C.byref(frame)), "dsrt_scene_upload_bodies")

    @property
    def body_count(self):
        return lib.dsrt_ctx_body_count(self._h)

    def set_body_poses(self, first_body, poses, stream=None, want_ms=False):
        """Pose bodies first_body ... of the resident scene on the device (dsrt_scene_set_body_poses; synchronous).  want_ms: returns (total, transform, refit, chain) ms."""
        p = _poses(poses)
        ms = C.c_float()
        _check(lib.dsrt_scene_set_body_poses(self._h, int(first_body), int(p.shape[0]), p.ctypes.data if p.size else None, C.c_void_p(stream) if stream else None,
                                             C.byref(ms) if want_ms else None), "dsrt_scene_set_body_poses")
        if not want_ms:
            return None
        split = (C.c_float * 3)()
        _check(lib.dsrt_ctx_body_update_ms(self._h, split), "dsrt_ctx_body_update_ms")
        return (ms.value, *split)

    def read_scene_words(self, array, first_word=0, n_words=None):
        """Test hook (dsrt_selftest_read_scene_words): 32-bit words of a resident array -- 0 node records, 1 triangle pair records, 2 shading records.
        n_words None: everything from first_word on."""
        if n_words is None:                          # (out = NULL: the hook only says whether the range lies inside the array)
            inside = lambda n: lib.dsrt_selftest_read_scene_words(self._h, int(array), int(first_word), n, None) == 0
            lo, hi = 0, 1
            while inside(hi):
                lo, hi = hi, hi * 2
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if inside(mid) else (lo, mid)
            n_words = lo
        out = np.zeros(int(n_words), np.uint32)
        _check(lib.dsrt_selftest_read_scene_words(self._h, int(array), int(first_word), int(n_words), out.ctypes.data), "dsrt_selftest_read_scene_words")
        return out

    def set_camera_sun(self, camera, sun_dir):
        _check(lib.dsrt_scene_set_camera_sun(self._h, C.byref(camera), _f3(sun_dir)), "dsrt_scene_set_camera_sun")

    def render(self, desc, d_rgb8_ptr, d_f32_ptr=None, stream=None, want_stats=False):
        """Launch on `stream` (raw hipStream_t as int); with want_stats the call synchronises and returns DsrtStats."""
        st = DsrtStats() if want_stats else None
        rc = lib.dsrt_render(self._h, C.byref(desc), C.c_void_p(d_rgb8_ptr), C.c_void_p(d_f32_ptr) if d_f32_ptr else None,
                             C.c_void_p(stream) if stream else None, C.byref(st) if st is not None else None)
        _check(rc, "dsrt_render")
        return st

    def render_batch(self, desc, cameras, sun_dirs, d_rgb8_ptr, d_f32_ptr=None, stream=None, want_stats=False):
        """dsrt_render_batch: len(cameras) views of the resident scene as one launch; the images land one after another in d_rgb8."""
        n = len(cameras)
        cams = (GPUCamera * n)(*cameras)
        suns = (C.c_float * (3 * n))(*[float(v) for s in sun_dirs for v in s])
        st = DsrtStats() if want_stats else None
        rc = lib.dsrt_render_batch(self._h, C.byref(desc), n, cams, suns, C.c_void_p(d_rgb8_ptr), C.c_void_p(d_f32_ptr) if d_f32_ptr else None,
                                   C.c_void_p(stream) if stream else None, C.byref(st) if st is not None else None)
        _check(rc, "dsrt_render_batch")
        return st

    def deinterleave(self, desc, d_gathered_ptr, d_image_ptr, stream=None):
        _check(lib.dsrt_deinterleave_tiles(self._h, C.byref(desc), C.c_void_p(d_gathered_ptr), C.c_void_p(d_image_ptr),
                                           C.c_void_p(stream) if stream else None), "dsrt_deinterleave_tiles")

    def deinterleave_batch(self, desc, frames, d_gathered_ptr, d_images_ptr, stream=None):
        """dsrt_deinterleave_batch: the gathered compact buffers of sharded batch launches -> `frames` whole images."""
        _check(lib.dsrt_deinterleave_batch(self._h, C.byref(desc), int(frames), C.c_void_p(d_gathered_ptr), C.c_void_p(d_images_ptr),
                                           C.c_void_p(stream) if stream else None), "dsrt_deinterleave_batch")

    def render_to_host(self, desc, want_f32=False):
        n = desc.width * desc.height * 3
        rgb = np.zeros(n, np.uint8)
        f32 = np.zeros(n, np.float32) if want_f32 else None
        st = DsrtStats()
        rc = lib.dsrt_render_to_host(self._h, C.byref(desc), rgb.ctypes.data, f32.ctypes.data if want_f32 else None, C.byref(st))
        _check(rc, "dsrt_render_to_host")
        shape = (desc.height, desc.width, 3)
        return rgb.reshape(shape), (f32.reshape(shape) if want_f32 else None), st

    def render_gbuffer(self, desc, ptrs, stream=None, want_stats=False):
        """dsrt_render_gbuffer: the G-buffer of the current camera into DEVICE buffers.  `ptrs` maps channel names (capi.GBUFFER_CHANNELS) to device
        pointers, e.g. torch tensors' data_ptr(); channels not named are not written.  Asynchronous on `stream` unless want_stats."""
        unknown = set(ptrs) - set(capi.GBUFFER_CHANNELS)
        if unknown:
            raise ValueError(f"unknown G-buffer channel(s) {sorted(unknown)}; known: {list(capi.GBUFFER_CHANNELS)}")
        gb = DsrtGBuffer(**{k: C.c_void_p(int(v)) for k, v in ptrs.items() if v})
        st = DsrtStats() if want_stats else None
        _check(lib.dsrt_render_gbuffer(self._h, C.byref(desc), C.byref(gb), C.c_void_p(stream) if stream else None, C.byref(st) if st is not None else None),
               "dsrt_render_gbuffer")
        return st

    def gbuffer_to_host(self, desc, channels=None):
        """dsrt_render_gbuffer_to_host: {channel: numpy array of shape (H, W) or (H, W, C)} for `channels` (default: all of capi.GBUFFER_CHANNELS)."""
        names = list(capi.GBUFFER_CHANNELS) if channels is None else list(channels)
        out = {}
        for n in names:
            dt, comps = capi.GBUFFER_CHANNELS[n]
            out[n] = np.zeros((desc.height, desc.width) + ((comps,) if comps > 1 else ()), dt)
        gb = DsrtGBuffer(**{n: C.c_void_p(a.ctypes.data) for n, a in out.items()})
        _check(lib.dsrt_render_gbuffer_to_host(self._h, C.byref(desc), C.byref(gb), None), "dsrt_render_gbuffer_to_host")
        return out

    def _coverage_struct(self, ptrs, rep):
        unknown = (set(ptrs) - set(capi.COVERAGE_CHANNELS)) | (set(rep or {}) - set(capi.GBUFFER_CHANNELS))
        if unknown:
            raise ValueError(f"unknown coverage channel(s) {sorted(unknown)}; known: {list(capi.COVERAGE_CHANNELS)} and, in rep, {list(capi.GBUFFER_CHANNELS)}")
        cov = capi.DsrtCoverage(**{k: C.c_void_p(int(v)) for k, v in ptrs.items() if v})
        cov.rep = DsrtGBuffer(**{k: C.c_void_p(int(v)) for k, v in (rep or {}).items() if v})
        return cov

    def render_coverage(self, desc, cov_desc=None, ptrs=None, rep=None, classes=None, stream=None, want_stats=False):
        """dsrt_render_coverage: the sub-pixel coverage of the current camera into DEVICE buffers.  `ptrs` maps names of capi.COVERAGE_CHANNELS to device pointers
        (e.g. torch tensors' data_ptr()), `rep` names of capi.GBUFFER_CHANNELS to those of the representative's record; what is not named is not written.
        cov_desc: coverage_desc() (default DIAGONAL 64); classes: coverage_classes([...]), needed for class_hits.  Asynchronous on `stream` unless want_stats."""
        cd = coverage_desc() if cov_desc is None else cov_desc
        cov = self._coverage_struct(ptrs or {}, rep)
        st = DsrtStats() if want_stats else None
        _check(lib.dsrt_render_coverage(self._h, C.byref(desc), C.byref(cd), C.byref(classes) if classes is not None else None, C.byref(cov),
                                        C.c_void_p(stream) if stream else None, C.byref(st) if st is not None else None), "dsrt_render_coverage")
        return st

    def coverage_to_host(self, desc, cov_desc=None, channels=None, rep=(), classes=None):
        """dsrt_render_coverage_to_host: {channel: numpy array (H, W)} for `channels` (default: all of capi.COVERAGE_CHANNELS; class_hits, shape (H, W, count), only
        with `classes`), and under "rep" the dict of the representative's G-buffer channels named in `rep` (True: all of them)."""
        cd = coverage_desc() if cov_desc is None else cov_desc
        names = [n for n in capi.COVERAGE_CHANNELS if n != "class_hits" or classes is not None] if channels is None else list(channels)
        rep_names = list(capi.GBUFFER_CHANNELS) if rep is True else list(rep or ())
        H, W = desc.height, desc.width
        out = {n: np.zeros((H, W) + ((classes.count,) if n == "class_hits" and classes is not None else ()), capi.COVERAGE_CHANNELS[n]) for n in names}
        out_rep = {}
        for n in rep_names:
            dt, comps = capi.GBUFFER_CHANNELS[n]
            out_rep[n] = np.zeros((H, W) + ((comps,) if comps > 1 else ()), dt)
        cov = self._coverage_struct({n: a.ctypes.data for n, a in out.items()}, {n: a.ctypes.data for n, a in out_rep.items()})
        _check(lib.dsrt_render_coverage_to_host(self._h, C.byref(desc), C.byref(cd), C.byref(classes) if classes is not None else None, C.byref(cov), None),
               "dsrt_render_coverage_to_host")
        if rep_names:
            out["rep"] = out_rep
        return out

    def trace_rays(self, origins, dirs, t_min=None, t_max=None, any_hit=False, channels=None, stream=None, want_stats=False):
        """Ray queries on the resident scene (include/dsrt.h, dsrt_trace_rays): {channel: array} for `channels` (capi.RAY_HIT_CHANNELS; default all of
        them, or `flags` alone with any_hit=True), of shape (N,) or (N, comps).  origins / dirs are float32 (N, 3), t_min / t_max float32 (N,) or None, all
        contiguous and all of one kind:
          * torch tensors on this context's device: the device path; outputs are tensors on that device, ordered on `stream` (a torch.cuda.Stream or a raw
            hipStream_t; default: torch's current stream), which first waits for torch's current stream;
          * numpy arrays: dsrt_trace_rays_to_host, numpy outputs.
        With want_stats, returns (outputs, DsrtStats) and the call synchronises."""
        names = (["flags"] if any_hit else list(capi.RAY_HIT_CHANNELS)) if channels is None else list(channels)
        unknown = set(names) - set(capi.RAY_HIT_CHANNELS)
        if unknown:
            raise ValueError(f"unknown ray-hit channel(s) {sorted(unknown)}; known: {list(capi.RAY_HIT_CHANNELS)}")
        inputs = {"origins": origins, "dirs": dirs, "t_min": t_min, "t_max": t_max}
        is_torch = _torch is not None and isinstance(origins, _torch.Tensor)
        n = None
        for key, x in inputs.items():
            if x is None:
                if key in ("origins", "dirs"):
                    raise ValueError(f"trace_rays: {key} is required")
                continue
            want_shape = "(N, 3)" if key in ("origins", "dirs") else "(N,)"
            if is_torch:
                if not isinstance(x, _torch.Tensor):
                    raise TypeError(f"trace_rays: {key} must be a torch tensor like origins, not {type(x).__name__}")
                if x.dtype != _torch.float32:
                    raise TypeError(f"trace_rays: {key} must be float32, not {x.dtype}")
                if x.device.type != "cuda" or x.device.index != self.device:
                    raise ValueError(f"trace_rays: {key} is on {x.device}, the context is on cuda:{self.device}")
                if not x.is_contiguous():
                    raise ValueError(f"trace_rays: {key} must be contiguous")
            else:
                if not isinstance(x, np.ndarray):
                    raise TypeError(f"trace_rays: {key} must be a numpy array or a torch tensor, not {type(x).__name__}")
                if x.dtype != np.float32:
                    raise TypeError(f"trace_rays: {key} must be float32, not {x.dtype}")
                if not x.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"trace_rays: {key} must be C-contiguous")
            shape = tuple(x.shape)
            if (key in ("origins", "dirs") and (len(shape) != 2 or shape[1] != 3)) or (key in ("t_min", "t_max") and len(shape) != 1):
                raise ValueError(f"trace_rays: {key} must have shape {want_shape}, not {shape}")
            if n is None:
                n = shape[0]
            elif shape[0] != n:
                raise ValueError(f"trace_rays: {key} holds {shape[0]} rays, origins {n}")
        mode = capi.TRACE_ANY if any_hit else capi.TRACE_CLOSEST
        st = DsrtStats() if want_stats else None
        if is_torch:
            torch_dt = {"<f4": _torch.float32, "<i4": _torch.int32, "u1": _torch.uint8}
            out = {}
            for k in names:
                dt, comps = capi.RAY_HIT_CHANNELS[k]
                out[k] = _torch.empty((n, comps) if comps > 1 else (n,), dtype=torch_dt[dt], device=origins.device)
            cur = _torch.cuda.current_stream(origins.device)
            ts = stream if isinstance(stream, _torch.cuda.Stream) else None
            raw = ts.cuda_stream if ts is not None else (int(stream) if stream else cur.cuda_stream)
            if raw != cur.cuda_stream:
                if ts is not None:
                    ts.wait_stream(cur)                                     # inputs written and outputs allocated on the current stream come first
                    for x in list(inputs.values()) + list(out.values()):
                        if x is not None:
                            x.record_stream(ts)
                else:
                    cur.synchronize()
            if n:
                rays = DsrtRays(**{k: C.c_void_p(x.data_ptr()) for k, x in inputs.items() if x is not None})
                hits = DsrtRayHits(**{k: C.c_void_p(x.data_ptr()) for k, x in out.items()})
                _check(lib.dsrt_trace_rays(self._h, int(n), C.byref(rays), mode, C.byref(hits), C.c_void_p(raw),
                                           C.byref(st) if st is not None else None), "dsrt_trace_rays")
        else:
            out = {}
            for k in names:
                dt, comps = capi.RAY_HIT_CHANNELS[k]
                out[k] = np.empty((n, comps) if comps > 1 else (n,), dt)
            if n:
                rays = DsrtRays(**{k: C.c_void_p(x.ctypes.data) for k, x in inputs.items() if x is not None})
                hits = DsrtRayHits(**{k: C.c_void_p(x.ctypes.data) for k, x in out.items()})
                _check(lib.dsrt_trace_rays_to_host(self._h, int(n), C.byref(rays), mode, C.byref(hits), C.byref(st) if st is not None else None),
                       "dsrt_trace_rays_to_host")
        return (out, st) if want_stats else out

    # ---- sample sets (include/dsrt.h, dsrt_render_accumulate): rng_mode 1 sums in caller-owned int64 device tensors ----
    def _device_tensor(self, x, dtype, numel, what, required=True):
        """`x`, if it is a contiguous torch tensor of `dtype` on this context's device with `numel` elements -- numel: (the count, the message's words for it) --
        or None for an optional one that is not given."""
        if x is None:
            if required:
                raise ValueError(f"{what} is required")
            return None
        if _torch is None or not isinstance(x, _torch.Tensor):
            raise TypeError(f"{what} must be a torch tensor")
        if x.dtype != dtype:
            raise TypeError(f"{what} must be {'int64' if dtype == _torch.int64 else dtype}, not {x.dtype}")
        if x.device.type != "cuda" or x.device.index != self.device:
            raise ValueError(f"{what} is on {x.device}, the context is on cuda:{self.device}")
        if not x.is_contiguous() or x.numel() != numel[0]:
            raise ValueError(f"{what} must be contiguous with {numel[1]} elements")
        return x

    def _accum(self, desc, sums, sum_sq, sq_required=True):
        """DsrtAccum of `sums` and `sum_sq`, int64 device tensors of width*height*3 elements (sum_sq may be None unless sq_required)."""
        n = desc.width * desc.height * 3
        numel = (n, f"width*height*3 = {n}")
        return DsrtAccum(_tensor_ptr(self._device_tensor(sums, _torch.int64, numel, "sums")),
                         _tensor_ptr(self._device_tensor(sum_sq, _torch.int64, numel, "sum_sq", sq_required)))

    def _pixel_tensor(self, desc, x, dtype, what, required=True):
        n = desc.width * desc.height
        return self._device_tensor(x, dtype, (n, f"width*height = {n}"), what, required)

    def _raw_stream(self, stream):
        if isinstance(stream, _torch.cuda.Stream):
            return stream.cuda_stream
        return int(stream) if stream else _torch.cuda.current_stream(self.device).cuda_stream

    def render_accumulate(self, desc, first, count, stride=1, sums=None, sum_sq=None, stream=None, want_stats=False):
        """dsrt_render_accumulate: ADD the sums of samples {first + j*stride : 0 <= j < count} of every pixel (a frame planned at desc.spp, rng_mode 1)
        to `sums` (and the squared samples to `sum_sq`, if given): int64 device tensors of width*height*3 elements, zeroed by the caller once.  On
        `stream` (a torch.cuda.Stream or a raw hipStream_t; default: torch's current stream); with want_stats the call synchronises and returns DsrtStats."""
        acc = self._accum(desc, sums, sum_sq, sq_required=False)
        st = DsrtStats() if want_stats else None
        _check(lib.dsrt_render_accumulate(self._h, C.byref(desc), int(first), int(count), int(stride), C.byref(acc), C.c_void_p(self._raw_stream(stream)),
                                          C.byref(st) if st is not None else None), "dsrt_render_accumulate")
        return st

    def resolve_accumulated(self, desc, sums, samples_done, sum_sq=None, want_rgb8=True, want_f32=False, want_var=False, stream=None):
        """dsrt_resolve_accumulated: the image of `sums` after `samples_done` samples per pixel.  Returns (rgb8, f32, var) as device tensors of shape
        (height, width, 3) -- uint8, float32, float32 (the variance of the mean; needs sum_sq) -- None for what was not asked for."""
        acc = self._accum(desc, sums, sum_sq, sq_required=want_var)
        out = _outputs(desc, dict(rgb8=want_rgb8, f32=want_f32, var=want_var), sums.device)
        _check(lib.dsrt_resolve_accumulated(self._h, C.byref(desc), C.byref(acc), int(samples_done), *map(_tensor_ptr, out), C.c_void_p(self._raw_stream(stream))),
               "dsrt_resolve_accumulated")
        return out

    # ---- adaptive sampling (include/dsrt.h, ADAPTIVE SAMPLING): masked sample sets, the convergence test, the per-pixel resolve, the driver ----
    def render_accumulate_masked(self, desc, first, count, stride=1, sums=None, sum_sq=None, mask=None, n=None, stream=None, want_stats=False):
        """dsrt_render_accumulate_masked: render_accumulate for the pixels whose byte of `mask` (uint8 device tensor, width*height, image order) is nonzero;
        `n` (optional int32 device tensor, width*height: the pixels' sample counts) gets `count` added where the mask is set."""
        acc = self._accum(desc, sums, sum_sq, sq_required=False)
        mask = self._pixel_tensor(desc, mask, _torch.uint8, "mask")
        n = self._pixel_tensor(desc, n, _torch.int32, "n", required=False)
        st = DsrtStats() if want_stats else None
        _check(lib.dsrt_render_accumulate_masked(self._h, C.byref(desc), int(first), int(count), int(stride), C.byref(acc), _tensor_ptr(mask), _tensor_ptr(n),
                                                 C.c_void_p(self._raw_stream(stream)), C.byref(st) if st is not None else None), "dsrt_render_accumulate_masked")
        return st

    def select_unconverged(self, desc, sums, sum_sq, n, rel_tol, floor=0.0, n_min=0, n_max=0xFFFFFFFF, mask=None, want_active=True, stream=None):
        """dsrt_select_unconverged: (mask, active) -- the uint8 device tensor (height, width) of the pixels that still need samples (written into `mask` if one is
        given) and how many they are (None without want_active: then the call does not synchronise)."""
        acc = self._accum(desc, sums, sum_sq)
        n = self._pixel_tensor(desc, n, _torch.int32, "n")
        mask = _torch.empty((desc.height, desc.width), dtype=_torch.uint8, device=sums.device) if mask is None else self._pixel_tensor(desc, mask, _torch.uint8, "mask")
        active = C.c_uint32(0)
        _check(lib.dsrt_select_unconverged(self._h, C.byref(desc), C.byref(acc), _tensor_ptr(n), float(rel_tol), float(floor), int(n_min), int(n_max),
                                           _tensor_ptr(mask), C.byref(active) if want_active else None, C.c_void_p(self._raw_stream(stream))),
               "dsrt_select_unconverged")
        return mask, (active.value if want_active else None)

    def resolve_accumulated_counts(self, desc, sums, n, sum_sq=None, want_rgb8=True, want_f32=False, want_var=False, stream=None):
        """dsrt_resolve_accumulated_counts: resolve_accumulated with every pixel's own sample count `n` (int32 device tensor) in place of samples_done."""
        acc = self._accum(desc, sums, sum_sq, sq_required=want_var)
        n = self._pixel_tensor(desc, n, _torch.int32, "n")
        out = _outputs(desc, dict(rgb8=want_rgb8, f32=want_f32, var=want_var), sums.device)
        _check(lib.dsrt_resolve_accumulated_counts(self._h, C.byref(desc), C.byref(acc), _tensor_ptr(n), *map(_tensor_ptr, out), C.c_void_p(self._raw_stream(stream))),
               "dsrt_resolve_accumulated_counts")
        return out

    def render_adaptive(self, desc, rel_tol, passes=8, min_passes=2, floor=0.0, want_rgb8=True, want_f32=False, want_var=False, stream=None):
        """dsrt_render_adaptive: the frame in up to `passes` interleaved passes, each pass from min_passes on over the pixels that have not converged to rel_tol.
        Returns (acc, (rgb8, f32, var), stats): the Accumulator holding the sums and the per-pixel counts `acc.n`, the images asked for, and a dict with
        passes_run, samples_total and active (pixels rendered by each pass that ran)."""
        acc = Accumulator(self, desc, moments=True, counts=True)
        out = _outputs(desc, dict(rgb8=want_rgb8, f32=want_f32, var=want_var), acc.sum.device)
        a = DsrtAccum(_tensor_ptr(acc.sum), _tensor_ptr(acc.sum_sq))
        ad = capi.DsrtAdaptive(int(passes), int(min_passes), float(rel_tol), float(floor))
        st = capi.DsrtAdaptiveStats()
        _check(lib.dsrt_render_adaptive(self._h, C.byref(desc), C.byref(ad), C.byref(a), _tensor_ptr(acc.n), *map(_tensor_ptr, out), C.c_void_p(self._raw_stream(stream)),
                                        C.byref(st)), "dsrt_render_adaptive")
        acc.samples_done = None                    # the counts are per pixel now: acc.resolve_counts(), not acc.resolve()
        return acc, out, {"passes_run": st.passes_run, "samples_total": st.samples_total, "active": list(st.active[:st.passes_run])}

    # ---- the denoiser (include/dsrt.h, DENOISER): the variance-guided a-trous filter over sums and G-buffer guides; with a `temporal` part, TEMPORAL ACCUMULATION:
    # the same with reprojected frame history in front of its iterations ----
    def _guide_tensors(self, desc, guides):
        if set(guides) != set(DENOISE_GUIDES):
            raise ValueError(f"guides must hold exactly {list(DENOISE_GUIDES)}, not {sorted(guides)}")
        out = {}
        for k in DENOISE_GUIDES:
            x, comps = guides[k], capi.GBUFFER_CHANNELS[k][1]
            if _torch is None or not isinstance(x, _torch.Tensor) or x.dtype != _torch.float32:
                raise TypeError(f"guide {k} must be a float32 torch tensor")
            out[k] = self._device_tensor(x, _torch.float32, (desc.width * desc.height * comps, f"width*height*{comps}"), f"guide {k}")
        return out

    def _denoise(self, on_device, desc, sums, sum_sq, guides, samples_done, n, params, wants, stream=None, temporal=None, motion=None, shading=None, coverage=None):
        """Every denoise_* method: from torch device tensors (on_device) or from numpy arrays into numpy arrays (the _to_host entry points); the outputs `wants` names.
        coverage = (alpha or None, alpha_min): denoise_accumulated_coverage.  temporal = (prev_camera, history_prev, history_next, DsrtTemporal or None):
        denoise_temporal; the host form makes the next history itself and returns it last.  motion = (first_tri, num_tris, poses_prev, poses_cur, prim_id):
        denoise_temporal_bodies.  shading = (flags, edge_guard): denoise_temporal_shaded, with or without a motion."""
        H, W = desc.height, desc.width
        ptr = _tensor_ptr if on_device else _array_ptr
        name = ("dsrt_denoise_accumulated_coverage" if coverage is not None else "dsrt_denoise_accumulated" if temporal is None else
                "dsrt_denoise_temporal_shaded" if shading is not None else "dsrt_denoise_temporal_bodies" if motion is not None else "dsrt_denoise_temporal")

        def pixels(x, dt, what, required=True):                                           # a width*height channel of the form's kind
            if on_device:
                return self._pixel_tensor(desc, x, getattr(_torch, np.dtype(dt).name), what, required)
            return None if x is None and not required else np.ascontiguousarray(x, dt).reshape(H, W)

        # the inputs
        if on_device:
            acc = self._accum(desc, sums, sum_sq)
            n = pixels(n, np.int32, "n", required=False)
            if n is None and samples_done is None:
                raise ValueError(f"{name[5:]} needs samples_done or per-pixel counts n")
            g = self._guide_tensors(desc, guides)
        else:
            S, S2 = (np.ascontiguousarray(x, np.uint64).reshape(H, W, 3) for x in (sums, sum_sq))
            acc = DsrtAccum(_array_ptr(S), _array_ptr(S2))
            n = pixels(n, np.uint32, "n", required=False)
            if set(guides) != set(DENOISE_GUIDES):
                raise ValueError(f"guides must hold exactly {list(DENOISE_GUIDES)}, not {sorted(guides)}")
            g = {k: np.ascontiguousarray(guides[k], np.float32).reshape((H, W) + ((3,) if capi.GBUFFER_CHANNELS[k][1] == 3 else ())) for k in DENOISE_GUIDES}
        gd = capi.DsrtDenoiseGuides(**{k: ptr(x) for k, x in g.items()})
        if temporal is not None:
            prev_camera, history_prev, history_next, tp = temporal
            hist = H * W * capi.HISTORY_FLOATS
            if on_device:
                for what, h in (("history_prev", history_prev), ("history_next", history_next)):
                    if h is None:
                        continue
                    if not isinstance(h, _torch.Tensor) or h.dtype != _torch.float32 or h.device.type != "cuda" or h.device.index != self.device:
                        raise TypeError(f"{what} must be a float32 torch tensor on cuda:{self.device}")
                    self._device_tensor(h, _torch.float32, (hist, f"width*height*{capi.HISTORY_FLOATS}"), what)
            else:                                                                         # (a host history is 16-byte aligned: copies that are)
                if history_prev is not None:
                    src, history_prev = history_prev, aligned_zeros(hist)
                    history_prev[:] = np.asarray(src, np.float32).reshape(-1)
                history_next = aligned_zeros(hist)
            tp = temporal_defaults() if tp is None else tp
        params = denoise_defaults() if params is None else params
        out = _outputs(desc, wants, sums.device if on_device else None)
        head = (self._h, C.byref(desc), C.byref(acc), int(samples_done or 0), ptr(n), C.byref(gd))
        tail = (C.byref(params), *map(ptr, out)) + ((C.c_void_p(self._raw_stream(stream)),) if on_device else ())

        # the entry point's own arguments, between the two
        mid, m, keep = (), None, None
        if coverage is not None:
            alpha = pixels(coverage[0], np.float32, "alpha", required=False)
            mid = (ptr(alpha), C.c_float(coverage[1]))
        elif temporal is not None:
            if motion is not None:
                prim = pixels(motion[4], np.int32, "prim_id")
                m, keep = _body_motion(*motion[:4], ptr(prim))
            if shading is not None:
                flags = pixels(shading[0], np.uint8, "flags")
                sh = temporal_shading(ptr(flags), shading[1])
                mid = (C.byref(m) if m is not None else None, C.byref(sh))
            elif motion is not None:
                mid = (C.byref(m),)
            mid += (C.byref(prev_camera) if prev_camera is not None else None, ptr(history_prev), ptr(history_next), C.byref(tp))
        if not on_device:
            name += "_to_host"
        _check(getattr(lib, name)(*head, *mid, *tail), name)
        del keep
        return tuple(out) if on_device or temporal is None else (*out, history_next.reshape(H, W, capi.HISTORY_FLOATS))

    def denoise_accumulated(self, desc, sums, sum_sq, guides, samples_done=None, n=None, params=None, want_rgb8=True, want_f32=False, want_linear=True,
                            want_var=False, stream=None):
        """dsrt_denoise_accumulated: the filtered image of `sums` / `sum_sq` (int64 device tensors, as render_accumulate's) after `samples_done` samples per pixel
        or the per-pixel counts `n` (int32 device tensor), guided by `guides` = {"normal", "position", "albedo", "range": float32 device tensors, G-buffer
        channels}.  params: a DsrtDenoise (denoise_defaults()).  Returns (rgb8, f32, linear, var) device tensors of shape (height, width, 3), None where not asked for."""
        return self._denoise(True, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var), stream)

    def denoise_accumulated_to_host(self, desc, sums, sum_sq, guides, samples_done=None, n=None, params=None, want_rgb8=True, want_f32=False, want_linear=True,
                                    want_var=False):
        """dsrt_denoise_accumulated_to_host: the same from numpy arrays (uint64 sums (H, W, 3), uint32 counts (H, W), float32 guides) into numpy arrays."""
        return self._denoise(False, desc, sums, sum_sq, guides, samples_done, n, params, dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var))

    def denoise_accumulated_coverage(self, desc, sums, sum_sq, guides, alpha, alpha_min=None, samples_done=None, n=None, params=None, want_rgb8=True, want_f32=False,
                                     want_linear=True, want_var=False, stream=None):
        """dsrt_denoise_accumulated_coverage: denoise_accumulated with COVERAGE DEMODULATION -- `alpha` a float32 device tensor of width*height elements (the alpha of a
        DIAGONAL render_coverage; None = the plain denoiser), `guides` usually that pass's rep channels.  alpha_min: default coverage_alpha_min()."""
        alpha_min = coverage_alpha_min() if alpha_min is None else alpha_min
        return self._denoise(True, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var), stream, coverage=(alpha, alpha_min))

    def denoise_accumulated_coverage_to_host(self, desc, sums, sum_sq, guides, alpha, alpha_min=None, samples_done=None, n=None, params=None, want_rgb8=True,
                                             want_f32=False, want_linear=True, want_var=False):
        """dsrt_denoise_accumulated_coverage_to_host: the same from numpy arrays into numpy arrays."""
        alpha_min = coverage_alpha_min() if alpha_min is None else alpha_min
        return self._denoise(False, desc, sums, sum_sq, guides, samples_done, n, params, dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var),
                             coverage=(alpha, alpha_min))

    def render_denoised_coverage_to_host(self, desc, cov_desc=None, alpha_min=None, params=None, want_f32=False, want_linear=True, want_var=False, want_alpha=False):
        """dsrt_render_denoised_coverage_to_host: desc.spp samples, a DIAGONAL coverage pass and the coverage-aware filter: (rgb8, f32, linear, var, alpha, DsrtStats)."""
        params = denoise_defaults() if params is None else params
        alpha_min = coverage_alpha_min() if alpha_min is None else alpha_min
        out = _outputs(desc, dict(rgb8=True, f32=want_f32, linear=want_linear, var=want_var))
        alpha = np.zeros((desc.height, desc.width), np.float32) if want_alpha else None
        st = DsrtStats()
        _check(lib.dsrt_render_denoised_coverage_to_host(self._h, C.byref(desc), C.byref(cov_desc) if cov_desc is not None else None, C.c_float(alpha_min), C.byref(params),
                                                         *map(_array_ptr, out), _array_ptr(alpha), C.byref(st)), "dsrt_render_denoised_coverage_to_host")
        return (*out, alpha, st)

    def render_denoised_to_host(self, desc, params=None, want_f32=False, want_linear=True, want_var=False):
        """dsrt_render_denoised_to_host: desc.spp samples, the G-buffer of the current camera and the filter, into numpy arrays: (rgb8, f32, linear, var, DsrtStats)."""
        params = denoise_defaults() if params is None else params
        out = _outputs(desc, dict(rgb8=True, f32=want_f32, linear=want_linear, var=want_var))
        st = DsrtStats()
        _check(lib.dsrt_render_denoised_to_host(self._h, C.byref(desc), C.byref(params), *map(_array_ptr, out), C.byref(st)), "dsrt_render_denoised_to_host")
        return (*out, st)

    def denoise_temporal(self, desc, sums, sum_sq, guides, history_next, prev_camera=None, history_prev=None, samples_done=None, n=None, temporal=None, params=None,
                         want_rgb8=True, want_f32=False, want_linear=True, want_var=False, want_prev_xy=False, want_weight=False, stream=None):
        """dsrt_denoise_temporal: denoise_accumulated with the history stage.  history_prev / history_next: float32 device tensors of width*height*16 elements
        (the caller ping-pongs two); prev_camera: the GPUCamera history_prev was written under -- both None for the first frame of a sequence.  temporal: a
        DsrtTemporal (temporal_defaults()).  Returns (rgb8, f32, linear, var, prev_xy, weight) device tensors -- prev_xy (height, width, 2), weight (height, width) --
        None where not asked for."""
        return self._denoise(True, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, prev_xy=want_prev_xy, weight=want_weight), stream,
                             temporal=(prev_camera, history_prev, history_next, temporal))

    def denoise_temporal_to_host(self, desc, sums, sum_sq, guides, prev_camera=None, history_prev=None, samples_done=None, n=None, temporal=None, params=None,
                                 want_rgb8=True, want_f32=False, want_linear=True, want_var=False, want_prev_xy=True, want_weight=True):
        """dsrt_denoise_temporal_to_host: the same from numpy arrays into numpy arrays.  history_prev: float32 (H, W, 16) or None.  Returns
        (rgb8, f32, linear, var, prev_xy, weight, history_next) -- history_next (H, W, 16), 64-byte aligned."""
        return self._denoise(False, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, prev_xy=want_prev_xy, weight=want_weight),
                             temporal=(prev_camera, history_prev, None, temporal))

    def denoise_temporal_bodies(self, desc, sums, sum_sq, guides, motion, history_next, prev_camera=None, history_prev=None, samples_done=None, n=None, temporal=None,
                                params=None, want_rgb8=True, want_f32=False, want_linear=True, want_var=False, want_prev_xy=False, want_weight=False,
                                want_prev_position=False, stream=None):
        """dsrt_denoise_temporal_bodies: denoise_temporal with the motion stage (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES).  motion = (first_tri, num_tris,
        poses_prev, poses_cur, prim_id): the bodies' triangle ranges, the poses of the frame history_prev was written under and of this one ((bodies, 12) each), and
        the current G-buffer's prim_id (int32 device tensor).  Returns denoise_temporal's tuple and prev_position (height, width, 3) after it."""
        return self._denoise(True, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, prev_xy=want_prev_xy, weight=want_weight,
                                  prev_position=want_prev_position), stream, temporal=(prev_camera, history_prev, history_next, temporal), motion=motion)

    def denoise_temporal_bodies_to_host(self, desc, sums, sum_sq, guides, motion, prev_camera=None, history_prev=None, samples_done=None, n=None, temporal=None,
                                        params=None, want_rgb8=True, want_f32=False, want_linear=True, want_var=False, want_prev_xy=True, want_weight=True,
                                        want_prev_position=True):
        """dsrt_denoise_temporal_bodies_to_host: the same from numpy arrays into numpy arrays (prim_id int32 (H, W)).  Returns
        (rgb8, f32, linear, var, prev_xy, weight, prev_position, history_next)."""
        return self._denoise(False, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, prev_xy=want_prev_xy, weight=want_weight,
                                  prev_position=want_prev_position), temporal=(prev_camera, history_prev, None, temporal), motion=motion)

    def set_temporal_bodies(self, on=True):
        """dsrt_ctx_set_temporal_bodies: render_denoised_temporal_to_host follows the resident scene's bodies -- a pose update no longer ends the sequence; the
        motion stage runs with the poses of this frame and of the context's last one.  Off by default."""
        _check(lib.dsrt_ctx_set_temporal_bodies(self._h, 1 if on else 0), "dsrt_ctx_set_temporal_bodies")
        return self

    @property
    def temporal_bodies(self):
        return bool(lib.dsrt_ctx_temporal_bodies(self._h))

    def denoise_temporal_shaded(self, desc, sums, sum_sq, guides, flags, history_next, motion=None, edge_guard=1, prev_camera=None, history_prev=None, samples_done=None,
                                n=None, temporal=None, params=None, want_rgb8=True, want_f32=False, want_linear=True, want_var=False, want_prev_xy=False,
                                want_weight=False, want_prev_position=False, want_status=False, stream=None):
        """dsrt_denoise_temporal_shaded: denoise_temporal_bodies with the sun state (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING).  flags: the current
        G-buffer's flags channel (uint8 device tensor); motion as denoise_temporal_bodies', or None for a static scene (then no prev_position); edge_guard 0 or 1.
        Returns denoise_temporal_bodies' tuple and status (height, width) uint8 after it."""
        return self._denoise(True, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, prev_xy=want_prev_xy, weight=want_weight,
                                  prev_position=want_prev_position, status=want_status), stream, temporal=(prev_camera, history_prev, history_next, temporal),
                             motion=motion, shading=(flags, edge_guard))

    def denoise_temporal_shaded_to_host(self, desc, sums, sum_sq, guides, flags, motion=None, edge_guard=1, prev_camera=None, history_prev=None, samples_done=None, n=None,
                                        temporal=None, params=None, want_rgb8=True, want_f32=False, want_linear=True, want_var=False, want_prev_xy=True, want_weight=True,
                                        want_prev_position=None, want_status=True):
        """dsrt_denoise_temporal_shaded_to_host: the same from numpy arrays into numpy arrays (flags uint8 (H, W)).  Returns
        (rgb8, f32, linear, var, prev_xy, weight, prev_position, status, history_next); prev_position is asked for by default where there is a motion."""
        want_prev_position = motion is not None if want_prev_position is None else want_prev_position
        return self._denoise(False, desc, sums, sum_sq, guides, samples_done, n, params,
                             dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, prev_xy=want_prev_xy, weight=want_weight,
                                  prev_position=want_prev_position, status=want_status), temporal=(prev_camera, history_prev, None, temporal), motion=motion,
                             shading=(flags, edge_guard))

    def set_temporal_shading(self, mode=2):
        """dsrt_ctx_set_temporal_shading: render_denoised_temporal_to_host keeps the sun state in its history -- 0 off (the default), 1 the tap test only, 2 with the
        edge guards."""
        _check(lib.dsrt_ctx_set_temporal_shading(self._h, int(mode)), "dsrt_ctx_set_temporal_shading")
        return self

    @property
    def temporal_shading(self):
        return int(lib.dsrt_ctx_temporal_shading(self._h))

    def render_denoised_temporal_to_host(self, desc, params=None, temporal=None, reset=False, want_f32=False, want_linear=True, want_var=False, want_prev_xy=False):
        """dsrt_render_denoised_temporal_to_host: render_denoised_to_host with the history the CONTEXT keeps from call to call (reset=True starts a new sequence;
        change desc.seed from frame to frame).  Returns (rgb8, f32, linear, var, prev_xy, DsrtStats)."""
        params = denoise_defaults() if params is None else params
        temporal = temporal_defaults() if temporal is None else temporal
        out = _outputs(desc, dict(rgb8=True, f32=want_f32, linear=want_linear, var=want_var, prev_xy=want_prev_xy))
        st = DsrtStats()
        _check(lib.dsrt_render_denoised_temporal_to_host(self._h, C.byref(desc), C.byref(params), C.byref(temporal), 1 if reset else 0, *map(_array_ptr, out), C.byref(st)),
               "dsrt_render_denoised_temporal_to_host")
        return (*out, st)

    # ---- the upscaler (include/dsrt.h, UPSCALER): a low-resolution linear image to the output resolution, guided by the G-buffers of both rasters ----
    def _upscale_guides(self, guides, width, height, what, on_device):
        """DsrtUpscaleGuides of {"normal", "position", "albedo", "range"[, "flags"]} at width x height, and the arrays that keep its pointers alive."""
        if not set(DENOISE_GUIDES) <= set(guides) <= set(UPSCALE_GUIDES):
            raise ValueError(f"{what} guides must hold {list(DENOISE_GUIDES)} and optionally 'flags', not {sorted(guides)}")
        keep = {}
        for k in UPSCALE_GUIDES:
            x = guides.get(k)
            if x is None:
                continue
            dt, comps = capi.GBUFFER_CHANNELS[k]
            n = width * height * comps
            if on_device:
                keep[k] = self._device_tensor(x, getattr(_torch, np.dtype(dt).name), (n, f"{what} width*height*{comps} = {n}"), f"{what} guide {k}")
            else:
                keep[k] = np.ascontiguousarray(x, dt).reshape(n)
        ptr = _tensor_ptr if on_device else _array_ptr
        return capi.DsrtUpscaleGuides(**{k: ptr(x) for k, x in keep.items()}), keep

    def upscale_guided(self, desc, lo_width, lo_height, lo_linear, lo_guides, hi_guides, lo_var=None, params=None, want_rgb8=True, want_f32=False, want_linear=True,
                       want_var=False, want_support=False, stream=None):
        """dsrt_upscale_guided (torch device tensors) or dsrt_upscale_guided_to_host (numpy arrays, chosen by lo_linear's type): the lo_width x lo_height linear image
        `lo_linear` (float32, lo_height*lo_width*3; `lo_var` its variance, needed for want_var) at desc.width x desc.height.  lo_guides / hi_guides: the G-buffer
        channels {"normal", "position", "albedo", "range"} and optionally "flags" (uint8) of the two rasters, same camera.  params: a DsrtUpscale (upscale_defaults()).
        Returns (rgb8, f32, linear, var, support) of shape (height, width[, 3]), None where not asked for."""
        on_device = _torch is not None and isinstance(lo_linear, _torch.Tensor)
        w, h = int(lo_width), int(lo_height)
        n = w * h * 3
        if on_device:
            numel = (n, f"lo_width*lo_height*3 = {n}")
            lin = self._device_tensor(lo_linear, _torch.float32, numel, "lo_linear")
            var = self._device_tensor(lo_var, _torch.float32, numel, "lo_var", required=False)
        else:
            lin = np.ascontiguousarray(lo_linear, np.float32).reshape(n)
            var = np.ascontiguousarray(lo_var, np.float32).reshape(n) if lo_var is not None else None
        lo, keep_lo = self._upscale_guides(lo_guides, w, h, "low-resolution", on_device)
        hi, keep_hi = self._upscale_guides(hi_guides, desc.width, desc.height, "output", on_device)
        params = upscale_defaults() if params is None else params
        out = _outputs(desc, dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, support=want_support), lin.device if on_device else None)
        ptr = _tensor_ptr if on_device else _array_ptr
        head = (self._h, C.byref(desc), w, h, ptr(lin), ptr(var), C.byref(lo), C.byref(hi), C.byref(params), *map(ptr, out))
        if on_device:
            _check(lib.dsrt_upscale_guided(*head, C.c_void_p(self._raw_stream(stream))), "dsrt_upscale_guided")
        else:
            _check(lib.dsrt_upscale_guided_to_host(*head), "dsrt_upscale_guided_to_host")
        del keep_lo, keep_hi
        return out

    def render_upscaled_to_host(self, lo_desc, out_width, out_height, denoise=None, params=None, want_f32=False, want_linear=True, want_var=False, want_lo_rgb8=False):
        """dsrt_render_upscaled_to_host: lo_desc.spp samples at lo_desc's size, the denoiser (`denoise`: a DsrtDenoise, None = the plain mean), the G-buffers of both
        rasters and the upscaler, into numpy arrays of out_height x out_width: (rgb8, f32, linear, var, lo_rgb8, DsrtStats); lo_rgb8 is the low-resolution image."""
        params = upscale_defaults() if params is None else params
        hi = DsrtRenderDesc.from_buffer_copy(lo_desc)
        hi.width, hi.height = int(out_width), int(out_height)
        out = _outputs(hi, dict(rgb8=True, f32=want_f32, linear=want_linear, var=want_var))
        lo_rgb8 = np.zeros((lo_desc.height, lo_desc.width, 3), np.uint8) if want_lo_rgb8 else None
        st = DsrtStats()
        _check(lib.dsrt_render_upscaled_to_host(self._h, C.byref(lo_desc), hi.width, hi.height, C.byref(denoise) if denoise is not None else None, C.byref(params),
                                                *map(_array_ptr, out), _array_ptr(lo_rgb8), C.byref(st)), "dsrt_render_upscaled_to_host")
        return (*out, lo_rgb8, st)

    # ---- the upscaler with coverage (include/dsrt.h, COVERAGE-AWARE UPSCALER): the same, with the alphas of a DIAGONAL coverage pass at each raster ----
    def upscale_guided_coverage(self, desc, lo_width, lo_height, lo_linear, lo_guides, hi_guides, lo_alpha, hi_alpha, alpha_min=None, lo_var=None, params=None,
                                want_rgb8=True, want_f32=False, want_linear=True, want_var=False, want_support=False, want_level=False, stream=None):
        """dsrt_upscale_guided_coverage (torch device tensors) or dsrt_upscale_guided_coverage_to_host (numpy arrays, chosen by lo_linear's type): upscale_guided with
        `lo_alpha` (float32, lo_height*lo_width) and `hi_alpha` (float32, height*width), the alphas of a DIAGONAL render_coverage at each raster (both None = the plain
        upscaler); lo_guides / hi_guides usually those passes' rep channels.  alpha_min: default upscale_coverage_alpha_min().
        Returns (rgb8, f32, linear, var, support, level) of shape (height, width[, 3]), None where not asked for; level is uint8, 0 .. 3."""
        on_device = _torch is not None and isinstance(lo_linear, _torch.Tensor)
        w, h = int(lo_width), int(lo_height)
        n = w * h * 3
        alpha_min = upscale_coverage_alpha_min() if alpha_min is None else alpha_min
        if on_device:
            numel = (n, f"lo_width*lo_height*3 = {n}")
            lin = self._device_tensor(lo_linear, _torch.float32, numel, "lo_linear")
            var = self._device_tensor(lo_var, _torch.float32, numel, "lo_var", required=False)
            a_lo = self._device_tensor(lo_alpha, _torch.float32, (w * h, f"lo_width*lo_height = {w * h}"), "lo_alpha", required=False)
            a_hi = self._device_tensor(hi_alpha, _torch.float32, (desc.width * desc.height, f"width*height = {desc.width * desc.height}"), "hi_alpha", required=False)
        else:
            lin = np.ascontiguousarray(lo_linear, np.float32).reshape(n)
            var = np.ascontiguousarray(lo_var, np.float32).reshape(n) if lo_var is not None else None
            a_lo = np.ascontiguousarray(lo_alpha, np.float32).reshape(w * h) if lo_alpha is not None else None
            a_hi = np.ascontiguousarray(hi_alpha, np.float32).reshape(desc.width * desc.height) if hi_alpha is not None else None
        lo, keep_lo = self._upscale_guides(lo_guides, w, h, "low-resolution", on_device)
        hi, keep_hi = self._upscale_guides(hi_guides, desc.width, desc.height, "output", on_device)
        params = upscale_defaults() if params is None else params
        out = _outputs(desc, dict(rgb8=want_rgb8, f32=want_f32, linear=want_linear, var=want_var, support=want_support, level=want_level), lin.device if on_device else None)
        ptr = _tensor_ptr if on_device else _array_ptr
        head = (self._h, C.byref(desc), w, h, ptr(lin), ptr(var), C.byref(lo), C.byref(hi), ptr(a_lo), ptr(a_hi), C.c_float(alpha_min), C.byref(params), *map(ptr, out))
        if on_device:
            _check(lib.dsrt_upscale_guided_coverage(*head, C.c_void_p(self._raw_stream(stream))), "dsrt_upscale_guided_coverage")
        else:
            _check(lib.dsrt_upscale_guided_coverage_to_host(*head), "dsrt_upscale_guided_coverage_to_host")
        del keep_lo, keep_hi
        return out

    def upscale_guided_coverage_to_host(self, desc, lo_width, lo_height, lo_linear, lo_guides, hi_guides, lo_alpha, hi_alpha, **kw):
        """dsrt_upscale_guided_coverage_to_host: upscale_guided_coverage from numpy arrays into numpy arrays (device tensors are copied to the host first)."""
        host = lambda x: x.cpu().numpy() if _torch is not None and isinstance(x, _torch.Tensor) else x           # noqa: E731
        kw = {k: host(x) if k == "lo_var" else x for k, x in kw.items()}
        return self.upscale_guided_coverage(desc, lo_width, lo_height, np.asarray(host(lo_linear)), {k: host(x) for k, x in lo_guides.items()},
                                            {k: host(x) for k, x in hi_guides.items()}, host(lo_alpha), host(hi_alpha), **kw)

    def render_upscaled_coverage_to_host(self, lo_desc, out_width, out_height, cov_lo=None, cov_hi=None, alpha_min=None, denoise=None, params=None, want_f32=False,
                                         want_linear=True, want_var=False, want_lo_rgb8=False, want_alpha=False):
        """dsrt_render_upscaled_coverage_to_host: lo_desc.spp samples at lo_desc's size, a DIAGONAL coverage pass there (cov_lo: a coverage_desc(), None = the
        default), the coverage-aware denoiser (`denoise`: a DsrtDenoise, None = the plain mean), a DIAGONAL coverage pass at the output size (cov_hi) and the
        coverage-aware upscaler, into numpy arrays of out_height x out_width: (rgb8, f32, linear, var, lo_rgb8, alpha_hi, DsrtStats)."""
        params = upscale_defaults() if params is None else params
        alpha_min = upscale_coverage_alpha_min() if alpha_min is None else alpha_min
        hi = DsrtRenderDesc.from_buffer_copy(lo_desc)
        hi.width, hi.height = int(out_width), int(out_height)
        out = _outputs(hi, dict(rgb8=True, f32=want_f32, linear=want_linear, var=want_var))
        lo_rgb8 = np.zeros((lo_desc.height, lo_desc.width, 3), np.uint8) if want_lo_rgb8 else None
        alpha = np.zeros((hi.height, hi.width), np.float32) if want_alpha else None
        st = DsrtStats()
        ref = lambda x: C.byref(x) if x is not None else None                        # noqa: E731
        _check(lib.dsrt_render_upscaled_coverage_to_host(self._h, C.byref(lo_desc), hi.width, hi.height, ref(cov_lo), ref(cov_hi), C.c_float(alpha_min), ref(denoise),
                                                         C.byref(params), *map(_array_ptr, out), _array_ptr(lo_rgb8), _array_ptr(alpha), C.byref(st)),
               "dsrt_render_upscaled_coverage_to_host")
        return (*out, lo_rgb8, alpha, st)

    # ---- the detector model (include/dsrt.h, SENSOR MODEL): a linear frame as raw DN ----
    def sensor_apply(self, desc, linear, params=None, want_dn=True, want_signal=False, want_rgb8=False, stream=None):
        """dsrt_sensor_apply (a torch device tensor) or dsrt_sensor_apply_to_host (a numpy array, chosen by linear's type): the linear frame `linear` (float32,
        desc.height*desc.width*3: the denoiser's or the upscaler's) through the detector `params` (a DsrtSensor: sensor_defaults()).  Returns (dn, signal, rgb8): uint16
        and float32 of shape (height, width, 3), or (height, width) with params.mono, and uint8 (height, width, 3); None where not asked for."""
        params = sensor_defaults() if params is None else params
        on_device = _torch is not None and isinstance(linear, _torch.Tensor)
        n = desc.width * desc.height * 3
        if on_device:
            lin = self._device_tensor(linear, _torch.float32, (n, f"width*height*3 = {n}"), "linear")
        else:
            lin = np.ascontiguousarray(linear, np.float32).reshape(n)
        planes = (desc.height, desc.width) if params.mono else (desc.height, desc.width, 3)
        shapes = ((want_dn, planes, np.uint16), (want_signal, planes, np.float32), (want_rgb8, (desc.height, desc.width, 3), np.uint8))
        if on_device:
            out = tuple(_torch.empty(shape, dtype=getattr(_torch, np.dtype(dt).name), device=lin.device) if want else None for want, shape, dt in shapes)
        else:
            out = tuple(np.zeros(shape, dt) if want else None for want, shape, dt in shapes)
        ptr = _tensor_ptr if on_device else _array_ptr
        head = (self._h, C.byref(desc), ptr(lin), C.byref(params), *map(ptr, out))
        if on_device:
            _check(lib.dsrt_sensor_apply(*head, C.c_void_p(self._raw_stream(stream))), "dsrt_sensor_apply")
        else:
            _check(lib.dsrt_sensor_apply_to_host(*head), "dsrt_sensor_apply_to_host")
        return out

    # ---- the star field (include/dsrt.h, POINT SOURCES): occluded point sources in the linear frame ----
    def render_stars(self, desc, dirs, flux, linear=None, occlusion=True, want=("layer", "xy", "status"), stream=None, want_stats=False):
        """dsrt_render_stars (torch device tensors) or dsrt_render_stars_to_host (numpy arrays, chosen by dirs' type): the stars `dirs` (float32 (N, 3), model frame,
        towards the star) of flux `flux` (float32 (N, 3)) through the context's camera and resident scene.  linear: the frame (float32, height*width*3) that
        "linear_out" adds the layer to.  want: names of capi.STAR_OUTPUTS.  Returns {name: array}: layer and linear_out (height, width, 3) float32, xy (N, 2) float32,
        status (N,) uint8.  With want_stats, returns (outputs, DsrtStats) and the call synchronises."""
        names = list(want)
        unknown = set(names) - set(capi.STAR_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown star output(s) {sorted(unknown)}; known: {list(capi.STAR_OUTPUTS)}")
        on_device = _torch is not None and isinstance(dirs, _torch.Tensor)
        n = int(dirs.shape[0])
        px3 = desc.width * desc.height * 3
        if on_device:
            d = self._device_tensor(dirs, _torch.float32, (n * 3, f"N*3 = {n * 3}"), "dirs")
            f = self._device_tensor(flux, _torch.float32, (n * 3, f"N*3 = {n * 3}"), "flux")
            lin = self._device_tensor(linear, _torch.float32, (px3, f"width*height*3 = {px3}"), "linear", required=False)
        else:
            d, f = (np.ascontiguousarray(x, np.float32).reshape(n * 3) for x in (dirs, flux))
            lin = None if linear is None else np.ascontiguousarray(linear, np.float32).reshape(px3)
        out = {}
        for k in names:
            dt, per, comps = capi.STAR_OUTPUTS[k]
            shape = (desc.height, desc.width, comps) if per == "pixel" else ((n, comps) if comps > 1 else (n,))
            out[k] = _torch.empty(shape, dtype=getattr(_torch, np.dtype(dt).name), device=d.device) if on_device else np.zeros(shape, dt)
        st = DsrtStats() if want_stats else None
        if n == 0 and not any(capi.STAR_OUTPUTS[k][1] == "pixel" for k in names):      # per-star outputs of no stars: nothing to launch
            return (out, st) if want_stats else out
        ptr = _tensor_ptr if on_device else _array_ptr
        stars = capi.DsrtStars(n, 1 if occlusion else 0, ptr(d) if n else None, ptr(f) if n else None, ptr(lin))
        sout = capi.DsrtStarsOut(**{k: ptr(x) for k, x in out.items()})
        head = (self._h, C.byref(desc), C.byref(stars), C.byref(sout))
        if on_device:
            _check(lib.dsrt_render_stars(*head, C.c_void_p(self._raw_stream(stream)), C.byref(st) if st is not None else None), "dsrt_render_stars")
        else:
            _check(lib.dsrt_render_stars_to_host(*head, C.byref(st) if st is not None else None), "dsrt_render_stars_to_host")
        return (out, st) if want_stats else out

    # ---- the lens model (include/dsrt.h, LENS MODEL): distortion and vignetting on the linear frame, and on its labels ----
    def lens_apply(self, desc, src, params, want=("image", "src_xy", "status"), stream=None):
        """dsrt_lens_apply (a torch device tensor) or dsrt_lens_apply_to_host (a numpy array, chosen by src's type): the pinhole frame `src` -- params.src_height *
        params.src_width * params.channels 32-bit elements: float32 for filters 1 and 2; float32, int32 or uint32 for nearest, which copies words -- through the lens
        `params` (a DsrtLens: lens_defaults(...)) into the frame of desc.width x desc.height.  want: names among image, src_xy, status.  Returns {name: array}: image
        (height, width, channels) of src's dtype -- (height, width) for one channel -- src_xy (height, width, 2) float32, status (height, width) uint8."""
        names = list(want)
        unknown = set(names) - {"image", "src_xy", "status"}
        if unknown:
            raise ValueError(f"unknown lens output(s) {sorted(unknown)}; known: image, src_xy, status")
        on_device = _torch is not None and isinstance(src, _torch.Tensor)
        ch = int(params.channels)
        n = params.src_width * params.src_height * ch
        words = ("float32",) if params.filter != capi.LENS_NEAREST else ("float32", "int32", "uint32")
        if on_device:
            kinds = [getattr(_torch, w) for w in words if hasattr(_torch, w)]
            if src.dtype not in kinds:
                raise TypeError(f"src must be one of {words} for filter {params.filter}, not {src.dtype}")
            s = self._device_tensor(src, src.dtype, (n, f"src_width*src_height*channels = {n}"), "src")
        else:
            s = np.ascontiguousarray(src)
            if s.dtype.name not in words:
                raise TypeError(f"src must be one of {words} for filter {params.filter}, not {s.dtype}")
            if s.size != n:
                raise ValueError(f"src has {s.size} elements, not src_width*src_height*channels = {n}")
        H, W = desc.height, desc.width
        shapes = {"image": ((H, W, ch) if ch > 1 else (H, W), None), "src_xy": ((H, W, 2), "float32"), "status": ((H, W), "uint8")}
        out = {}
        for k in names:
            shape, dt = shapes[k]
            if on_device:
                out[k] = _torch.empty(shape, dtype=s.dtype if dt is None else getattr(_torch, dt), device=s.device)
            else:
                out[k] = np.zeros(shape, s.dtype if dt is None else dt)
        ptr = _tensor_ptr if on_device else _array_ptr
        lout = capi.DsrtLensOut(**{k: ptr(x) for k, x in out.items()})
        head = (self._h, C.byref(desc), ptr(s), C.byref(params), C.byref(lout))
        if on_device:
            _check(lib.dsrt_lens_apply(*head, C.c_void_p(self._raw_stream(stream))), "dsrt_lens_apply")
        else:
            _check(lib.dsrt_lens_apply_to_host(*head), "dsrt_lens_apply_to_host")
        return out

    def poke_node_word(self, word_index, value):
        """Test hook (dsrt_selftest_poke_node_word): overwrite one 32-bit word of the resident node records; returns the previous value."""
        old = C.c_uint32()
        _check(lib.dsrt_selftest_poke_node_word(self._h, int(word_index), int(value) & 0xFFFFFFFF, C.byref(old)), "dsrt_selftest_poke_node_word")
        return old.value

    SCHEDULE_ARRAYS = ("tile_cost", "tile_order", "tile_work", "batch_table", "pixel_list")

    def read_schedule(self, array, first_word, n_words):
        """Test hook (dsrt_selftest_read_schedule): n_words 32-bit words of a working buffer of the scheduling pre-pass as the context's last launch left it;
        `array` a name of SCHEDULE_ARRAYS or its number.  include/dsrt.h says what is valid when."""
        which = self.SCHEDULE_ARRAYS.index(array) if isinstance(array, str) else int(array)
        out = np.zeros(int(n_words), np.uint32)
        _check(lib.dsrt_selftest_read_schedule(self._h, which, int(first_word), int(n_words), out.ctypes.data), "dsrt_selftest_read_schedule")
        return out

    def selftest_tile_order(self, cost, tile, items_per_pixel, resident_lanes, spp):
        """dsrt_selftest_tile_order: dsrt_tile_order_kernel on the cost words given -> (order, sched[5]); order entries the kernel did not write are 0xFFFFFFFF."""
        cost = np.ascontiguousarray(cost, np.uint32)
        order, sched = np.zeros(cost.size, np.uint32), np.zeros(5, np.uint32)
        _check(lib.dsrt_selftest_tile_order(self._h, cost.ctypes.data if cost.size else None, int(cost.size), int(tile), int(items_per_pixel), int(resident_lanes), int(spp),
                                            order.ctypes.data if cost.size else None, sched.ctypes.data), "dsrt_selftest_tile_order")
        return order, sched

    def selftest_tile_reorder(self, work, order, sched):
        """dsrt_selftest_tile_reorder: dsrt_tile_reorder_kernel on (work, order, sched[5]) -> the order it leaves."""
        work, out, sched = np.ascontiguousarray(work, np.uint32), np.array(order, np.uint32), np.ascontiguousarray(sched, np.uint32)
        _check(lib.dsrt_selftest_tile_reorder(self._h, work.ctypes.data if work.size else None, int(work.size), out.ctypes.data if out.size else None, int(out.size),
                                              sched.ctypes.data), "dsrt_selftest_tile_reorder")
        return out

    def selftest_batch_table(self, sched, tt, rng_mode, spp, light_chunk_len, order_base):
        """dsrt_selftest_batch_table: dsrt_batch_table_kernel on `sched` (frames x >= 5 words) and the frames' order_base -> (table words (2 * frames, 24), total)."""
        sched = np.ascontiguousarray(sched, np.uint32)
        frames, stride = sched.shape
        base = np.ascontiguousarray(order_base, np.uint32)
        table, total = np.zeros((2 * frames, 24), np.uint32), np.zeros(1, np.uint32)
        _check(lib.dsrt_selftest_batch_table(self._h, sched.ctypes.data, stride, frames, int(tt), int(rng_mode), int(spp), int(light_chunk_len), base.ctypes.data,
                                             table.ctypes.data, total.ctypes.data), "dsrt_selftest_batch_table")
        return table, int(total[0])

    def selftest_philox(self, seed, subsequence, n):
        ours, theirs = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _check(lib.dsrt_selftest_philox(self._h, int(seed), int(subsequence), int(n), ours.ctypes.data, theirs.ctypes.data), "dsrt_selftest_philox")
        return ours, theirs

    def selftest_devkat(self, fn, in12):
        """dsrt_selftest_devkat: the kernel's material / frame helpers on n x 12 input words -> n x 12 output words (float32 arrays)."""
        a = np.ascontiguousarray(in12, np.float32).reshape(-1, 12)
        out = np.zeros_like(a)
        _check(lib.dsrt_selftest_devkat(self._h, int(fn), a.ctypes.data, out.ctypes.data, int(a.shape[0])), "dsrt_selftest_devkat")
        return out

    def selftest_math(self, fn, x, y=0.0):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        _check(lib.dsrt_selftest_math(self._h, int(fn), x.ctypes.data, float(y), out.ctypes.data, int(x.size)), "dsrt_selftest_math")
        return out


class Accumulator:
    """The sums of one rng_mode 1 frame (include/dsrt.h, SAMPLE SETS) and how many samples per pixel they hold.  Render sets into it with any context on
    the same device (`ctx` defaults to the one given here), resolve it whenever, and add another accumulator's sums to it with `+=` (sample sharding:
    contexts, streams or -- after a copy or an all-reduce of the int64 tensors -- devices that rendered disjoint sets of the same frame).

        acc = Accumulator(ctx, desc, moments=True)
        for p in range(4):                       # four interleaved passes: a preview after each
            acc.render(p, count, stride=4)       # count = len(range(p, desc.spp, 4))
            rgb, _, var = acc.resolve(want_var=True)
    """

    def __init__(self, ctx, desc, moments=False, counts=False):
        if desc.rng_mode != 1:
            raise ValueError("sample sets are rng_mode 1's")
        self.ctx, self.desc = ctx, desc
        n = desc.width * desc.height * 3
        self.sum = _torch.zeros(n, dtype=_torch.int64, device=f"cuda:{ctx.device}")
        self.sum_sq = _torch.zeros(n, dtype=_torch.int64, device=f"cuda:{ctx.device}") if moments else None
        # per-pixel sample counts (adaptive sampling: masked sets give pixels different counts), int32 (height, width); None = every pixel has samples_done
        self.n = _torch.zeros((desc.height, desc.width), dtype=_torch.int32, device=f"cuda:{ctx.device}") if counts else None
        self.samples_done = 0

    @staticmethod
    def pass_count(spp, first, stride):
        """Samples in the set {first, first + stride, ...} below spp."""
        return len(range(first, spp, stride))

    def render(self, first, count=None, stride=1, ctx=None, stream=None, want_stats=False, mask=None):
        """Add the set {first + j*stride : 0 <= j < count} (count: all of them below spp by default) and count its samples.  With `mask` (uint8 device
        tensor, nonzero = active) only for the active pixels: the accumulator then keeps per-pixel counts (`n`) and is resolved with resolve_counts()."""
        count = self.pass_count(self.desc.spp, first, stride) if count is None else count
        if mask is None:
            st = (ctx or self.ctx).render_accumulate(self.desc, first, count, stride, self.sum, self.sum_sq, stream=stream, want_stats=want_stats)
            if self.n is not None:                  # behind the launch, on its stream (torch's current one unless another was given)
                if not stream:
                    self.n += count
                else:
                    with _torch.cuda.stream(stream if isinstance(stream, _torch.cuda.Stream) else _torch.cuda.ExternalStream(int(stream))):
                        self.n += count
            if self.samples_done is not None:
                self.samples_done += count
            return st
        if self.n is None:                          # the first masked set: until now every pixel had samples_done samples
            self.n = _torch.full((self.desc.height, self.desc.width), self.samples_done, dtype=_torch.int32, device=self.sum.device)
        self.samples_done = None
        return (ctx or self.ctx).render_accumulate_masked(self.desc, first, count, stride, self.sum, self.sum_sq, mask, self.n, stream=stream, want_stats=want_stats)

    def __iadd__(self, other):
        d, o = self.desc, other.desc
        if (d.width, d.height, d.spp, d.seed) != (o.width, o.height, o.spp, o.seed):
            raise ValueError("accumulators of different frames (width, height, spp or seed differ)")
        if self.sum_sq is not None and other.sum_sq is None:
            raise ValueError("this accumulator sums squared samples and the other does not")
        if self.n is not None or other.n is not None or self.samples_done is None or other.samples_done is None:
            raise ValueError("accumulators with per-pixel counts are not added (add their sum and n tensors)")
        self.sum += other.sum.to(self.sum.device)
        if self.sum_sq is not None:
            self.sum_sq += other.sum_sq.to(self.sum_sq.device)
        self.samples_done += other.samples_done
        return self

    def resolve(self, want_rgb8=True, want_f32=False, want_var=False, stream=None):
        """(rgb8, f32, var) device tensors of the current sums (Context.resolve_accumulated)."""
        if self.samples_done is None:
            raise ValueError("this accumulator holds masked sets (per-pixel counts): resolve_counts()")
        return self.ctx.resolve_accumulated(self.desc, self.sum, self.samples_done, self.sum_sq if want_var else None, want_rgb8, want_f32, want_var, stream)

    def resolve_counts(self, want_rgb8=True, want_f32=False, want_var=False, stream=None):
        """(rgb8, f32, var) of the current sums with every pixel's own count `n` (Context.resolve_accumulated_counts)."""
        if self.n is None:
            raise ValueError("this accumulator has no per-pixel counts (counts=True, or a masked render)")
        return self.ctx.resolve_accumulated_counts(self.desc, self.sum, self.n, self.sum_sq if want_var else None, want_rgb8, want_f32, want_var, stream)

    def _empty_guides(self):
        """Uninitialised guide tensors of this frame: {"normal", "position", "albedo", "range"}, float32, (H, W, 3) or (H, W)."""
        H, W = self.desc.height, self.desc.width
        return {k: _torch.empty((H, W, 3) if capi.GBUFFER_CHANNELS[k][1] == 3 else (H, W), dtype=_torch.float32, device=self.sum.device) for k in DENOISE_GUIDES}

    def guides(self, ctx=None, stream=None):
        """The denoiser's guides of the context's current camera: {"normal", "position", "albedo", "range"} float32 device tensors (Context.render_gbuffer)."""
        ctx = ctx or self.ctx
        g = self._empty_guides()
        ctx.render_gbuffer(self.desc, {k: x.data_ptr() for k, x in g.items()}, stream=ctx._raw_stream(stream))
        return g

    def coverage(self, cov_desc=None, ctx=None, stream=None):
        """(alpha, guides) of a coverage pass over the context's current camera (Context.render_coverage; default DIAGONAL 64): alpha a float32 device tensor
        (H, W), guides the representative's {"normal", "position", "albedo", "range"} -- what denoise(alpha=..., guides=...) takes."""
        ctx = ctx or self.ctx
        g = self._empty_guides()
        alpha = _torch.empty((self.desc.height, self.desc.width), dtype=_torch.float32, device=self.sum.device)
        ctx.render_coverage(self.desc, cov_desc, {"alpha": alpha.data_ptr()}, {k: x.data_ptr() for k, x in g.items()}, stream=ctx._raw_stream(stream))
        return alpha, g

    def denoise(self, params=None, guides=None, want_rgb8=True, want_f32=False, want_linear=True, want_var=False, stream=None, alpha=None, alpha_min=None):
        """(rgb8, f32, linear, var) of the current sums through the variance-guided filter (Context.denoise_accumulated); needs moments=True.  Without
        `guides` the G-buffer of the context's current camera is rendered first.  alpha (a float32 device tensor, or True = a DIAGONAL 64 coverage pass of the
        current camera, whose representatives then are the guides unless `guides` is given) / alpha_min: the coverage-aware filter (Context.denoise_accumulated_coverage)."""
        if self.sum_sq is None:
            raise ValueError("the denoiser is guided by the variance: Accumulator(..., moments=True)")
        if alpha is not None:
            if alpha is True:
                alpha, rep_guides = self.coverage(stream=stream)
                guides = rep_guides if guides is None else guides
            guides = self.guides(stream=stream) if guides is None else guides
            return self.ctx.denoise_accumulated_coverage(self.desc, self.sum, self.sum_sq, guides, alpha, alpha_min, samples_done=self.samples_done,
                                                         n=self.n if self.samples_done is None else None, params=params, want_rgb8=want_rgb8, want_f32=want_f32,
                                                         want_linear=want_linear, want_var=want_var, stream=stream)
        guides = self.guides(stream=stream) if guides is None else guides
        return self.ctx.denoise_accumulated(self.desc, self.sum, self.sum_sq, guides, samples_done=self.samples_done, n=self.n if self.samples_done is None else None,
                                            params=params, want_rgb8=want_rgb8, want_f32=want_f32, want_linear=want_linear, want_var=want_var, stream=stream)


class TemporalDenoiser:
    """A sequence of frames through Context.denoise_temporal: owns the two history tensors and the previous frame's camera.

        td = TemporalDenoiser(ctx, desc)
        for f, (cam, sun) in enumerate(views):
            ctx.set_camera_sun(cam, sun)
            d = make_desc(W, H, spp, seed=seed0 + f, rng_mode=1)           # a different seed per frame: the blend takes the frames as independent
            acc = Accumulator(ctx, d, moments=True); acc.render(0)
            rgb, _, linear, var, prev_xy, weight = td.step(acc, cam, want_prev_xy=True)
    """

    def __init__(self, ctx, desc, temporal=None, params=None):
        self.ctx, self.width, self.height = ctx, desc.width, desc.height
        self.temporal = temporal_defaults() if temporal is None else temporal
        self.params = denoise_defaults() if params is None else params
        n = desc.width * desc.height * capi.HISTORY_FLOATS
        self.history = [_torch.zeros(n, dtype=_torch.float32, device=f"cuda:{ctx.device}") for _ in range(2)]
        self.current = 0                    # history[current] holds the last frame's records once prev_camera is set
        self.prev_camera = None

    def reset(self):
        """Start a new sequence: the next step has no history."""
        self.prev_camera = None

    def step(self, accumulator, camera, guides=None, params=None, temporal=None, stream=None, **wants):
        """One frame: `accumulator` holds its sums (moments=True), `camera` is the GPUCamera it was rendered with (the context's current one: without `guides`
        the G-buffer is rendered here).  Returns Context.denoise_temporal's tuple; `wants`: its want_* flags."""
        d = accumulator.desc
        if (d.width, d.height) != (self.width, self.height):
            raise ValueError("the accumulator's frame has another size than this sequence")
        if accumulator.sum_sq is None:
            raise ValueError("the denoiser is guided by the variance: Accumulator(..., moments=True)")
        guides = accumulator.guides(stream=stream) if guides is None else guides
        first = self.prev_camera is None
        nxt = self.current if first else self.current ^ 1
        out = self.ctx.denoise_temporal(d, accumulator.sum, accumulator.sum_sq, guides, self.history[nxt], None if first else self.prev_camera,
                                        None if first else self.history[self.current], samples_done=accumulator.samples_done,
                                        n=accumulator.n if accumulator.samples_done is None else None, temporal=temporal or self.temporal, params=params or self.params,
                                        stream=stream, **wants)
        self.current = nxt
        self.prev_camera = GPUCamera.from_buffer_copy(camera)
        return out


class Multi:
    """All GPUs of a node from one process (DsrtMulti): a frame, or every frame of a sequence, sharded by interleaved screen tiles; one RCCL gather
    per frame (render_frame) or per batch launch (render_sequence)."""

    def __init__(self, devices, frames_in_flight=1):
        devs = (C.c_int * len(devices))(*[int(x) for x in devices])
        h = C.c_void_p()
        _check(lib.dsrt_multi_create(devs, len(devices), int(frames_in_flight), C.byref(h)), "dsrt_multi_create")
        self._h, self.n = h, len(devices)

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.dsrt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def uses_rccl(self):
        return bool(lib.dsrt_multi_uses_rccl(self._h))

    def upload(self, scene_host_view):
        _check(lib.dsrt_multi_scene_upload(self._h, C.byref(scene_host_view)), "dsrt_multi_scene_upload")

    def render_frame(self, desc, camera, sun_dir):
        """-> (rgb8 image H x W x 3, per-rank kernel ms, wall seconds)"""
        img = np.zeros((desc.height, desc.width, 3), np.uint8)
        ms = (C.c_float * self.n)()
        sec = C.c_double()
        _check(lib.dsrt_multi_render_frame(self._h, C.byref(desc), C.byref(camera), _f3(sun_dir), img.ctypes.data, ms, C.byref(sec)), "dsrt_multi_render_frame")
        return img, list(ms), sec.value

    def render_sequence(self, desc, cameras, sun_dirs, want_images=True):
        """Every rank renders its tiles of every frame as sharded batch launches (dsrt_multi_render_sequence).  -> (list of images or None, wall seconds)"""
        n = len(cameras)
        cams = (GPUCamera * n)(*cameras)
        suns = (C.c_float * (3 * n))(*[float(v) for s3 in sun_dirs for v in s3])
        imgs = [np.zeros((desc.height, desc.width, 3), np.uint8) for _ in range(n)] if want_images else None
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs]) if want_images else None
        sec = C.c_double()
        _check(lib.dsrt_multi_render_sequence(self._h, C.byref(desc), cams, suns, n, ptrs, C.byref(sec)), "dsrt_multi_render_sequence")
        return imgs, sec.value
