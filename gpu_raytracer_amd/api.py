"""ctypes binding of librt_hip.so (the C ABI in include/rt_hip.h).

This is the stub a host-language binding would look like (see INTEGRATION.md for the
Rust `extern "C"` version).  There is no fallback: if the library is missing, or no HIP
device is present, the calls raise.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_HIP_LIB", os.path.join(_HERE, "librt_hip.so"))  # RT_HIP_LIB: development override (kernel variants)

RT_OK = 0
ERRORS = {-1: "RT_ERR_BAD_ARG", -2: "RT_ERR_OOM", -3: "RT_ERR_HIP", -4: "RT_ERR_NOT_UPLOADED", -5: "RT_ERR_INTERNAL"}
MODE_LEGACY, MODE_WAVEFRONT, MODE_EXTENDED = 0, 1, 2
FLAG_COUNTERS = 1
FLAG_NO_SHADOWS = 2
FLAG_KERNEL_V1 = 4
FLAG_KERNEL_SM = 8
FLAG_NO_SHADOW_GRID = 16
FLAG_KERNEL_PIPELINE = 32
FLAG_NO_BEAMS = 64
FLAG_STAGE_TIMES = 128
FLAG_ACCUMULATE = 256  # RT_FLAG_ACCUMULATE: add this call's samples to the context's running image (extended mode)
FLAG_ACCUMULATE_RESTART = 512  # RT_FLAG_ACCUMULATE_RESTART: ... starting a new one at sample 0
ACCUMULATE_MAX_SAMPLES = 1 << 24  # RT_ACCUMULATE_MAX_SAMPLES
PREPARE_SHADOW_GRIDS = 1
PREPARE_QUALITY_TREE = 2
QUERY_COUNTERS = 1  # RT_QUERY_COUNTERS of rt_intersect / rt_occluded
QUERY_CHUNK = 4194304  # RT_QUERY_CHUNK: host batches are staged in chunks of at most this many rays
QUERY_COUNT_ALL = 2  # RT_QUERY_COUNT_ALL of rt_intersect_all / rt_closest_point_all / rt_overlap_box / rt_overlap_obb / rt_overlap_triangle / rt_contact_capsule: counts are all candidates in the range, not the records written
MULTI_HIT_MAX = 16  # RT_MULTI_HIT_MAX: the most hits rt_intersect_all lists per ray
NEAREST_MAX = 16  # RT_NEAREST_MAX: the most primitives rt_closest_point_all lists per point
OVERLAP_MAX = 32  # RT_OVERLAP_MAX: the most primitives rt_overlap_box / rt_overlap_obb / rt_overlap_triangle list per query
SWEEP_AXIS_SPHERE = 13  # RT_SWEEP_AXIS_SPHERE of rt_box_sweep_hit.axis: the contact is with a sphere primitive
SWEEP_AXIS_NONE = 0xFFFFFFFF  # RT_SWEEP_AXIS_NONE: a miss, or in contact at the start
SWEEP_TRIANGLE_AXIS_SPHERE = 26  # RT_SWEEP_TRIANGLE_AXIS_SPHERE of rt_triangle_sweep_hit.axis: the contact is with a sphere primitive
OVERLAP_ANY = 4  # RT_OVERLAP_ANY of rt_overlap_box / rt_overlap_obb / rt_overlap_triangle: counts are 1 where anything touches the box, else 0, and the walk stops at the first
POSED_MESH_MAX = 65536  # RT_POSED_MESH_MAX: the most triangles of a query mesh of rt_overlap_mesh / rt_sweep_mesh
CONTACT_MAX = 16  # RT_CONTACT_MAX: the most primitives rt_contact_capsule lists per capsule
CONTACT_ANY = 4  # RT_CONTACT_ANY of rt_contact_capsule: counts are 1 where anything is in range of the capsule, else 0, and the walk stops at the first
INSIDE_MAX_RAYS = 7  # RT_INSIDE_MAX_RAYS: the most parity rays rt_inside / rt_signed_distance trace per point
INSIDE_DIRECTIONS = np.array([  # RT_INSIDE_DIRECTIONS: direction k of vote k, used as given
    [0.5377, 0.7431, 0.3982], [-0.6241, 0.3517, 0.6977], [0.2893, -0.4719, 0.8328],
    [-0.3361, -0.8154, -0.4703], [0.8467, -0.2249, -0.4821], [-0.1873, 0.5566, -0.8094],
    [0.4129, 0.1683, -0.8951]], np.float32)
AO_MAX_SAMPLES = 4096  # RT_AO_MAX_SAMPLES: the most samples rt_ambient_occlusion takes per point
DIRECT_AMBIENT, DIRECT_NO_SHADOWS, DIRECT_NO_SHADOW_GRID = 4, 8, 16  # RT_DIRECT_* of rt_direct_light_params.flags
DIRECT_MAX_LIGHTS = 32  # RT_DIRECT_MAX_LIGHTS: rt_direct_light's lit_mask has one bit per light
PATH_NO_SHADOWS, PATH_CAMERA_DRAWS = 32, 64  # RT_PATH_* of rt_path_params.flags
PATH_MAX_SAMPLES = 4096  # RT_PATH_MAX_SAMPLES: the most paths rt_radiance traces per ray, rt_radiance_sh per probe
MAX_BOUNCES = T.MAX_BOUNCES  # RT_MAX_BOUNCES
UPDATE_REBUILD = 1  # RT_UPDATE_REBUILD of rt_update_geometry
AOV_SAMPLES_PER_LAUNCH = T.AOV_SAMPLES_PER_LAUNCH  # RT_AOV_SAMPLES_PER_LAUNCH: rt_aovs traces at most this many samples per kernel
DENOISE_DEMODULATE = T.DENOISE_DEMODULATE  # RT_DENOISE_DEMODULATE of rt_denoise_params.flags
DENOISE_MAX_ITERATIONS = T.DENOISE_MAX_ITERATIONS
DENOISE_DEFAULTS = dict(iterations=T.DENOISE_DEFAULT_ITERATIONS, sigma_color=T.DENOISE_DEFAULT_SIGMA_COLOR, sigma_normal=T.DENOISE_DEFAULT_SIGMA_NORMAL,
                        sigma_depth=T.DENOISE_DEFAULT_SIGMA_DEPTH, sigma_albedo=T.DENOISE_DEFAULT_SIGMA_ALBEDO)  # RT_DENOISE_DEFAULT_*
STAT_MEGAKERNEL_FALLBACK, STAT_SINGLE_PASS, STAT_REFIT, STAT_REBUILT = 1, 2, 4, 8  # RT_STAT_* (rt_stats.flags)
PRIM_MISS = 0xFFFFFFFF
PRIM_SPHERE_FLAG = 0x80000000
EXTENDED_AVAILABLE = True

# every symbol include/rt_hip.h declares
ABI_SYMBOLS = [
    "rt_create", "rt_upload_scene", "rt_upload_scene_packed", "rt_upload_textures", "rt_prepare", "rt_render", "rt_dispatch_tile",
    "rt_read_rgb32f", "rt_read_rgba8_channels", "rt_read_rgba8_combined", "rt_read_hits",
    "rt_get_stats", "rt_last_error", "rt_destroy", "rt_version",
    "rt_intersect", "rt_occluded", "rt_camera_rays", "rt_intersect_all",
    "rt_surface", "rt_ambient_occlusion", "rt_direct_light", "rt_radiance", "rt_radiance_sh", "rt_irradiance", "rt_closest_point", "rt_closest_point_all", "rt_sweep_sphere", "rt_sweep_box", "rt_sweep_capsule",
    "rt_inside", "rt_signed_distance", "rt_overlap_box", "rt_contact_capsule", "rt_overlap_obb", "rt_sweep_obb", "rt_overlap_triangle", "rt_sweep_triangle", "rt_contact_triangle",
    "rt_overlap_mesh", "rt_sweep_mesh",
    "rt_update_geometry",
    "rt_accumulated_samples",
    "rt_aovs", "rt_sample_rays", "rt_denoise",
    "rt_render_adaptive", "rt_read_adaptive",
]


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


_lib = None


def load():
    """Load librt_hip.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m gpu_raytracer_amd.build` "
                              "(there is no CPU fallback for the hot path)")
        lib = C.CDLL(LIB_PATH)
        lib.rt_last_error.restype = C.c_char_p
        lib.rt_last_error.argtypes = [C.c_void_p]
        lib.rt_version.restype = C.c_char_p
        lib.rt_destroy.restype = None
        lib.rt_destroy.argtypes = [C.c_void_p]
        for name in ABI_SYMBOLS:
            if "RT_HIP_LIB" in os.environ and not hasattr(lib, name):
                continue  # an older build under A/B (development only): entry points added since are simply absent
            fn = getattr(lib, name)
            if name not in ("rt_last_error", "rt_version", "rt_destroy"):
                fn.restype = C.c_int
        _lib = lib
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p(0)


# -- ray batches (rt_intersect / rt_occluded / rt_intersect_all / rt_surface / rt_radiance / rt_camera_rays) ---------------------------------------------------------
# A batch is a C-contiguous float32 array of shape (N, 8), one rt_ray per row: ox oy oz tmin dx dy dz tmax; numpy, or a torch
# tensor on the CPU or on a device of the context.  torch is imported only when a tensor is handed in.

def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _check_batch(a, name, cols, dtype_name):
    """Raises before any library call when `a` is not a C-contiguous (N, cols) array of dtype_name ("float32" or "bool")."""
    if _is_torch(a):
        import torch
        want = {"float32": torch.float32, "bool": torch.bool}[dtype_name]
        if a.dtype != want:
            raise TypeError(f"{name}: dtype {a.dtype}, expected torch.{dtype_name}")
        shape, contiguous = tuple(a.shape), a.is_contiguous()
    elif isinstance(a, np.ndarray):
        if a.dtype != np.dtype(dtype_name):
            raise TypeError(f"{name}: dtype {a.dtype}, expected {dtype_name}")
        shape, contiguous = a.shape, a.flags.c_contiguous
    else:
        raise TypeError(f"{name}: a numpy array or a torch tensor, not {type(a).__name__}")
    if (cols and (len(shape) != 2 or shape[1] != cols)) or (not cols and len(shape) != 1):
        raise ValueError(f"{name}: shape {shape}, expected {'(N, %d)' % cols if cols else '(N,)'}")
    if not contiguous:
        raise ValueError(f"{name}: not C-contiguous")
    return shape[0]


def _contiguous(a):
    return a.is_contiguous() if _is_torch(a) else a.flags.c_contiguous


def _check_kind_dtype(a, name, dtype_name):
    if _is_torch(a):
        import torch
        if a.dtype != getattr(torch, dtype_name):
            raise TypeError(f"{name}: dtype {a.dtype}, expected torch.{dtype_name}")
    elif not isinstance(a, np.ndarray):
        raise TypeError(f"{name}: a numpy array or a torch tensor, not {type(a).__name__}")
    elif a.dtype != np.dtype(dtype_name):
        raise TypeError(f"{name}: dtype {a.dtype}, expected {dtype_name}")


def _check_hit_lists(a, n, max_hits):
    """Raises unless `a` is a C-contiguous float32 (n, max_hits, 4) array: rt_intersect_all's records, ray-major."""
    _check_kind_dtype(a, "out", "float32")
    if len(a.shape) != 3 or tuple(a.shape[1:]) != (max_hits, 4):
        raise ValueError(f"out: shape {tuple(a.shape)}, expected (N, {max_hits}, 4)")
    if not _contiguous(a):
        raise ValueError("out: not C-contiguous")
    if a.shape[0] != n:
        raise ValueError(f"out: {a.shape[0]} rows for {n} rays")


def _check_nearest_lists(a, n, max_nearest):
    """Raises unless `a` is a C-contiguous float32 (n, max_nearest, 8) array: rt_closest_point_all's records, query-major."""
    _check_kind_dtype(a, "out", "float32")
    if len(a.shape) != 3 or tuple(a.shape[1:]) != (max_nearest, 8):
        raise ValueError(f"out: shape {tuple(a.shape)}, expected (N, {max_nearest}, 8)")
    if not _contiguous(a):
        raise ValueError("out: not C-contiguous")
    if a.shape[0] != n:
        raise ValueError(f"out: {a.shape[0]} rows for {n} points")


def _check_contact_lists(a, n, max_contacts, what="capsules"):
    """Raises unless `a` is a C-contiguous float32 (n, max_contacts, 8) array: rt_contact_capsule's or rt_contact_triangle's records, query-major."""
    _check_kind_dtype(a, "out", "float32")
    if len(a.shape) != 3 or tuple(a.shape[1:]) != (max_contacts, 8):
        raise ValueError(f"out: shape {tuple(a.shape)}, expected (N, {max_contacts}, 8)")
    if not _contiguous(a):
        raise ValueError("out: not C-contiguous")
    if a.shape[0] != n:
        raise ValueError(f"out: {a.shape[0]} rows for {n} {what}")


def _check_prim_lists(a, n, max_prims, what="boxes"):
    """Raises unless `a` is a C-contiguous (n, max_prims) array of ids (rt_overlap_box's, query-major): uint32 for numpy, int32 for torch."""
    _check_kind_dtype(a, "out", "int32" if _is_torch(a) else "uint32")
    if len(a.shape) != 2 or a.shape[1] != max_prims:
        raise ValueError(f"out: shape {tuple(a.shape)}, expected (N, {max_prims})")
    if not _contiguous(a):
        raise ValueError("out: not C-contiguous")
    if a.shape[0] != n:
        raise ValueError(f"out: {a.shape[0]} rows for {n} {what}")


def _check_counts(a, n, what="rays"):
    """Raises unless `a` is a C-contiguous (n,) array of counts (rt_intersect_all's, rt_ambient_occlusion's): uint32 for numpy, int32 for torch."""
    _check_kind_dtype(a, "counts", "int32" if _is_torch(a) else "uint32")
    if len(a.shape) != 1:
        raise ValueError(f"counts: shape {tuple(a.shape)}, expected (N,)")
    if not _contiguous(a):
        raise ValueError("counts: not C-contiguous")
    if a.shape[0] != n:
        raise ValueError(f"counts: {a.shape[0]} rows for {n} {what}")


def _addr(a):
    return C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data)


def _empty_like_batch(rays, shape, dtype_name):
    if _is_torch(rays):
        import torch
        return torch.empty(shape, dtype={"float32": torch.float32, "bool": torch.bool}[dtype_name], device=rays.device)
    return np.empty(shape, np.dtype(dtype_name))


def _out_like(out, batch, batch_name, n, cols, dtype_name="float32"):
    """The output array of a query over `batch` (n records): made like it (kind, device) when `out` is None, else `out` once it is of
    the same kind and a C-contiguous (n, cols) array - (n,) with cols = 0 - of dtype_name."""
    if out is None:
        return _empty_like_batch(batch, (n, cols) if cols else (n,), dtype_name)
    if _is_torch(out) != _is_torch(batch):
        raise TypeError(f"out: must be the same kind (numpy / torch) as {batch_name}")
    if _check_batch(out, "out", cols, dtype_name) != n:
        raise ValueError(f"out: {out.shape[0]} rows for {n} {batch_name}")
    return out


def _counts_like(counts, batch, batch_name, n):
    """The (n,) counts array beside a query's output (_check_counts): made like `batch` when None, else checked."""
    if counts is None:
        if _is_torch(batch):
            import torch
            return torch.empty((n,), dtype=torch.int32, device=batch.device)
        return np.empty((n,), np.uint32)
    if _is_torch(counts) != _is_torch(batch):
        raise TypeError(f"counts: must be the same kind (numpy / torch) as {batch_name}")
    _check_counts(counts, n, batch_name)
    return counts


def _votes_like(votes, batch, n):
    """The (n,) uint8 votes array of inside / signed_distance: None when not asked for (False / None), made like `batch` for True,
    else the caller's array, checked."""
    if votes is None or votes is False:
        return None
    if votes is True:
        if _is_torch(batch):
            import torch
            return torch.empty((n,), dtype=torch.uint8, device=batch.device)
        return np.empty((n,), np.uint8)
    _check_kind_dtype(votes, "votes", "uint8")
    if _is_torch(votes) != _is_torch(batch):
        raise TypeError("votes: must be the same kind (numpy / torch) as points")
    if len(votes.shape) != 1:
        raise ValueError(f"votes: shape {tuple(votes.shape)}, expected (N,)")
    if not _contiguous(votes):
        raise ValueError("votes: not C-contiguous")
    if votes.shape[0] != n:
        raise ValueError(f"votes: {votes.shape[0]} rows for {n} points")
    return votes


def _inside_params(rays, counters):
    """The rt_inside_params record (types.INSIDE_PARAMS) of inside / signed_distance, `rays` checked before the library sees it."""
    if isinstance(rays, bool) or not isinstance(rays, (int, np.integer)) or rays not in (1, 3, 5, 7):
        raise ValueError(f"rays: {rays!r}, expected one of the integers 1, 3, 5, 7")
    ip = np.zeros((), dtype=T.INSIDE_PARAMS)
    ip["rays"], ip["flags"] = int(rays), QUERY_COUNTERS if counters else 0
    return ip


def _path_params(samples,max_bounces, seed, first_sample, flags):
    """The rt_path_params record (types.PATH_PARAMS) of radiance / radiance_sh / irradiance from their four integers, checked."""
    for name, v, lo, hi in (("samples", samples, 1, PATH_MAX_SAMPLES), ("max_bounces", max_bounces, 0, MAX_BOUNCES), ("seed", seed, 0, 0xFFFFFFFF),
                            ("first_sample", first_sample, 0, 0xFFFFFFFF)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name}: {v!r}, expected an integer in {lo} .. {hi}")
    if int(first_sample) + int(samples) > 1 << 32:
        raise ValueError(f"first_sample: {first_sample!r} + samples {samples!r} passes 2^32")
    pp = np.zeros((), dtype=T.PATH_PARAMS)
    pp["samples"], pp["max_bounces"], pp["seed"], pp["first_sample"], pp["flags"] = int(samples), int(max_bounces), int(seed), int(first_sample), flags
    return pp


def _sync_torch(*tensors):
    """The library reads device tensors on its own stream: finish what torch has queued for them first."""
    for a in tensors:
        if _is_torch(a) and a.device.type != "cpu":
            import torch
            torch.cuda.current_stream(a.device).synchronize()


def make_rays(origins, directions, tmin=1e-5, tmax=float("inf")):
    """(N, 3) origins and directions (numpy or torch, the result has the same kind and device) -> an (N, 8) float32 ray batch.
    tmin / tmax: scalars or (N,) arrays."""
    if _is_torch(origins):
        import torch
        o = origins.reshape(-1, 3)
        out = torch.empty((o.shape[0], 8), dtype=torch.float32, device=o.device)
    else:
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        out = np.empty((o.shape[0], 8), np.float32)
    out[:, 0:3] = o
    out[:, 3] = tmin
    out[:, 4:7] = directions.reshape(-1, 3) if _is_torch(directions) else np.asarray(directions, np.float32).reshape(-1, 3)
    out[:, 7] = tmax
    return out


def split_hits(hits):
    """(N, 4) hit records -> (t, u, v, prim).  prim: uint32 for numpy, int64 for torch (a miss is 4294967295 = PRIM_MISS)."""
    if _is_torch(hits):
        import torch
        prim = hits[:, 3].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return hits[:, 0], hits[:, 1], hits[:, 2], prim
    return hits[:, 0], hits[:, 1], hits[:, 2], np.ascontiguousarray(hits[:, 3]).view(np.uint32)


def split_surface(points):
    """(N, 8) surface records (rt_surface_point) -> (position (N, 3), prim_id (N,), normal (N, 3), material_id (N,)).  The ids are the
    records' uint32 words: uint32 for numpy, int64 for torch (a miss is 4294967295 = PRIM_MISS), as split_hits gives prim."""
    if _is_torch(points):
        import torch
        ids = [points[:, c].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF for c in (3, 7)]
    else:
        ids = [np.ascontiguousarray(points[:, c]).view(np.uint32) for c in (3, 7)]
    return points[:, 0:3], ids[0], points[:, 4:7], ids[1]


def make_points(positions, radius=float("inf")):
    """(N, 3) positions (numpy or torch, the result has the same kind and device) -> an (N, 4) float32 batch of rt_point_query
    records: px py pz radius.  radius: a scalar or an (N,) array; only surface strictly nearer than it is reported."""
    if _is_torch(positions):
        import torch
        p = positions.reshape(-1, 3)
        out = torch.empty((p.shape[0], 4), dtype=torch.float32, device=p.device)
    else:
        p = np.asarray(positions, np.float32).reshape(-1, 3)
        out = np.empty((p.shape[0], 4), np.float32)
    out[:, 0:3] = p
    out[:, 3] = radius
    return out


def split_nearest(nearest):
    """(N, 8) closest-point records (rt_nearest) -> (position (N, 3), distance (N,), u (N,), v (N,), prim_id (N,), material_id (N,)).
    The ids are the records' uint32 words: uint32 for numpy, int64 for torch (a miss is 4294967295 = PRIM_MISS), as split_hits gives prim."""
    if _is_torch(nearest):
        import torch
        ids = [nearest[:, c].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF for c in (6, 7)]
    else:
        ids = [np.ascontiguousarray(nearest[:, c]).view(np.uint32) for c in (6, 7)]
    return nearest[:, 0:3], nearest[:, 3], nearest[:, 4], nearest[:, 5], ids[0], ids[1]


def make_sweeps(origins, directions, radius, tmax=float("inf")):
    """(N, 3) origins and directions (numpy or torch, the result has the same kind and device) -> an (N, 8) float32 batch of rt_sweep
    records: ox oy oz radius dx dy dz tmax.  radius / tmax: scalars or (N,) arrays; contacts at 0 <= t < tmax are reported."""
    out = make_rays(origins, directions, tmin=0.0, tmax=tmax)
    out[:, 3] = radius
    return out


def make_boxes(center, half_extent):
    """(N, 3) centres (numpy or torch, the result has the same kind and device) -> an (N, 8) float32 batch of rt_box records:
    cx cy cz 0 hx hy hz 0.  half_extent: a scalar, a triple or an (N, 3) array, >= 0 per axis; 0 is allowed (a slab, a segment, a point)."""
    if _is_torch(center):
        import torch
        c = center.reshape(-1, 3)
        out = torch.zeros((c.shape[0], 8), dtype=torch.float32, device=c.device)
        h = half_extent if _is_torch(half_extent) else torch.as_tensor(np.asarray(half_extent, np.float32), device=c.device)
    else:
        c = np.asarray(center, np.float32).reshape(-1, 3)
        out = np.zeros((c.shape[0], 8), np.float32)
        h = np.asarray(half_extent, np.float32)
    out[:, 0:3] = c
    out[:, 4:7] = h
    return out


def split_sweep_hits(records):
    """(N, 8) sweep records (rt_sweep_hit) -> (position (N, 3), t (N,), u (N,), v (N,), prim_id (N,), material_id (N,)): rt_nearest's
    layout with t where the distance is, so the ids come as split_nearest gives them."""
    return split_nearest(records)


def make_box_sweeps(centers, half_extents, directions, tmax=float("inf")):
    """(N, 3) centres and directions (numpy or torch, the result has the same kind and device) -> an (N, 12) float32 batch of
    rt_box_sweep records: cx cy cz 0 hx hy hz 0 dx dy dz tmax.  half_extents: a scalar, a triple or an (N, 3) array, >= 0 per axis; 0
    is allowed (a moving slab, segment, point).  tmax: a scalar or an (N,) array; contacts at 0 <= t < tmax are reported."""
    boxes = make_boxes(centers, half_extents)
    if _is_torch(boxes):
        import torch
        out = torch.zeros((boxes.shape[0], 12), dtype=torch.float32, device=boxes.device)
        d = directions if _is_torch(directions) else torch.as_tensor(np.asarray(directions, np.float32), device=boxes.device)
        tmax = tmax if _is_torch(tmax) else torch.as_tensor(np.asarray(tmax, np.float32), device=boxes.device)
    else:
        out = np.zeros((boxes.shape[0], 12), np.float32)
        d = np.asarray(directions, np.float32)
    out[:, 0:8] = boxes
    out[:, 8:11] = d.reshape(-1, 3)
    out[:, 11] = tmax
    return out


def make_obbs(center, half_extent, rotation):
    """(N, 3) centres (numpy or torch, the result has the same kind and device) -> an (N, 12) float32 batch of rt_obb records:
    cx cy cz 0 hx hy hz 0 qx qy qz qw.  half_extent as for make_boxes, along the box's own axes.  rotation: a quaternion x, y, z, w
    or an (N, 4) array of them, turning the box's axes into world axes; it need not be normalised."""
    boxes = make_boxes(center, half_extent)
    if _is_torch(boxes):
        import torch
        out = torch.zeros((boxes.shape[0], 12), dtype=torch.float32, device=boxes.device)
        q = rotation if _is_torch(rotation) else torch.as_tensor(np.asarray(rotation, np.float32), device=boxes.device)
    else:
        out = np.zeros((boxes.shape[0], 12), np.float32)
        q = np.asarray(rotation, np.float32)
    out[:, 0:8] = boxes
    out[:, 8:12] = q
    return out


def make_triangles(v0, v1, v2):
    """Three (N, 3) arrays of vertices (numpy or torch, the result has the kind and device of v0) -> an (N, 12) float32 batch of
    rt_query_triangle records: v0 0 v1 0 v2 0 (x y z per vertex).  Two or three equal vertices are allowed (a segment, a point)."""
    if _is_torch(v0):
        import torch
        a = v0.reshape(-1, 3)
        out = torch.zeros((a.shape[0], 12), dtype=torch.float32, device=a.device)
        b, c = (v if _is_torch(v) else torch.as_tensor(np.asarray(v, np.float32), device=a.device) for v in (v1, v2))
    else:
        a = np.asarray(v0, np.float32).reshape(-1, 3)
        out = np.zeros((a.shape[0], 12), np.float32)
        b, c = np.asarray(v1, np.float32), np.asarray(v2, np.float32)
    out[:, 0:3] = a
    out[:, 4:7] = b.reshape(-1, 3)
    out[:, 8:11] = c.reshape(-1, 3)
    return out


def make_triangle_sweeps(v0, v1, v2, direction, tmax=float("inf")):
    """Three (N, 3) arrays of vertices at t = 0 and (N, 3) directions (numpy or torch, the result has the kind and device of v0) -> an
    (N, 16) float32 batch of rt_triangle_sweep records: v0 0 v1 0 v2 0 dx dy dz tmax.  Equal vertices are allowed (a moving segment,
    a moving point).  tmax: a scalar or an (N,) array; contacts at 0 <= t < tmax are reported."""
    tris = make_triangles(v0, v1, v2)
    if _is_torch(tris):
        import torch
        out = torch.zeros((tris.shape[0], 16), dtype=torch.float32, device=tris.device)
        d = direction if _is_torch(direction) else torch.as_tensor(np.asarray(direction, np.float32), device=tris.device)
        tmax = tmax if _is_torch(tmax) else torch.as_tensor(np.asarray(tmax, np.float32), device=tris.device)
    else:
        out = np.zeros((tris.shape[0], 16), np.float32)
        d = np.asarray(direction, np.float32)
    out[:, 0:12] = tris
    out[:, 12:15] = d.reshape(-1, 3)
    out[:, 15] = tmax
    return out


def split_triangle_sweep_hits(records):
    """(N, 8) triangle-sweep records (rt_triangle_sweep_hit) -> (normal (N, 3), t (N,), axis (N,), prim_id (N,), material_id (N,)): the
    layout of split_box_sweep_hits, with axis 0 .. 25, SWEEP_TRIANGLE_AXIS_SPHERE or SWEEP_AXIS_NONE."""
    return split_box_sweep_hits(records)


def make_obb_sweeps(center, half_extent, rotation, direction, tmax=float("inf")):
    """(N, 3) centres and world directions (numpy or torch, the result has the same kind and device) -> an (N, 16) float32 batch of
    rt_obb_sweep records: cx cy cz 0 hx hy hz 0 qx qy qz qw dx dy dz tmax.  half_extent and rotation as for make_obbs; tmax: a scalar
    or an (N,) array; contacts at 0 <= t < tmax are reported."""
    sweeps = make_box_sweeps(center, half_extent, direction, tmax)
    boxes = make_obbs(center, half_extent, rotation)
    if _is_torch(boxes):
        import torch
        out = torch.zeros((boxes.shape[0], 16), dtype=torch.float32, device=boxes.device)
    else:
        out = np.zeros((boxes.shape[0], 16), np.float32)
    out[:, 0:12] = boxes
    out[:, 12:16] = sweeps[:, 8:12]
    return out


def make_poses(position, rotation):
    """(N, 3) positions (numpy or torch, the result has the same kind and device) -> an (N, 8) float32 batch of rt_pose records:
    px py pz 0 qx qy qz qw.  rotation: a quaternion x, y, z, w or an (N, 4) array of them, turning the mesh's axes into world axes,
    as for make_obbs; it need not be normalised.  The position is added after the rotation."""
    if _is_torch(position):
        import torch
        p = position.reshape(-1, 3)
        out = torch.zeros((p.shape[0], 8), dtype=torch.float32, device=p.device)
        q = rotation if _is_torch(rotation) else torch.as_tensor(np.asarray(rotation, np.float32), device=p.device)
    else:
        p = np.asarray(position, np.float32).reshape(-1, 3)
        out = np.zeros((p.shape[0], 8), np.float32)
        q = np.asarray(rotation, np.float32)
    out[:, 0:3] = p
    out[:, 4:8] = q
    return out


def make_pose_sweeps(position, rotation, direction, tmax=float("inf")):
    """(N, 3) positions and world directions (numpy or torch, the result has the same kind and device) -> an (N, 12) float32 batch of
    rt_pose_sweep records: px py pz 0 qx qy qz qw dx dy dz tmax.  position and rotation as for make_poses; the direction is not
    turned by the pose; tmax: a scalar or an (N,) array; contacts at 0 <= t < tmax are reported."""
    poses = make_poses(position, rotation)
    if _is_torch(poses):
        import torch
        out = torch.zeros((poses.shape[0], 12), dtype=torch.float32, device=poses.device)
        d = direction if _is_torch(direction) else torch.as_tensor(np.asarray(direction, np.float32), device=poses.device)
        tmax = tmax if _is_torch(tmax) else torch.as_tensor(np.asarray(tmax, np.float32), device=poses.device)
    else:
        out = np.zeros((poses.shape[0], 12), np.float32)
        d = np.asarray(direction, np.float32)
    out[:, 0:8] = poses
    out[:, 8:11] = d.reshape(-1, 3)
    out[:, 11] = tmax
    return out


def split_mesh_sweep_hits(records):
    """(N, 8) posed-mesh sweep records (rt_mesh_sweep_hit) -> (normal (N, 3), t (N,), axis (N,), triangle (N,), prim_id (N,),
    material_id (N,)): split_triangle_sweep_hits with the mesh triangle that touches first, PRIM_MISS for a miss.  The words are uint32
    for numpy, int64 for torch."""
    if _is_torch(records):
        import torch
        words = [records[:, c].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF for c in (4, 5, 6, 7)]
    else:
        words = [np.ascontiguousarray(records[:, c]).view(np.uint32) for c in (4, 5, 6, 7)]
    return records[:, 0:3], records[:, 3], words[0], words[1], words[2], words[3]


def pose_frames(poses):
    """The rotation matrices of an (N, 8) batch of poses (or the first 8 columns of an (N, 12) batch of pose sweeps) -> (R (N, 3, 3)
    float32, valid (N,) bool): the frame of csrc/obb_rules.h rule 1 in numpy float32, operation for operation, and the validity of
    csrc/mesh_pose_rules.h rule 1 (position and rotation finite, the squared norm finite and > 0)."""
    poses = np.asarray(poses, np.float32)
    x, y, z, w = (poses[:, 4 + k] for k in range(4))
    with np.errstate(all="ignore"):
        n = ((x * x + y * y) + z * z) + w * w
        s = np.float32(2.0) / n
        xs, ys, zs = x * s, y * s, z * s
        wx, wy, wz = w * xs, w * ys, w * zs
        xx, xy, xz, yy, yz, zz = x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
        one = np.float32(1.0)
        R = np.stack([one - (yy + zz), xy - wz, xz + wy, xy + wz, one - (xx + zz), yz - wx, xz - wy, yz + wx, one - (xx + yy)], axis=1).reshape(-1, 3, 3)
    valid = np.isfinite(poses[:, 0:3]).all(axis=1) & np.isfinite(poses[:, 4:8]).all(axis=1) & np.isfinite(n) & (n > 0)
    return R.astype(np.float32), valid


def pose_triangles(mesh, poses):
    """The (M, 12) mesh (make_triangles) at each pose of an (N, 8) batch (make_poses; an (N, 12) batch of pose sweeps is read the same)
    -> (N, M, 12) float32 rt_query_triangle records: the posing statement of rt_overlap_mesh / rt_sweep_mesh in numpy float32,
    operation for operation - w_a = ((R_a0 v_0 + R_a1 v_1) + R_a2 v_2) + position_a with R = pose_frames(poses) - so row [i, j] is
    bit for bit the triangle the device judges for pose i and mesh triangle j.  What the tests compare with, and what a caller
    draws the body with.  The rows of an invalid pose are not to be used (the calls answer it without looking at them)."""
    mesh, poses = np.asarray(mesh, np.float32), np.asarray(poses, np.float32)
    if mesh.ndim != 2 or mesh.shape[1] != 12:
        raise ValueError(f"mesh: shape {mesh.shape}, expected (M, 12)")
    if poses.ndim != 2 or poses.shape[1] not in (8, 12):
        raise ValueError(f"poses: shape {poses.shape}, expected (N, 8) or (N, 12)")
    R, _ = pose_frames(poses)
    out = np.zeros((poses.shape[0], mesh.shape[0], 12), np.float32)
    with np.errstate(all="ignore"):
        for k in range(3):
            v = mesh[None, :, 4 * k:4 * k + 3]  # (1, M, 3)
            for a in range(3):
                r = (R[:, a, 0, None] * v[:, :, 0] + R[:, a, 1, None] * v[:, :, 1]) + R[:, a, 2, None] * v[:, :, 2]
                out[:, :, 4 * k + a] = r + poses[:, a, None]
    return out


def split_box_sweep_hits(records):
    """(N, 8) box-sweep records (rt_box_sweep_hit, of sweep_box or sweep_obb) -> (normal (N, 3), t (N,), axis (N,), prim_id (N,), material_id (N,)).  axis and the
    ids are the records' uint32 words: uint32 for numpy, int64 for torch (a miss is 4294967295 = PRIM_MISS with axis SWEEP_AXIS_NONE)."""
    if _is_torch(records):
        import torch
        words = [records[:, c].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF for c in (4, 6, 7)]
    else:
        words = [np.ascontiguousarray(records[:, c]).view(np.uint32) for c in (4, 6, 7)]
    return records[:, 0:3], records[:, 3], words[0], words[1], words[2]


def make_capsule_sweeps(origins, axes, directions, radius, tmax=float("inf")):
    """(N, 3) origins (end A of each axis) and directions (numpy or torch, the result has the same kind and device) -> an (N, 12)
    float32 batch of rt_capsule_sweep records: ox oy oz radius ax ay az 0 dx dy dz tmax.  axes: B - A, a triple or an (N, 3) array;
    zero is allowed (a moving sphere).  radius / tmax: scalars or (N,) arrays; contacts at 0 <= t < tmax are reported."""
    if _is_torch(origins):
        import torch
        o = origins.reshape(-1, 3)
        out = torch.zeros((o.shape[0], 12), dtype=torch.float32, device=o.device)
        conv = lambda x: x if _is_torch(x) else torch.as_tensor(np.asarray(x, np.float32), device=o.device)
    else:
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        out = np.zeros((o.shape[0], 12), np.float32)
        conv = lambda x: np.asarray(x, np.float32)
    out[:, 0:3] = o
    out[:, 3] = conv(radius)
    out[:, 4:7] = conv(axes).reshape(-1, 3)
    out[:, 8:11] = conv(directions).reshape(-1, 3)
    out[:, 11] = conv(tmax)
    return out


def split_capsule_sweep_hits(records):
    """(N, 8) capsule-sweep records (rt_capsule_sweep_hit) -> (position (N, 3), t (N,), s (N,), prim_id (N,), material_id (N,)).  The
    ids are the records' uint32 words: uint32 for numpy, int64 for torch (a miss is 4294967295 = PRIM_MISS)."""
    if _is_torch(records):
        import torch
        words = [records[:, c].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF for c in (6, 7)]
    else:
        words = [np.ascontiguousarray(records[:, c]).view(np.uint32) for c in (6, 7)]
    return records[:, 0:3], records[:, 3], records[:, 4], words[0], words[1]


def make_capsules(origin, radius, axis):
    """(N, 3) origins (end A of each axis; numpy or torch, the result has the same kind and device) -> an (N, 8) float32 batch of
    rt_capsule records: ox oy oz radius ax ay az 0, the first eight columns of make_capsule_sweeps.  radius: a scalar or an (N,) array,
    > 0, inf allowed.  axis: B - A, a triple or an (N, 3) array; zero is allowed (a resting sphere)."""
    if _is_torch(origin):
        import torch
        o = origin.reshape(-1, 3)
        out = torch.zeros((o.shape[0], 8), dtype=torch.float32, device=o.device)
        conv = lambda x: x if _is_torch(x) else torch.as_tensor(np.asarray(x, np.float32), device=o.device)
    else:
        o = np.asarray(origin, np.float32).reshape(-1, 3)
        out = np.zeros((o.shape[0], 8), np.float32)
        conv = lambda x: np.asarray(x, np.float32)
    out[:, 0:3] = o
    out[:, 3] = conv(radius)
    out[:, 4:7] = conv(axis).reshape(-1, 3)
    return out


def split_contacts(records):
    """(N, 8) contact records (rt_contact; contact_capsule's out.reshape(-1, 8)) -> (position (N, 3), distance (N,), s (N,), prim_id
    (N,), material_id (N,)): rt_capsule_sweep_hit's layout with the distance where t is, so the ids come as split_capsule_sweep_hits
    gives them (an unused slot is 4294967295 = PRIM_MISS).  normal = (origin + axis * s - position) / distance, depth = radius - distance."""
    return split_capsule_sweep_hits(records)


def make_contact_triangles(v0, v1, v2, margin):
    """Three (N, 3) arrays of vertices (numpy or torch, the result has the kind and device of v0) and margins (a scalar or an (N,)
    array, > 0, inf allowed) -> an (N, 12) float32 batch of rt_triangle_contact_query records: v0 margin v1 0 v2 0.  Equal vertices
    are allowed (a segment, a point)."""
    out = make_triangles(v0, v1, v2)
    if _is_torch(out):
        import torch
        margin = margin if _is_torch(margin) else torch.as_tensor(np.asarray(margin, np.float32), device=out.device)
    else:
        margin = np.asarray(margin, np.float32)
    out[:, 3] = margin
    return out


def split_triangle_contacts(records):
    """(N, 8) triangle-contact records (rt_triangle_contact; contact_triangle's out.reshape(-1, 8)) -> (position (N, 3), distance
    (N,), qu (N,), qv (N,), prim_id (N,), material_id (N,)): rt_nearest's layout with the query's weights where the primitive's are, so
    the ids come as split_nearest gives them (an unused slot is 4294967295 = PRIM_MISS).  normal = ((v0 + (v1 - v0) qu + (v2 - v0) qv) -
    position) / distance, depth = margin - distance."""
    return split_nearest(records)


def split_lighting(lighting):
    """(N, 4) lighting records (rt_lighting) -> (radiance (N, 3), lit_mask (N,)).  lit_mask is the records' uint32 word: uint32 for
    numpy, int64 for torch; bit li set: light li entered the sum."""
    if _is_torch(lighting):
        import torch
        mask = lighting[:, 3].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    else:
        mask = np.ascontiguousarray(lighting[:, 3]).view(np.uint32)
    return lighting[:, 0:3], mask


def split_radiance(results):
    """(N, 4) path results (rt_path_result) -> (radiance (N, 3), segments (N,)).  segments is the records' uint32 word: uint32 for
    numpy, int64 for torch; the segments traced for the ray over all its samples."""
    if _is_torch(results):
        import torch
        segments = results[:, 3].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    else:
        segments = np.ascontiguousarray(results[:, 3]).view(np.uint32)
    return results[:, 0:3], segments


def make_probes(positions):
    """(N, 3) positions (numpy or torch, the result has the same kind and device) -> an (N, 4) float32 batch of rt_probe records:
    px py pz and the ignored pad word, zero."""
    return make_points(positions, 0.0)


def split_sh(results):
    """(N, 28) probe results (rt_sh9) -> (sh (N, 9, 3), segments (N,)).  sh[:, j, c] is coefficient j of colour channel c; segments is
    the records' uint32 word: uint32 for numpy, int64 for torch; the segments traced for the probe over all its samples."""
    if _is_torch(results):
        import torch
        segments = results[:, 27].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    else:
        segments = np.ascontiguousarray(results[:, 27]).view(np.uint32)
    return results[:, 0:27].reshape(-1, 9, 3), segments


def split_irradiance(results):
    """(N, 4) irradiance records (rt_irradiance_result) -> (irradiance (N, 3), segments (N,)).  segments is the records' uint32 word:
    uint32 for numpy, int64 for torch; the segments traced for the point over all its samples."""
    return split_radiance(results)


_SH9_COSINE = (np.pi, 2.0 * np.pi / 3.0, 2.0 * np.pi / 3.0, 2.0 * np.pi / 3.0, np.pi / 4.0, np.pi / 4.0, np.pi / 4.0, np.pi / 4.0, np.pi / 4.0)


def _sh9_basis(directions):
    """The 9 real SH basis functions of rt_radiance_sh at (N, 3) unit directions (numpy or torch) -> (N, 9), in the input's dtype."""
    x, y, z = directions[:, 0], directions[:, 1], directions[:, 2]
    cols = [0.2820948 + 0.0 * x, 0.4886025 * y, 0.4886025 * z, 0.4886025 * x, 1.0925484 * (x * y), 1.0925484 * (y * z),
            0.31539157 * (3.0 * (z * z) - 1.0), 1.0925484 * (x * z), 0.5462742 * (x * x - y * y)]
    if _is_torch(directions):
        import torch
        return torch.stack(cols, dim=1)
    return np.stack(cols, axis=1)


def sh9_irradiance(sh, normals):
    """The cosine-convolved irradiance of (N, 9, 3) coefficients (split_sh) at (N, 3) unit normals -> (N, 3): sum_j A_j sh_j Y_j(n) with
    A = pi (j = 0), 2 pi / 3 (j = 1..3), pi / 4 (j = 4..8) (Ramamoorthi and Hanrahan 2001).  numpy or torch, both of one kind."""
    if _is_torch(sh) != _is_torch(normals):
        raise TypeError("normals: must be the same kind (numpy / torch) as sh")
    weights = _sh9_basis(normals)
    if _is_torch(sh):
        import torch
        weights = weights * torch.tensor(_SH9_COSINE, dtype=weights.dtype, device=weights.device)
    else:
        weights = weights * np.asarray(_SH9_COSINE, weights.dtype)
    return (sh * weights[:, :, None]).sum(1)


def split_aovs(aovs):
    """(..., 8) AOV records (rt_aov: albedo xyz, depth, normal xyz, coverage; numpy or torch) -> dict of views: albedo (..., 3),
    depth (...), normal (..., 3), coverage (...)."""
    return {"albedo": aovs[..., 0:3], "depth": aovs[..., 3], "normal": aovs[..., 4:7], "coverage": aovs[..., 7]}


def split_adaptive(records):
    """(..., 8) adaptive-sampling records (rt_adaptive_pixel: S xyz, n, H xyz, error; numpy or torch) -> dict of views: sum (..., 3),
    samples (...), odd (..., 3), error (...)."""
    return {"sum": records[..., 0:3], "samples": records[..., 3], "odd": records[..., 4:7], "error": records[..., 7]}


def _check_image(a, name, h, w, c):
    """Raises unless `a` is a C-contiguous float32 (h, w, c) numpy array or torch tensor."""
    if _is_torch(a):
        import torch
        if a.dtype != torch.float32:
            raise TypeError(f"{name}: dtype {a.dtype}, expected torch.float32")
        shape, contiguous = tuple(a.shape), a.is_contiguous()
    elif isinstance(a, np.ndarray):
        if a.dtype != np.float32:
            raise TypeError(f"{name}: dtype {a.dtype}, expected float32")
        shape, contiguous = a.shape, a.flags.c_contiguous
    else:
        raise TypeError(f"{name}: a numpy array or a torch tensor, not {type(a).__name__}")
    if tuple(shape) != (h, w, c):
        raise ValueError(f"{name}: shape {tuple(shape)}, expected {(h, w, c)}")
    if not contiguous:
        raise ValueError(f"{name}: not C-contiguous")


def render_params(width, height, camera, mode=MODE_LEGACY, spp=1, max_bounces=4, frame_seed=0, tile_size=0, tile_rank=0, tile_world=1,
                  counters=False, no_shadows=False, kernel_v1=False, kernel_sm=False, no_shadow_grid=False, kernel_pipeline=False, no_beams=False,
                  stage_times=False, accumulate=False, restart=False):
    """An rt_render_params record (types.RENDER_PARAMS) from the keyword arguments of Context.render."""
    if restart and not accumulate:
        raise ValueError("render: restart=True needs accumulate=True")
    p = np.zeros((), dtype=T.RENDER_PARAMS)
    p["camera"] = camera
    p["width"], p["height"], p["spp"], p["max_bounces"], p["mode"] = width, height, spp, max_bounces, mode
    p["frame_seed"], p["tile_size"], p["tile_rank"], p["tile_world"] = frame_seed, tile_size, tile_rank, tile_world
    p["flags"] = (FLAG_COUNTERS if counters else 0) | (FLAG_NO_SHADOWS if no_shadows else 0) | (FLAG_KERNEL_V1 if kernel_v1 else 0) | (FLAG_KERNEL_SM if kernel_sm else 0) | (FLAG_NO_SHADOW_GRID if no_shadow_grid else 0) | (FLAG_KERNEL_PIPELINE if kernel_pipeline else 0) | (FLAG_NO_BEAMS if no_beams else 0) | (FLAG_STAGE_TIMES if stage_times else 0)
    p["flags"] |= (FLAG_ACCUMULATE if accumulate else 0) | (FLAG_ACCUMULATE_RESTART if restart else 0)
    return p


def _init_torch_device_runtime():
    """torch ships its own HIP runtime.  In one process it has to come up before the library's: torch initialised after a
    context exists reports "No HIP GPUs are available".  Done only when the program has imported torch."""
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available():
        torch.cuda.init()


class Context:
    """One rt_ctx.  Mirrors the life cycle RenderState/BufferManager/ComputeRenderer have in the reference."""

    def __init__(self, device_ids=(0,)):
        self.lib = load()
        _init_torch_device_runtime()
        self._h = C.c_void_p(0)
        ids = (C.c_int * len(device_ids))(*device_ids)
        rc = self.lib.rt_create(C.byref(self._h), ids, C.c_int(len(device_ids)))
        if rc != RT_OK:
            raise RtError(rc, self.lib.rt_last_error(None).decode())
        self.width = self.height = 0

    def _check(self, rc):
        if rc != RT_OK:
            raise RtError(rc, self.lib.rt_last_error(self._h).decode())

    def close(self):
        if self._h:
            self.lib.rt_destroy(self._h)
            self._h = C.c_void_p(0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- uploads ---------------------------------------------------------------------
    def upload_scene(self, scene, ref_nodes=None, ref_tri_indices=None):
        keep = [np.ascontiguousarray(a) for a in (scene.spheres, scene.lights, scene.vertices, scene.triangles, scene.materials)]
        sp, li, ve, tr, ma = keep
        rn = np.ascontiguousarray(ref_nodes) if ref_nodes is not None else None
        ri = np.ascontiguousarray(ref_tri_indices, dtype=np.uint32) if ref_tri_indices is not None else None
        self._check(self.lib.rt_upload_scene(
            self._h, _p(sp), C.c_uint32(len(sp)), _p(li), C.c_uint32(len(li)), _p(ve), C.c_uint32(len(ve)),
            _p(tr), C.c_uint32(len(tr)), _p(ma), C.c_uint32(len(ma)),
            _p(rn), C.c_uint32(0 if rn is None else len(rn)), _p(ri), C.c_uint32(0 if ri is None else len(ri))))
        self._n_vertices, self._n_spheres = len(ve), len(sp)

    def upload_scene_packed(self, metadata, offsets, tri_bufs, triangles_per_buffer, materials):
        md = np.ascontiguousarray(metadata, dtype=np.uint32)
        off = np.ascontiguousarray(offsets)
        bufs = [np.ascontiguousarray(b) for b in tri_bufs]
        ptrs = (C.c_void_p * 3)(*[b.ctypes.data if b.size else None for b in bufs])
        counts = (C.c_uint32 * 3)(*[len(b) for b in bufs])
        ma = np.ascontiguousarray(materials)
        self._check(self.lib.rt_upload_scene_packed(
            self._h, _p(md), C.c_size_t(md.size), _p(off), ptrs, counts, C.c_uint32(triangles_per_buffer),
            _p(ma), C.c_uint32(len(ma))))
        o = off.reshape(-1)[0]
        self._n_vertices, self._n_spheres = int(o["vertices_count"]), int(o["spheres_count"])

    def update_geometry(self, vertices=None, spheres=None, rebuild=False):
        """rt_update_geometry: new positions for the uploaded scene, in place.  vertices: (n, 3) float32, numpy or a torch tensor on
        the CPU or on a device of the context; spheres: a types.SPHERE structured array (numpy).  None = unchanged; the counts
        must be those of the last upload.  The tree is refitted, or rebuilt with rebuild=True.  Returns the stats (flags:
        STAT_REFIT / STAT_REBUILT)."""
        n_up_v, n_up_s = getattr(self, "_n_vertices", None), getattr(self, "_n_spheres", None)
        if n_up_v is None:
            raise RtError(-4, "update_geometry: no scene uploaded")
        if vertices is not None:
            if _check_batch(vertices, "vertices", 3, "float32") != n_up_v:
                raise ValueError(f"vertices: count {len(vertices)}, the scene was uploaded with {n_up_v}")
        if spheres is not None:
            if not isinstance(spheres, np.ndarray) or spheres.dtype != T.SPHERE:
                raise TypeError(f"spheres: a numpy array of dtype types.SPHERE, not {getattr(spheres, 'dtype', type(spheres).__name__)}")
            if spheres.ndim != 1:
                raise ValueError(f"spheres: shape {spheres.shape}, expected (N,)")
            if len(spheres) != n_up_s:
                raise ValueError(f"spheres: count {len(spheres)}, the scene was uploaded with {n_up_s}")
            spheres = np.ascontiguousarray(spheres)
        if vertices is not None:
            _sync_torch(vertices)
        self._check(self.lib.rt_update_geometry(
            self._h, _addr(vertices) if vertices is not None else C.c_void_p(0), C.c_uint32(0 if vertices is None else n_up_v),
            _p(spheres) if spheres is not None else C.c_void_p(0), C.c_uint32(0 if spheres is None else n_up_s),
            C.c_uint32(UPDATE_REBUILD if rebuild else 0)))
        return self.stats()

    def upload_textures(self, textures, texture_data):
        """Bindings 6-7 (TextureInfo[] + texture bytes): validated and recorded, never sampled (as in the reference)."""
        ti = np.ascontiguousarray(textures, dtype=T.TEXTURE_INFO)
        td = np.ascontiguousarray(texture_data, dtype=np.uint8)
        self._check(self.lib.rt_upload_textures(self._h, _p(ti), C.c_uint32(len(ti)), _p(td), C.c_size_t(td.size)))

    def prepare(self, what=PREPARE_SHADOW_GRIDS):
        """rt_prepare: build ahead of time what the first extended-mode frame would otherwise build (PREPARE_SHADOW_GRIDS: the light grids), and /
        or rebuild the tree with the host builder for a scene that stays (PREPARE_QUALITY_TREE)."""
        self._check(self.lib.rt_prepare(self._h, C.c_uint32(what)))

    # -- rendering -------------------------------------------------------------------
    def render(self, width, height, camera, mode=MODE_LEGACY, spp=1, max_bounces=4, frame_seed=0, tile_size=0,
               tile_rank=0, tile_world=1, counters=False, no_shadows=False, kernel_v1=False, kernel_sm=False, no_shadow_grid=False, kernel_pipeline=False, no_beams=False, stage_times=False,
               accumulate=False, restart=False):
        """rt_render.  accumulate=True (extended mode): add the spp samples to the context's running image and leave the mean over all of
        them in the targets (accumulated_samples() tells how many); restart=True with it starts a new running image at sample 0."""
        p = render_params(width, height, camera, mode=mode, spp=spp, max_bounces=max_bounces, frame_seed=frame_seed, tile_size=tile_size,
                          tile_rank=tile_rank, tile_world=tile_world, counters=counters, no_shadows=no_shadows, kernel_v1=kernel_v1,
                          kernel_sm=kernel_sm, no_shadow_grid=no_shadow_grid, kernel_pipeline=kernel_pipeline, no_beams=no_beams,
                          stage_times=stage_times, accumulate=accumulate, restart=restart)
        self._check(self.lib.rt_render(self._h, _p(p)))
        self.width, self.height = width, height
        return self.stats()

    def accumulated_samples(self):
        """rt_accumulated_samples: samples in the running image of the accumulating renders (0: none)."""
        n = C.c_uint32(0)
        self._check(self.lib.rt_accumulated_samples(self._h, C.byref(n)))
        return n.value

    def render_adaptive(self, width, height, camera, spp, threshold, min_samples=4, restart=False, **render_kw):
        """rt_render_adaptive: an accumulating extended-mode call (mode=2 and accumulate=True are implied) that traces spp samples only
        for the pixels the convergence rule leaves active (rt_hip.h "Adaptive sampling"); the other keyword arguments are Context.render's.
        Returns the call's stats (pixels: the pixels that received samples)."""
        render_kw.setdefault("mode", MODE_EXTENDED)
        p = render_params(width, height, camera, spp=spp, accumulate=True, restart=restart, **render_kw)
        ap = np.zeros((), dtype=T.ADAPTIVE_PARAMS)
        ap["threshold"], ap["min_samples"] = threshold, min_samples
        self._check(self.lib.rt_render_adaptive(self._h, _p(p), _p(ap)))
        self.width, self.height = width, height
        return self.stats()

    def read_adaptive(self):
        """rt_read_adaptive: the (height, width, 8) float32 records S, n, H, error of the adaptive running image (split_adaptive; a numpy
        array views as types.ADAPTIVE_PIXEL)."""
        out = np.zeros((self.height, self.width, 8), np.float32)
        self._check(self.lib.rt_read_adaptive(self._h, _p(out), C.c_size_t(self.height * self.width)))
        return out

    def dispatch_tile(self, pc):
        pcb = np.ascontiguousarray(pc)
        self._check(self.lib.rt_dispatch_tile(self._h, _p(pcb)))
        res = pcb["resolution"].reshape(-1)
        self.width, self.height = int(res[0]), int(res[1])

    # -- read-back -------------------------------------------------------------------
    def read_rgb32f(self):
        out = np.zeros((self.height, self.width, 3), np.float32)
        self._check(self.lib.rt_read_rgb32f(self._h, _p(out), C.c_size_t(out.size)))
        return out

    def read_rgba8_channels(self):
        outs = [np.zeros((self.height, self.width, 4), np.uint8) for _ in range(3)]
        self._check(self.lib.rt_read_rgba8_channels(self._h, _p(outs[0]), _p(outs[1]), _p(outs[2]), C.c_size_t(outs[0].size)))
        return outs

    def read_rgba8_combined(self):
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(self.lib.rt_read_rgba8_combined(self._h, _p(out), C.c_size_t(out.size)))
        return out

    def read_hits(self):
        prim = np.zeros((self.height, self.width), np.uint32)
        t = np.zeros((self.height, self.width), np.float32)
        self._check(self.lib.rt_read_hits(self._h, _p(prim), _p(t), C.c_size_t(prim.size)))
        return prim, t

    def debug_beams(self, n_blocks):
        """Development aid: per owned 8x8 pixel block the length of its camera-beam triangle list (0xFFFFFFFF: none)."""
        out = np.zeros(n_blocks, np.uint32)
        m = self.lib.rt_debug_beams(self._h, _p(out), C.c_uint32(n_blocks))
        if m < 0:
            raise RtError(m, "rt_debug_beams")
        return out[:m]

    def debug_stage_times(self):
        """(sum of the k_wf_shadow_grid launch durations in ms, launches) of the last frame rendered with stage_times=True."""
        out = (C.c_double * 2)()
        self._check(self.lib.rt_debug_stage_times(self._h, out))
        return float(out[0]), int(out[1])

    def debug_counters(self):
        out = (C.c_ulonglong * 8)()
        self._check(self.lib.rt_debug_counters(self._h, out))
        names = ("transition_passes", "transition_lanes", "node_iters", "node_lanes", "leaf_iters", "leaf_lanes", "cycles_transition", "cycles_traversal")
        return dict(zip(names, [int(v) for v in out]))

    def debug_stack_mark(self):
        """Development aid: the most traversal-stack entries a lane of k_wf_trace held in the last pipeline frame rendered with counters=True
        (WF_TOTAL_STACK_MAX, which rt_debug_counters reports in its first slot after such a frame)."""
        return self.debug_counters()["transition_passes"]

    def debug_shadow_grid(self, light=None):
        """Development aid: the light grids (csrc/shadow_grid.h) of the first device.  light=None: totals and the last counted frame's use."""
        out = (C.c_ulonglong * 8)()
        self._check(self.lib.rt_debug_shadow_grid(self._h, C.c_uint32(0xFFFFFFFF if light is None else light), out))
        names = ("lights_with_grid", "entries", "bytes", "segments_answered", "entries_read") if light is None else ("kind", "res", "entries", "near", "longest", "heavy_cells", "filled_cells")
        return dict(zip(names, [int(v) for v in out]))

    def debug_check_bvh(self):
        """Development aid: validate the tree this context holds on its first device the way the kernels decode it.
        Returns dict(failures, nodes, leaves, depth, real_depth, placed_once, method) - method 0 host SAH, 1 host PLOC, 2 device build."""
        out = (C.c_uint32 * 8)()
        fails = self.lib.rt_debug_check_bvh(self._h, out)
        names = ("nodes", "leaves", "depth", "real_depth", "placed_once", "method", "nodes_hash", "tris_hash")
        d = dict(zip(names, [int(v) for v in out]))
        d["failures"] = int(fails)
        return d

    # -- ray queries ---------------------------------------------------------------------
    def _query(self, fn, rays, out, cols, dtype_name, counters, in_cols=8, in_name="rays"):
        n = _check_batch(rays, in_name, in_cols, "float32")
        out = _out_like(out, rays, in_name, n, cols, dtype_name)
        _sync_torch(rays, out)
        self._check(getattr(self.lib, fn)(self._h, _addr(rays), C.c_size_t(n), _addr(out), C.c_uint32(QUERY_COUNTERS if counters else 0)))
        return out

    def intersect(self, rays, out=None, counters=False):
        """rt_intersect: closest hit of each ray of an (N, 8) batch -> (N, 4) float32 (t, u, v, prim_id bits; split_hits),
        same kind and device as `rays`."""
        return self._query("rt_intersect", rays, out, 4, "float32", counters)

    def occluded(self, rays, out=None, counters=False):
        """rt_occluded: any hit in each ray's range -> (N,) bool, same kind and device as `rays`."""
        return self._query("rt_occluded", rays, out, 0, "bool", counters)

    def intersect_all(self, rays, max_hits, out=None, counts=None, count_all=False, counters=False):
        """rt_intersect_all: the first max_hits (0 .. MULTI_HIT_MAX) hits along each ray of an (N, 8) batch, ordered as rt_intersect
        would pick them -> (hits, counts), same kind and device as `rays`.  hits: (N, max_hits, 4) float32, unused slots miss
        records (split_hits takes hits.reshape(-1, 4)), None for max_hits=0; counts: (N,) uint32 (numpy) / int32 (torch), the
        records listed per ray, or with count_all every candidate in the ray's range.  max_hits=0 needs count_all: a crossing count."""
        n = _check_batch(rays, "rays", 8, "float32")
        if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or not 0 <= max_hits <= MULTI_HIT_MAX:
            raise ValueError(f"max_hits: {max_hits!r}, expected an integer in 0 .. {MULTI_HIT_MAX}")
        max_hits = int(max_hits)
        if max_hits == 0 and not count_all:
            raise ValueError("max_hits: 0 lists nothing, which needs count_all=True (a pure crossing count)")
        if out is not None and _is_torch(out) != _is_torch(rays):
            raise TypeError("out: must be the same kind (numpy / torch) as rays")
        if max_hits == 0:
            out = None
        elif out is None:
            out = _empty_like_batch(rays, (n, max_hits, 4), "float32")
        else:
            _check_hit_lists(out, n, max_hits)
        counts = _counts_like(counts, rays, "rays", n)
        _sync_torch(rays, out, counts)
        flags = (QUERY_COUNTERS if counters else 0) | (QUERY_COUNT_ALL if count_all else 0)
        self._check(self.lib.rt_intersect_all(self._h, _addr(rays), C.c_size_t(n), C.c_uint32(max_hits),
                                              _addr(out) if out is not None else C.c_void_p(0), _addr(counts), C.c_uint32(flags)))
        return out, counts

    def surface(self, rays, out=None, counters=False):
        """rt_surface: the hit point, face-forwarded geometric normal, prim_id and material_id of each ray's closest hit -> (N, 8)
        float32 rt_surface_point records (split_surface), same kind and device as `rays`; a miss is all zero but prim_id = PRIM_MISS."""
        return self._query("rt_surface", rays, out, 8, "float32", counters)

    def ambient_occlusion(self, points, samples, seed=0, max_distance=float("inf"), bias=1e-3, out=None, counts=None, counters=False):
        """rt_ambient_occlusion: `samples` (1 .. AO_MAX_SAMPLES) cosine-distributed occlusion rays from each record of an (N, 8) batch
        of surface points (surface()) -> (visibility, counts), same kind and device as `points`.  visibility: (N,) float32, the
        fraction of a point's samples that reached max_distance; counts: (N,) uint32 (numpy) / int32 (torch), their number.  Sample s
        of point i draws from rng_for(seed + i, s); its ray starts at position + normal * bias."""
        n = _check_batch(points, "points", 8, "float32")
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= AO_MAX_SAMPLES:
            raise ValueError(f"samples: {samples!r}, expected an integer in 1 .. {AO_MAX_SAMPLES}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= 0xFFFFFFFF:
            raise ValueError(f"seed: {seed!r}, expected an integer in 0 .. 2^32 - 1")
        try:
            max_distance, bias = float(max_distance), float(bias)
        except (TypeError, ValueError):
            raise ValueError(f"max_distance / bias: {max_distance!r}, {bias!r}, expected numbers") from None
        if not max_distance > 0:
            raise ValueError(f"max_distance: {max_distance!r}, expected > 0 (inf allowed)")
        if not (np.isfinite(bias) and bias >= 0):
            raise ValueError(f"bias: {bias!r}, expected finite and >= 0")
        out = _out_like(out, points, "points", n, 0)
        counts = _counts_like(counts, points, "points", n)
        ap = np.zeros((), dtype=T.AO_PARAMS)
        ap["samples"], ap["seed"], ap["max_distance"], ap["bias"] = int(samples), int(seed), max_distance, bias
        ap["flags"] = QUERY_COUNTERS if counters else 0
        _sync_torch(points, out, counts)
        self._check(self.lib.rt_ambient_occlusion(self._h, _addr(points), C.c_size_t(n), _p(ap), _addr(out), _addr(counts)))
        return out, counts

    def direct_light(self, points, bias=1e-3, ambient=False, shadows=True, use_grids=True, out=None, counters=False):
        """rt_direct_light: the scene's lights at each record of an (N, 8) batch of surface points (surface()), with shadows -> (N, 4)
        float32 rt_lighting records (split_lighting: radiance, lit_mask), same kind and device as `points`.  The normal is used as
        given: surface()'s face-forwarded one lights the side the ray arrived on.  ambient: add 0.1 * albedo first (the frames'
        terminal vertex); shadows=False: no shadow segments; use_grids=False: every segment walks the tree (same results)."""
        n = _check_batch(points, "points", 8, "float32")
        try:
            bias = float(bias)
        except (TypeError, ValueError):
            raise ValueError(f"bias: {bias!r}, expected a number") from None
        if not (np.isfinite(bias) and bias >= 0):
            raise ValueError(f"bias: {bias!r}, expected finite and >= 0")
        out = _out_like(out, points, "points", n, 4)
        dp = np.zeros((), dtype=T.DIRECT_LIGHT_PARAMS)
        dp["bias"] = bias
        dp["flags"] = ((DIRECT_AMBIENT if ambient else 0) | (0 if shadows else DIRECT_NO_SHADOWS) | (0 if use_grids else DIRECT_NO_SHADOW_GRID)
                       | (QUERY_COUNTERS if counters else 0))
        _sync_torch(points, out)
        self._check(self.lib.rt_direct_light(self._h, _addr(points), C.c_size_t(n), _p(dp), _addr(out)))
        return out

    def radiance(self, rays, samples=1, max_bounces=4, seed=0, first_sample=0, shadows=True, camera_draws=False, out=None, counters=False):
        """rt_radiance: the extended mode's path radiance along each ray of an (N, 8) batch, `samples` (1 .. PATH_MAX_SAMPLES) paths
        per ray averaged as the frames average a pixel's samples -> (N, 4) float32 rt_path_result records (split_radiance: radiance,
        segments), same kind and device as `rays`.  Sample k of ray i draws from rng_for(seed + i, first_sample + k); max_bounces as
        in an extended-mode frame; shadows=False: no shadow segments; camera_draws=True: two draws are dropped first, the ones a
        jittered camera sample (sample_rays) spent on its jitter."""
        n = _check_batch(rays, "rays", 8, "float32")
        pp = _path_params(samples, max_bounces, seed, first_sample,
                          (0 if shadows else PATH_NO_SHADOWS) | (PATH_CAMERA_DRAWS if camera_draws else 0) | (QUERY_COUNTERS if counters else 0))
        out = _out_like(out, rays, "rays", n, 4)
        _sync_torch(rays, out)
        self._check(self.lib.rt_radiance(self._h, _addr(rays), C.c_size_t(n), _p(pp), _addr(out)))
        return out

    def radiance_sh(self, probes, samples, max_bounces=4, seed=0, first_sample=0, shadows=True, out=None, counters=False):
        """rt_radiance_sh: the radiance field at each probe of an (N, 4) batch (make_probes: position and an ignored word) as 9 L2
        spherical-harmonic coefficients per colour channel, from `samples` (1 .. PATH_MAX_SAMPLES) paths along uniformly drawn
        directions -> (N, 28) float32 rt_sh9 records (split_sh: sh (N, 9, 3), segments), same kind and device as `probes`.  Sample k of
        probe i draws its direction and its path from rng_for(seed + i, first_sample + k): it is radiance() along that direction with
        camera_draws=True, projected in sample order.  max_bounces and shadows as radiance()."""
        n = _check_batch(probes, "probes", 4, "float32")
        pp = _path_params(samples, max_bounces, seed, first_sample, (0 if shadows else PATH_NO_SHADOWS) | (QUERY_COUNTERS if counters else 0))
        out = _out_like(out, probes, "probes", n, 28)
        _sync_torch(probes, out)
        self._check(self.lib.rt_radiance_sh(self._h, _addr(probes), C.c_size_t(n), _p(pp), _addr(out)))
        return out

    def irradiance(self, points, samples, max_bounces=4, seed=0, first_sample=0, shadows=True, out=None, counters=False):
        """rt_irradiance: the cosine-weighted irradiance at each record of an (N, 8) batch of surface points (surface()), from `samples`
        (1 .. PATH_MAX_SAMPLES) paths along directions of the cosine lobe around the record's normal -> (N, 4) float32
        rt_irradiance_result records (split_irradiance: irradiance, segments), same kind and device as `points`.  The normal is used as
        given: surface()'s face-forwarded one gathers on the side the ray arrived on; a miss record is no point and gives zeros.  Sample
        k of point i draws its direction and its path from rng_for(seed + i, first_sample + k): it is radiance() along that direction
        from position + normal * 1e-3 with camera_draws=True, summed in sample order and scaled by pi / samples.  max_bounces and
        shadows as radiance()."""
        n = _check_batch(points, "points", 8, "float32")
        pp = _path_params(samples, max_bounces, seed, first_sample, (0 if shadows else PATH_NO_SHADOWS) | (QUERY_COUNTERS if counters else 0))
        out = _out_like(out, points, "points", n, 4)
        _sync_torch(points, out)
        self._check(self.lib.rt_irradiance(self._h, _addr(points), C.c_size_t(n), _p(pp), _addr(out)))
        return out

    def closest_point(self, points, out=None, counters=False):
        """rt_closest_point: the nearest point of the scene's surface to each record of an (N, 4) batch of points (make_points:
        position, radius) -> (N, 8) float32 rt_nearest records (split_nearest: position, distance, u, v, prim_id, material_id), same
        kind and device as `points`.  Only surface strictly nearer than the radius is reported; a miss is position 0, the radius as
        distance and prim_id = PRIM_MISS."""
        return self._query("rt_closest_point", points, out, 8, "float32", counters, in_cols=4, in_name="points")

    def closest_point_all(self, points, max_nearest, out=None, counts=None, count_all=False, counters=False):
        """rt_closest_point_all: the max_nearest (0 .. NEAREST_MAX) nearest primitives within the radius of each record of an (N, 4)
        batch of points (make_points), nearest first as rt_closest_point would pick them -> (out, counts), same kind and device as
        `points`.  out: (N, max_nearest, 8) float32 rt_nearest records, unused slots miss records (split_nearest takes
        out.reshape(-1, 8)), None for max_nearest=0; counts: (N,) uint32 (numpy) / int32 (torch), the records listed per point, or with
        count_all every primitive within the radius (with an infinite radius that tests the whole scene for every point).
        max_nearest=0 needs count_all: a pure count."""
        n = _check_batch(points, "points", 4, "float32")
        if isinstance(max_nearest, bool) or not isinstance(max_nearest, (int, np.integer)) or not 0 <= max_nearest <= NEAREST_MAX:
            raise ValueError(f"max_nearest: {max_nearest!r}, expected an integer in 0 .. {NEAREST_MAX}")
        max_nearest = int(max_nearest)
        if max_nearest == 0 and not count_all:
            raise ValueError("max_nearest: 0 lists nothing, which needs count_all=True (a pure count)")
        if out is not None and _is_torch(out) != _is_torch(points):
            raise TypeError("out: must be the same kind (numpy / torch) as points")
        if max_nearest == 0:
            out = None
        elif out is None:
            out = _empty_like_batch(points, (n, max_nearest, 8), "float32")
        else:
            _check_nearest_lists(out, n, max_nearest)
        counts = _counts_like(counts, points, "points", n)
        _sync_torch(points, out, counts)
        flags = (QUERY_COUNTERS if counters else 0) | (QUERY_COUNT_ALL if count_all else 0)
        self._check(self.lib.rt_closest_point_all(self._h, _addr(points), C.c_size_t(n), C.c_uint32(max_nearest),
                                                  _addr(out) if out is not None else C.c_void_p(0), _addr(counts), C.c_uint32(flags)))
        return out, counts

    def _inside_query(self, fn, points, rays, out, cols, dtype_name, votes, counters):
        n = _check_batch(points, "points", 4, "float32")
        ip = _inside_params(rays, counters)
        out = _out_like(out, points, "points", n, cols, dtype_name)
        v = _votes_like(votes, points, n)
        _sync_torch(points, out, v)
        self._check(getattr(self.lib, fn)(self._h, _addr(points), C.c_size_t(n), _p(ip), _addr(out), _addr(v) if v is not None else C.c_void_p(0)))
        return out if v is None else (out, v)

    def inside(self, points, rays=3, out=None, votes=False, counters=False):
        """rt_inside: whether each record of an (N, 4) batch of points (make_points; the radius is ignored) lies inside the scene's
        solids -> (N,) bool, same kind and device as `points`: inside some sphere, or a majority of `rays` (1, 3, 5 or 7) crossing
        parities along the fixed INSIDE_DIRECTIONS is odd.  The triangles must form a watertight surface.  votes=True (or an (N,) uint8
        array to fill) -> (inside, votes), votes the odd parities of all `rays` rays: strictly between 0 and `rays` where the rays
        disagree.  Without votes a point stops at its majority (stats()["rays"] tells how many rays that took)."""
        return self._inside_query("rt_inside", points, rays, out, 0, "bool", votes, counters)

    def signed_distance(self, points, rays=3, out=None, votes=False, counters=False):
        """rt_signed_distance: closest_point's (N, 8) float32 records of an (N, 4) batch of points (make_points), the distance negative
        where inside() holds -> records (split_nearest), same kind and device as `points`; on a miss within a finite radius the
        distance is -radius inside, +radius outside (a truncated field).  rays, votes: as inside() -> (records, votes)."""
        return self._inside_query("rt_signed_distance", points, rays, out, 8, "float32", votes, counters)

    def overlap_box(self, boxes, max_prims, *, out=None, counts=None, count_all=False, any_hit=False, counters=False):
        """rt_overlap_box: the primitives that touch each closed axis-aligned box of an (N, 8) batch (make_boxes: centre, half extent)
        -> (prims, counts), same kind and device as `boxes`.  prims: (N, max_prims) ids as split_hits gives prim, uint32 (numpy) /
        int32 (torch, the same bits), the max_prims (0 .. OVERLAP_MAX) touching primitives of lowest key - spheres by index, then
        triangles by index - ascending, unused slots PRIM_MISS; None for max_prims=0.  counts: (N,) uint32 / int32, the ids listed per
        box; with count_all every touching primitive; with any_hit 1 where anything touches the box, else 0 (the walk stops at the
        first).  max_prims=0 needs count_all or any_hit; any_hit needs max_prims=0 and excludes count_all."""
        return self._overlap("rt_overlap_box", boxes, 8, max_prims, out, counts, count_all, any_hit, counters)

    def overlap_obb(self, boxes, max_prims, *, out=None, counts=None, count_all=False, any_hit=False, counters=False):
        """rt_overlap_obb: overlap_box for the closed oriented boxes of an (N, 12) batch (make_obbs: centre, half extent, rotation
        quaternion x y z w, which need not be normalised) -> (prims, counts) exactly as overlap_box gives them.  With the rotation
        (0, 0, 0, 1) the answer is overlap_box's."""
        return self._overlap("rt_overlap_obb", boxes, 12, max_prims, out, counts, count_all, any_hit, counters)

    def overlap_triangle(self, triangles, max_prims, *, out=None, counts=None, count_all=False, any_hit=False, counters=False):
        """rt_overlap_triangle: the primitives that touch each closed triangle of an (N, 12) batch (make_triangles: three vertices; a
        segment or a point is allowed, a non-finite vertex touches nothing) -> (prims, counts) exactly as overlap_box gives them.  A
        sphere is its surface: a triangle wholly inside the ball does not touch it.  A query that is one of the scene's own triangles
        lists that triangle and its neighbours."""
        return self._overlap("rt_overlap_triangle", triangles, 12, max_prims, out, counts, count_all, any_hit, counters, name="triangles")

    def _overlap(self, fn, boxes, cols, max_prims, out, counts, count_all, any_hit, counters, name="boxes"):
        """The call every overlap query makes: `boxes` is its (N, cols) batch, `name` what the messages call it."""
        n = _check_batch(boxes, name, cols, "float32")
        if isinstance(max_prims, bool) or not isinstance(max_prims, (int, np.integer)) or not 0 <= max_prims <= OVERLAP_MAX:
            raise ValueError(f"max_prims: {max_prims!r}, expected an integer in 0 .. {OVERLAP_MAX}")
        max_prims = int(max_prims)
        if any_hit and (count_all or max_prims > 0):
            raise ValueError("any_hit: lists nothing and counts to one, which needs max_prims=0 and excludes count_all")
        if max_prims == 0 and not (count_all or any_hit):
            raise ValueError("max_prims: 0 lists nothing, which needs count_all=True (a pure count) or any_hit=True")
        if out is not None and _is_torch(out) != _is_torch(boxes):
            raise TypeError(f"out: must be the same kind (numpy / torch) as {name}")
        if max_prims == 0:
            out = None
        elif out is None:
            if _is_torch(boxes):
                import torch
                out = torch.empty((n, max_prims), dtype=torch.int32, device=boxes.device)
            else:
                out = np.empty((n, max_prims), np.uint32)
        else:
            _check_prim_lists(out, n, max_prims, name)
        counts = _counts_like(counts, boxes, name, n)
        _sync_torch(boxes, out, counts)
        flags = (QUERY_COUNTERS if counters else 0) | (QUERY_COUNT_ALL if count_all else 0) | (OVERLAP_ANY if any_hit else 0)
        self._check(getattr(self.lib, fn)(self._h, _addr(boxes), C.c_size_t(n), C.c_uint32(max_prims),
                                          _addr(out) if out is not None else C.c_void_p(0), _addr(counts), C.c_uint32(flags)))
        return out, counts

    def contact_capsule(self, capsules, max_contacts, *, out=None, counts=None, count_all=False, any_hit=False, counters=False):
        """rt_contact_capsule: the primitives each resting capsule of an (N, 8) batch (make_capsules: origin, radius, axis) touches ->
        (out, counts), same kind and device as `capsules`.  out: (N, max_contacts, 8) float32 rt_contact records (split_contacts takes
        out.reshape(-1, 8): position, distance, s, prim_id, material_id), the max_contacts (0 .. CONTACT_MAX) nearest primitives whose
        distance from the axis segment is strictly below the radius, nearest first, unused slots miss records; None for
        max_contacts=0.  counts: (N,) uint32 (numpy) / int32 (torch), the records listed per capsule; with count_all every primitive
        in range; with any_hit 1 where anything is in range, else 0 (the walk stops at the first: the occupancy test).
        max_contacts=0 needs count_all or any_hit; any_hit needs max_contacts=0 and excludes count_all.  With a zero axis the
        records are closest_point_all's with s = 0 where u is."""
        return self._contact_query("rt_contact_capsule", capsules, "capsules", 8, max_contacts, out, counts, count_all, any_hit, counters)

    def contact_triangle(self, tris, max_contacts, out=None, counts=None, count_all=False, any_hit=False, counters=False):
        """rt_contact_triangle: the primitives near each resting triangle of an (N, 12) batch (make_contact_triangles: three vertices
        and a margin) -> (out, counts), same kind and device as `tris`.  out: (N, max_contacts, 8) float32 rt_triangle_contact records
        (split_triangle_contacts takes out.reshape(-1, 8): position, distance, qu, qv, prim_id, material_id), the max_contacts (0 ..
        CONTACT_MAX) nearest primitives whose distance from the triangle is strictly below its margin, nearest first, unused slots
        miss records; None for max_contacts=0.  position is the primitive's point, (qu, qv) the weights of the triangle's own v1 and
        v2 at its point of the closest pair; two triangles that intersect are at distance 0.  counts, count_all and any_hit as for
        contact_capsule.  With three equal vertices the records are closest_point_all's with qu = qv = 0."""
        return self._contact_query("rt_contact_triangle", tris, "tris", 12, max_contacts, out, counts, count_all, any_hit, counters)

    def _contact_query(self, fn, batch, in_name, in_cols, max_contacts, out, counts, count_all, any_hit, counters):
        """contact_capsule and contact_triangle: the checks, the outputs and the call."""
        n = _check_batch(batch, in_name, in_cols, "float32")
        if isinstance(max_contacts, bool) or not isinstance(max_contacts, (int, np.integer)) or not 0 <= max_contacts <= CONTACT_MAX:
            raise ValueError(f"max_contacts: {max_contacts!r}, expected an integer in 0 .. {CONTACT_MAX}")
        max_contacts = int(max_contacts)
        if any_hit and (count_all or max_contacts > 0):
            raise ValueError("any_hit: lists nothing and counts to one, which needs max_contacts=0 and excludes count_all")
        if max_contacts == 0 and not (count_all or any_hit):
            raise ValueError("max_contacts: 0 lists nothing, which needs count_all=True (a pure count) or any_hit=True")
        if out is not None and _is_torch(out) != _is_torch(batch):
            raise TypeError(f"out: must be the same kind (numpy / torch) as {in_name}")
        if max_contacts == 0:
            out = None
        elif out is None:
            out = _empty_like_batch(batch, (n, max_contacts, 8), "float32")
        else:
            _check_contact_lists(out, n, max_contacts, in_name)
        counts = _counts_like(counts, batch, in_name, n)
        _sync_torch(batch, out, counts)
        flags = (QUERY_COUNTERS if counters else 0) | (QUERY_COUNT_ALL if count_all else 0) | (CONTACT_ANY if any_hit else 0)
        self._check(getattr(self.lib, fn)(self._h, _addr(batch), C.c_size_t(n), C.c_uint32(max_contacts),
                                          _addr(out) if out is not None else C.c_void_p(0), _addr(counts), C.c_uint32(flags)))
        return out, counts

    def sweep_sphere(self, sweeps, out=None, counters=False):
        """rt_sweep_sphere: the first contact of each moving sphere of an (N, 8) batch (make_sweeps: origin, radius, direction, tmax)
        with the scene's surface -> (N, 8) float32 rt_sweep_hit records (split_sweep_hits: position, t, u, v, prim_id, material_id),
        same kind and device as `sweeps`.  Only contacts at 0 <= t < tmax are reported; a miss is position 0, tmax as t and
        prim_id = PRIM_MISS.  The contact normal is origin + direction * t - position."""
        return self._query("rt_sweep_sphere", sweeps, out, 8, "float32", counters, in_name="sweeps")

    def sweep_box(self, sweeps, out=None, counters=False):
        """rt_sweep_box: the first contact of each moving axis-aligned box of an (N, 12) batch (make_box_sweeps: centre, half extent,
        direction, tmax) with the scene's surface -> (N, 8) float32 rt_box_sweep_hit records (split_box_sweep_hits: normal, t, axis,
        prim_id, material_id), same kind and device as `sweeps`.  Only contacts at 0 <= t < tmax are reported; a miss is normal 0,
        tmax as t, axis SWEEP_AXIS_NONE and prim_id = PRIM_MISS; a start in contact is t = 0 with normal 0 and SWEEP_AXIS_NONE."""
        return self._query("rt_sweep_box", sweeps, out, 8, "float32", counters, in_cols=12, in_name="sweeps")

    def sweep_obb(self, sweeps, out=None, counters=False):
        """rt_sweep_obb: sweep_box for the moving oriented boxes of an (N, 16) batch (make_obb_sweeps: centre, half extent, rotation,
        direction, tmax) -> (N, 8) float32 rt_box_sweep_hit records (split_box_sweep_hits), same kind and device as `sweeps`.  The
        normal is in world space, `axis` is read in the box's frame; misses and starts in contact as sweep_box reports them.  With the
        rotation (0, 0, 0, 1) the answer is sweep_box's."""
        return self._query("rt_sweep_obb", sweeps, out, 8, "float32", counters, in_cols=16, in_name="sweeps")

    def sweep_triangle(self, sweeps, out=None, counters=False):
        """rt_sweep_triangle: the first contact of each moving triangle of an (N, 16) batch (make_triangle_sweeps: three vertices,
        direction, tmax) with the scene -> (N, 8) float32 records, normal nx ny nz | t | axis | 0 | prim_id | material_id
        (split_triangle_sweep_hits).  axis numbers the separating axis that closed last (0 - 2 the coordinate axes, 3 the scene
        triangle's normal, 4 the moving triangle's, 5 - 13 the edge pairs, 14 - 25 the in-plane axes of coplanar and segment pairs),
        SWEEP_TRIANGLE_AXIS_SPHERE for a sphere; a miss has normal 0, tmax as t, SWEEP_AXIS_NONE and prim_id = PRIM_MISS; a start in
        contact - exactly where overlap_triangle lists something - is t = 0 with normal 0 and SWEEP_AXIS_NONE."""
        return self._query("rt_sweep_triangle", sweeps, out, 8, "float32", counters, in_cols=16, in_name="sweeps")

    def _posed_mesh(self, mesh, batch, cols, name):
        """What overlap_mesh and sweep_mesh check of their inputs: (m, n)."""
        m = _check_batch(mesh, "mesh", 12, "float32")
        n = _check_batch(batch, name, cols, "float32")
        if not 1 <= m <= POSED_MESH_MAX:
            raise ValueError(f"mesh: {m} triangles, expected 1 .. {POSED_MESH_MAX}")
        return m, n

    def overlap_mesh(self, mesh, poses, *, first=False, any_hit=False, counters=False):
        """rt_overlap_mesh: the (M, 12) mesh (make_triangles, 1 .. POSED_MESH_MAX triangles), given once, at each pose of an (N, 8)
        batch (make_poses) -> pairs, or (pairs, first) with first=True; (N,) uint32 (numpy) / int32 (torch, the same bits), same kind
        and device as `poses`.  pairs: the number of (mesh triangle, primitive) pairs that touch - the sum of overlap_triangle's
        count_all counts over pose_triangles(mesh, poses)[i], at most 0xFFFFFFFF; first: the lowest mesh triangle that touches
        anything, PRIM_MISS if none.  any_hit: pairs is 1 where anything touches, else 0, and a pose stops at its first touch;
        it excludes first.  An invalid pose (non-finite position or rotation, a zero quaternion) touches nothing.  mesh, poses and
        the results are all host or all device memory of one device."""
        m, n = self._posed_mesh(mesh, poses, 8, "poses")
        if any_hit and first:
            raise ValueError("first: any_hit may stop at any touching triangle, which excludes first")
        pairs = _counts_like(None, poses, "poses", n)
        low = _counts_like(None, poses, "poses", n) if first else None
        _sync_torch(mesh, poses, pairs, low)
        flags = (QUERY_COUNTERS if counters else 0) | (OVERLAP_ANY if any_hit else 0)
        self._check(self.lib.rt_overlap_mesh(self._h, _addr(mesh), C.c_size_t(m), _addr(poses), C.c_size_t(n), _addr(pairs),
                                             _addr(low) if low is not None else C.c_void_p(0), C.c_uint32(flags)))
        return (pairs, low) if first else pairs

    def sweep_mesh(self, mesh, sweeps, out=None, counters=False):
        """rt_sweep_mesh: the first contact of the (M, 12) mesh (make_triangles, 1 .. POSED_MESH_MAX triangles), given once, posed
        and moved by each record of an (N, 12) batch (make_pose_sweeps: position, rotation, world direction, tmax) -> (N, 8) float32
        rt_mesh_sweep_hit records, normal nx ny nz | t | axis | triangle | prim_id | material_id (split_mesh_sweep_hits), same kind
        and device as `sweeps`: sweep_triangle's record of the posed triangle pose_triangles(mesh, sweeps)[i, triangle] that touches
        first - at equal t the lowest scene key, then the lowest mesh triangle.  A miss, and an invalid pose, has normal 0, tmax as
        t, SWEEP_AXIS_NONE and triangle = prim_id = PRIM_MISS."""
        m, n = self._posed_mesh(mesh, sweeps, 12, "sweeps")
        out = _out_like(out, sweeps, "sweeps", n, 8, "float32")
        _sync_torch(mesh, sweeps, out)
        self._check(self.lib.rt_sweep_mesh(self._h, _addr(mesh), C.c_size_t(m), _addr(sweeps), C.c_size_t(n), _addr(out),
                                           C.c_uint32(QUERY_COUNTERS if counters else 0)))
        return out

    def sweep_capsule(self, sweeps, out=None, counters=False):
        """rt_sweep_capsule: the first contact of each moving capsule of an (N, 12) batch (make_capsule_sweeps: origin, radius, axis,
        direction, tmax) with the scene's surface -> (N, 8) float32 rt_capsule_sweep_hit records (split_capsule_sweep_hits: position,
        t, s, prim_id, material_id), same kind and device as `sweeps`.  Only contacts at 0 <= t < tmax are reported; a miss is position
        0, tmax as t, s = 0 and prim_id = PRIM_MISS; with a zero axis the records are sweep_sphere's with s where u is."""
        return self._query("rt_sweep_capsule", sweeps, out, 8, "float32", counters, in_cols=12, in_name="sweeps")

    def camera_rays(self, width, height, camera, mode=MODE_LEGACY, out=None):
        """rt_camera_rays: the width x height pixel-centre rays of mode 0/1 as a (width * height, 8) batch, row-major, y down.
        `out` (optional): a numpy array or torch tensor (CPU or device) to write them to."""
        cam = np.zeros((), T.CAMERA)
        cam[...] = camera
        n = width * height
        if out is None:
            out = np.empty((n, 8), np.float32)
        elif _check_batch(out, "out", 8, "float32") != n:
            raise ValueError(f"out: {len(out)} rows for {n} pixels")
        _sync_torch(out)
        self._check(self.lib.rt_camera_rays(self._h, _p(cam), C.c_uint32(width), C.c_uint32(height), C.c_uint32(mode), _addr(out)))
        return out

    # -- feature buffers and denoising -----------------------------------------------------------------------------------
    def aovs(self, width, height, camera, out=None, **render_kw):
        """rt_aovs: the first-hit albedo, depth, normal and coverage of the frame the same arguments give Context.render (its keyword
        arguments: mode, spp, frame_seed, tile_*, accumulate, ...) -> (height, width, 8) float32 records (split_aovs; a numpy array
        views as types.AOV).  `out` (optional): a numpy array or torch tensor (CPU or device) of that shape to write them to."""
        p = render_params(width, height, camera, **render_kw)
        if out is None:
            out = np.empty((height, width, 8), np.float32)
        else:
            _check_image(out, "out", height, width, 8)
        _sync_torch(out)
        self._check(self.lib.rt_aovs(self._h, _p(p), _addr(out)))
        return out

    def sample_rays(self, width, height, camera, sample, out=None, **render_kw):
        """rt_sample_rays: the extended mode's camera rays of global sample `sample` of the frame the arguments describe (mode=2 is
        implied; spp and accumulate decide the jitter as in a frame) as a (width * height, 8) batch for intersect()."""
        render_kw.setdefault("mode", MODE_EXTENDED)
        p = render_params(width, height, camera, **render_kw)
        n = width * height
        if out is None:
            out = np.empty((n, 8), np.float32)
        elif _check_batch(out, "out", 8, "float32") != n:
            raise ValueError(f"out: {len(out)} rows for {n} pixels")
        _sync_torch(out)
        self._check(self.lib.rt_sample_rays(self._h, _p(p), C.c_uint32(sample), _addr(out)))
        return out

    def denoise(self, rgb, aovs, out=None, iterations=DENOISE_DEFAULTS["iterations"], sigma_color=DENOISE_DEFAULTS["sigma_color"],
                sigma_normal=DENOISE_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"],
                sigma_albedo=DENOISE_DEFAULTS["sigma_albedo"], demodulate=True):
        """rt_denoise: the edge-avoiding a-trous filter of an (h, w, 3) float32 image guided by its (h, w, 8) AOV records (aovs()).
        Both numpy, or both torch tensors on the CPU or on one device of the context; the result (`out`, or a new array of the same
        kind and device) is (h, w, 3).  out may be rgb (in place)."""
        if _is_torch(rgb) != _is_torch(aovs):
            raise TypeError("aovs: must be the same kind (numpy / torch) as rgb")
        h, w = (tuple(getattr(rgb, "shape", ())) + (0, 0))[:2]
        _check_image(rgb, "rgb", h, w, 3)
        _check_image(aovs, "aovs", h, w, 8)
        if out is None:
            out = _empty_like_batch(rgb, (h, w, 3), "float32")
        else:
            if _is_torch(out) != _is_torch(rgb):
                raise TypeError("out: must be the same kind (numpy / torch) as rgb")
            _check_image(out, "out", h, w, 3)
        dp = np.zeros((), dtype=T.DENOISE_PARAMS)
        dp["width"], dp["height"], dp["iterations"] = w, h, iterations
        dp["flags"] = DENOISE_DEMODULATE if demodulate else 0
        dp["sigma_color"], dp["sigma_normal"], dp["sigma_depth"], dp["sigma_albedo"] = sigma_color, sigma_normal, sigma_depth, sigma_albedo
        _sync_torch(rgb, aovs, out)
        self._check(self.lib.rt_denoise(self._h, _p(dp), _addr(rgb), _addr(aovs), _addr(out)))
        return out

    def stats(self):
        st = np.zeros((), dtype=T.STATS)
        self._check(self.lib.rt_get_stats(self._h, _p(st)))
        return {k: st[k].item() for k in st.dtype.names if not k.startswith("_")}


def version():
    return load().rt_version().decode()
