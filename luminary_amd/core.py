"""ctypes binding of the low-level core C ABI (include/lum_core.h): context, scene upload, wavefront passes, counters."""
import ctypes as C

import numpy as np

from . import DeviceSceneView, _lib

DIRTY_CONSTANTS, DIRTY_MATERIALS, DIRTY_INSTANCES, DIRTY_LIGHTS, DIRTY_MESHES, DIRTY_TEXTURES, DIRTY_PARTICLES, DIRTY_ALL = 1, 2, 4, 8, 16, 32, 64, 127
DIRTY_MESH_POSITIONS = 128  # moved vertices: refit (not part of DIRTY_ALL, which builds)
DIRTY_INSTANCE_TRANSFORMS = 256  # moved instances: the top level is rebuilt on the device, the mesh trees stay (not part of DIRTY_ALL)
DIRTY_MESH_SKIN = 512  # bound meshes posed (Core.mesh_skin_pose): their vertices are written on the device, then they are refitted (not part of DIRTY_ALL)
DIRTY_LIGHT_POSITIONS = 1024  # emissive triangles moved: the bound light tree is refitted on the device (Core.light_refit_bind; not part of DIRTY_ALL)
DIRTY_MESH_SHUTTER = 2048  # meshes that hold both shutter keys got a time (Core.shutter_time): a HIP kernel writes them between their keys (not part of DIRTY_ALL)
BVH_BUILDERS = {"sah": 0, "lbvh": 1, "ploc": 2, "sah_gpu": 3}
CNT_TRACE, CNT_SHADOW, CNT_LIGHT_BVH, CNT_VERTICES, CNT_NODES, CNT_TRIS, CNT_NODES_SHADOW, CNT_TRIS_SHADOW, CNT_NODES_LIGHT, CNT_TRIS_LIGHT, CNT_NODES_LDS, CNT_NODES_LDS_SHADOW, CNT_AMBIENT_DEFERRED, CNT_AMBIENT_FALLBACK = range(14)
CNT_COUNT = 16  # LUMC_CNT_COUNT
KERNELS = ("generate", "trace", "shade", "shadow", "accumulate", "light_query", "resolve", "output", "sky", "sort", "volume", "matte")
FIRST_HIT_GUIDES, FIRST_HIT_MATTES = 1, 2  # LUMC_FIRST_HIT_*
FIRST_HIT_OWNER = 4  # the image history's owner plane, with FIRST_HIT_GUIDES (lumc_set_history_motion)
HISTORY_MOTION_SAME, HISTORY_MOTION_MOVED, HISTORY_MOTION_VOID = 0, 1, 2  # LUMC_HISTORY_MOTION_*
MATTE_INSTANCE, MATTE_MATERIAL = 1, 2  # LUMC_MATTE_*: layers
MATTE_ID_EMPTY, MATTE_ID_MISS, MATTE_ID_OCEAN, MATTE_ID_PARTICLE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
MATTE_SLOTS, MATTE_MAX_MASK_IDS = 8, 16


class CoreError(RuntimeError):
    pass


class OutputParams(C.Structure):
    """include/lum_core.h LumOutputParams == oracle/oracle.h OracleOutputParamsAbi."""
    _fields_ = [("src_width", C.c_uint32), ("src_height", C.c_uint32), ("dst_width", C.c_uint32), ("dst_height", C.c_uint32),
                ("inv_sample_count", C.c_float), ("exposure", C.c_float), ("tonemap", C.c_uint32), ("filter", C.c_uint32), ("dithering", C.c_uint32),
                ("purkinje", C.c_uint32), ("use_color_correction", C.c_uint32), ("passthrough", C.c_uint32), ("purkinje_kappa1", C.c_float),
                ("purkinje_kappa2", C.c_float), ("cc_h", C.c_float), ("cc_s", C.c_float), ("cc_v", C.c_float), ("film_grain", C.c_float),
                ("agx_slope", C.c_float), ("agx_power", C.c_float), ("agx_saturation", C.c_float), ("supersampling", C.c_uint32),
                ("undersampling_stage", C.c_uint32)]

    def output_planes_shape(self):
        """Shape of the display-referred planes the chain keeps: the frame >> max(undersampling stage, supersampling)."""
        uo = max(self.undersampling_stage, self.supersampling)
        return (3, self.src_height >> uo, self.src_width >> uo)


def default_output_params(width, height, sample_count, dst=None, supersampling=0, undersampling_stage=0):
    """Camera defaults of the reference (camera.c:7-66): AgX, dithering and Purkinje shift on, exposure exp(0). `width`, `height`: the
    rendered frame (output size << supersampling); `dst` defaults to the nominal output size."""
    p = OutputParams()
    p.src_width, p.src_height = width, height
    p.supersampling, p.undersampling_stage = supersampling, undersampling_stage
    p.dst_width, p.dst_height = dst if dst else (width >> supersampling, height >> supersampling)
    p.inv_sample_count = np.float32(1.0) / np.float32(sample_count)
    p.exposure = 1.0
    p.tonemap, p.filter, p.dithering, p.purkinje = 4, 0, 1, 1
    p.purkinje_kappa1, p.purkinje_kappa2 = 0.2, 0.29
    p.agx_slope = p.agx_power = p.agx_saturation = 1.0
    return p


class AdaptiveParams(C.Structure):
    """include/lum_core.h LumAdaptiveParams."""
    _fields_ = [("max_sampling_rate", C.c_uint32), ("avg_sampling_rate", C.c_uint32), ("update_interval", C.c_uint32), ("exposure", C.c_float),
                ("tone", OutputParams)]


class AdaptiveInfo(C.Structure):
    """include/lum_core.h LumAdaptiveInfo."""
    _fields_ = [("stage_id", C.c_uint32), ("executions", C.c_uint32 * 5), ("num_blocks", C.c_uint32), ("blocks_x", C.c_uint32), ("blocks_y", C.c_uint32),
                ("tasks_per_execution", C.c_uint32), ("variance_total", C.c_float), ("build_pending", C.c_uint32)]


LENS_MAX_INTERFACES = 24  # LUMC_LENS_MAX_INTERFACES


class LensInterface(C.Structure):
    _fields_ = [("radius", C.c_float), ("vertex", C.c_float), ("cylindrical_radius", C.c_float)]


class LensMedium(C.Structure):
    _fields_ = [("design_ior", C.c_float), ("abbe", C.c_float), ("cylindrical_radius", C.c_float)]


class PhysicalCamera(C.Structure):
    """include/lum_core.h LumPhysicalCamera: the converted physical camera (radii, mm) and its lens."""
    _fields_ = [(n, C.c_float) for n in ("aperture_point", "aperture_radius", "exit_pupil_point", "exit_pupil_radius", "image_plane_distance",
                                          "sensor_width")] + \
               [("allow_reflections", C.c_uint32), ("num_interfaces", C.c_uint32), ("interfaces", LensInterface * LENS_MAX_INTERFACES),
                ("media", LensMedium * (LENS_MAX_INTERFACES + 1))]


class DenoiseParams(C.Structure):
    """include/lum_core.h LumDenoiseParams"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("uniform_samples", C.c_uint32)]


def default_denoise_params(uniform_samples=0, **fields):
    p = DenoiseParams()
    _lib().lumc_denoise_default_params(C.byref(p))
    p.uniform_samples = uniform_samples
    for k, v in fields.items():
        setattr(p, k, v)
    return p


class MeshRefitStats(C.Structure):
    """LumMeshRefitStats"""
    _fields_ = [("refits", C.c_uint64), ("rebuilds", C.c_uint64), ("last_refits", C.c_uint32), ("last_rebuilds", C.c_uint32), ("max_cost_growth", C.c_double),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_refit", C.c_double), ("seconds_rebuild", C.c_double), ("seconds_assemble", C.c_double),
                ("seconds_hash", C.c_double), ("seconds_download", C.c_double), ("seconds_lights", C.c_double)]


class InstanceUpdateStats(C.Structure):
    """LumInstanceUpdateStats"""
    _fields_ = [("device_updates", C.c_uint64), ("fallbacks", C.c_uint64), ("relayouts", C.c_uint64), ("tlas_nodes", C.c_uint32), ("tlas_depth", C.c_uint32),
                ("tlas_capacity", C.c_uint32), ("hittable", C.c_uint32), ("seconds", C.c_double), ("seconds_relayout", C.c_double), ("seconds_upload", C.c_double),
                ("seconds_boxes", C.c_double), ("seconds_build", C.c_double), ("seconds_leaves", C.c_double)]


class ResidentRefitStats(C.Structure):
    """LumResidentRefitStats"""
    _fields_ = [("updates", C.c_uint64), ("fallbacks", C.c_uint64), ("last_meshes", C.c_uint32), ("last_launches", C.c_uint32), ("last_bytes_downloaded", C.c_uint64),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_hash", C.c_double), ("seconds_refit", C.c_double), ("seconds_cost", C.c_double),
                ("seconds_top_level", C.c_double)]


class MeshSkinStats(C.Structure):
    """LumMeshSkinStats"""
    _fields_ = [("poses", C.c_uint64), ("rebuild_downloads", C.c_uint64), ("last_meshes", C.c_uint32), ("last_launches", C.c_uint32), ("last_bytes_uploaded", C.c_uint64),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_skin", C.c_double)]


def _skin_arrays(rest_positions, rest_normals, bone_ids, weights):
    p = np.ascontiguousarray(rest_positions, dtype=np.float32).reshape(-1, 9)
    n = np.ascontiguousarray(rest_normals, dtype=np.float32).reshape(-1, 9)
    i = np.ascontiguousarray(bone_ids, dtype=np.uint16).reshape(-1, 12)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 12)
    assert len(p) == len(n) == len(i) == len(w), "9 position floats, 9 normal floats, 12 ids and 12 weights per triangle"
    return p, n, i, w


def skin_host(rest_positions, rest_normals, bone_ids, weights, bones):
    """lumc_skin_host, no device needed: the host twin of the skinning kernel over triangles of rest positions / normals [n, 9], bone ids / weights [n, 12] (four
    slots per corner) and bones [b, 12] (row-major 3 x 4). Returns (positions [n, 9] float32, normals [n, 9] float32, packed normal words [n, 3] uint32)."""
    fn = _lib().lumc_skin_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    p, n, i, w = _skin_arrays(rest_positions, rest_normals, bone_ids, weights)
    b = np.ascontiguousarray(bones, dtype=np.float32).reshape(-1, 12)
    op, on, pk = np.zeros_like(p), np.zeros_like(n), np.zeros((len(p), 3), np.uint32)
    if fn(p.ctypes.data, n.ctypes.data, i.ctypes.data, w.ctypes.data, len(p), b.ctypes.data, len(b), op.ctypes.data, on.ctypes.data, pk.ctypes.data) != 0:
        raise CoreError("lumc_skin_host refused its arguments (bone count 1 ... 1024, ids below it)")
    return op, on, pk


class FireflyStats(C.Structure):
    """LumFireflyStats"""
    _fields_ = [("buckets", C.c_uint32), ("reserved", C.c_uint32), ("bytes", C.c_uint64), ("resolves", C.c_uint64), ("last_rewritten", C.c_uint32),
                ("last_trimmed", C.c_uint32), ("last_nonfinite", C.c_uint32), ("samples", C.c_uint32)]


def firefly_resolve_host(sums, counts, image):
    """lumc_firefly_resolve_host, no device needed: the host twin of the firefly resolve. sums [K, 3, P] float32 bucket sums, counts [K] ids per bucket, image
    [3, P] (or [3, H, W]) the planar result image. Returns (image after the resolve - a copy, same shape -, (pixels rewritten, buckets trimmed, pixels with a
    non-finite bucket)); raises ValueError where the twin refuses (K outside 4 ... 16, counts all zero)."""
    fn = _lib().lumc_firefly_resolve_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    s = np.ascontiguousarray(sums, dtype=np.float32)
    n = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    out = np.ascontiguousarray(image, dtype=np.float32).copy()
    K = len(n)
    pixels = out.size // 3
    if s.ndim < 2 or s.shape[0] != K or s.size != K * 3 * pixels:
        raise ValueError("firefly_resolve_host: sums [K, 3, P], counts [K] and image [3, P] do not fit")
    stats = (C.c_uint32 * 3)()
    if fn(s.ctypes.data, n.ctypes.data, K, pixels, out.ctypes.data, C.addressof(stats)) != 0:
        raise ValueError("lumc_firefly_resolve_host refused its arguments")
    return out, tuple(int(x) for x in stats)


class MatteStats(C.Structure):
    """LumMatteStats"""
    _fields_ = [("samples", C.c_uint32), ("layers", C.c_uint32), ("bytes", C.c_uint64), ("dropped_pixels", C.c_uint32 * 2), ("valid", C.c_uint32),
                ("reserved", C.c_uint32), ("seconds", C.c_double)]


def matte_host(ids, ranks=MATTE_SLOTS):
    """lumc_matte_host, no device needed: the host twin of the matte kernels. ids [samples, pixels] uint32 in ascending sample id, MATTE_ID_EMPTY = the sample has
    no path. Returns a dict: slots_id, slots_count [8, P], ids [ranks, P] uint32, coverage [ranks, P] float32, dropped, rays [P]; raises ValueError where the twin
    refuses (samples outside 1 ... 1024, ranks outside 1 ... 8)."""
    fn = _lib().lumc_matte_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    if a.ndim != 2:
        raise ValueError("matte_host: ids [samples, pixels]")
    S, P = a.shape
    R = max(min(int(ranks), MATTE_SLOTS), 1)
    out = {"slots_id": np.zeros((MATTE_SLOTS, P), np.uint32), "slots_count": np.zeros((MATTE_SLOTS, P), np.uint32), "ids": np.zeros((R, P), np.uint32),
           "coverage": np.zeros((R, P), np.float32), "dropped": np.zeros(P, np.uint32), "rays": np.zeros(P, np.uint32)}
    if fn(a.ctypes.data, S, P, int(ranks), *[out[k].ctypes.data for k in ("slots_id", "slots_count", "ids", "coverage", "dropped", "rays")]) != 0:
        raise ValueError("lumc_matte_host refused its arguments")
    return out


def matte_mask_host_twin(slots_id, slots_count, samples, ids):
    """lumc_matte_mask_host_twin, no device needed: the mask [P] float32 of up to 16 ids over raw slots [8, P]; raises ValueError where the twin refuses."""
    fn = _lib().lumc_matte_mask_host_twin
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    si = np.ascontiguousarray(slots_id, dtype=np.uint32)
    sc = np.ascontiguousarray(slots_count, dtype=np.uint32)
    if si.shape != sc.shape or si.ndim != 2 or si.shape[0] != MATTE_SLOTS:
        raise ValueError("matte_mask_host_twin: slots [8, pixels]")
    want = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    mask = np.zeros(si.shape[1], np.float32)
    if fn(si.ctypes.data, sc.ctypes.data, si.shape[1], int(samples), want.ctypes.data if want.size else None, want.size, mask.ctypes.data) != 0:
        raise ValueError("lumc_matte_mask_host_twin refused its arguments")
    return mask


class HistoryParams(C.Structure):
    """LumHistoryParams"""
    _fields_ = [("enabled", C.c_uint32), ("max_history", C.c_float), ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("clamp_sigma", C.c_float)]


class HistoryKey(C.Structure):
    """LumHistoryKey: the thin-lens camera a frame was shown from, as the scene view holds it"""
    _fields_ = [("pos", C.c_float * 3), ("rotation", C.c_float * 4), ("fov", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32)]


class HistoryStats(C.Structure):
    """LumHistoryStats"""
    _fields_ = [("carries", C.c_uint64), ("blends", C.c_uint64), ("drops", C.c_uint64), ("bytes", C.c_uint64), ("last_carried", C.c_uint32), ("last_rejected", C.c_uint32),
                ("last_off", C.c_uint32), ("has_state", C.c_uint32), ("has_carried", C.c_uint32), ("reserved", C.c_uint32), ("carry_ms", C.c_double), ("blend_ms", C.c_double),
                ("carry_launches", C.c_uint32), ("blend_launches", C.c_uint32), ("dropped_why", C.c_char_p)]


def history_params(enabled=True, max_history=32.0, depth_tolerance=0.02, normal_threshold=0.9, clamp_sigma=0.0):
    return HistoryParams(1 if enabled else 0, max_history, depth_tolerance, normal_threshold, clamp_sigma)


def history_key(pos, rotation, fov, width, height):
    """rotation: the quaternion (x, y, z, w)"""
    return HistoryKey((C.c_float * 3)(*[float(v) for v in pos]), (C.c_float * 4)(*[float(v) for v in rotation]), float(fov), int(width), int(height))


def _f32(a, shape, what):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size != int(np.prod(shape)):
        raise ValueError("%s: %d floats expected" % (what, int(np.prod(shape))))
    return a.reshape(shape)


def history_reproject_host(now_key, old_key, params, normal, depth, old_shown, old_weight, old_normal, old_depth):
    """lumc_history_reproject_host, no device needed: the host twin of k_history_reproject. normal [3, P], depth [P] of now_key's frame; old_* of old_key's.
    Returns (carried [3, P], carried_weight [P], (carried, rejected, off)); raises ValueError where the twin refuses."""
    fn = _lib().lumc_history_reproject_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 12
    P, Q = now_key.width * now_key.height, old_key.width * old_key.height
    ins = [_f32(normal, (3, P), "normal"), _f32(depth, (P,), "depth"), _f32(old_shown, (3, Q), "old_shown"), _f32(old_weight, (Q,), "old_weight"),
           _f32(old_normal, (3, Q), "old_normal"), _f32(old_depth, (Q,), "old_depth")]
    carried, weight = np.zeros((3, P), np.float32), np.zeros(P, np.float32)
    stats = (C.c_uint32 * 3)()
    if fn(C.addressof(now_key), C.addressof(old_key), C.addressof(params), *[a.ctypes.data for a in ins], carried.ctypes.data, weight.ctypes.data, C.addressof(stats)) != 0:
        raise ValueError("lumc_history_reproject_host refused its arguments")
    return carried, weight, tuple(int(x) for x in stats)


def history_blend_host(params, width, height, uniform_samples, image, carried=None, carried_weight=None):
    """lumc_history_blend_host, no device needed: the host twin of k_history_blend. image [3, P] planar (a copy is blended); carried [3, P], carried_weight [P] or
    both None. Returns (image after the blend, shown [3, P], weight [P])."""
    fn = _lib().lumc_history_blend_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
    P = int(width) * int(height)
    out = _f32(image, (3, P), "image").copy()
    c = None if carried is None else _f32(carried, (3, P), "carried")
    w = None if carried_weight is None else _f32(carried_weight, (P,), "carried_weight")
    shown, weight = np.zeros((3, P), np.float32), np.zeros(P, np.float32)
    if fn(C.addressof(params), int(width), int(height), int(uniform_samples), out.ctypes.data, None if c is None else c.ctypes.data, None if w is None else w.ctypes.data,
          shown.ctypes.data, weight.ctypes.data) != 0:
        raise ValueError("lumc_history_blend_host refused its arguments")
    return out, shown, weight


def history_centre_ray_host(key, px, py):
    fn = _lib().lumc_history_centre_ray_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    d = np.zeros(3, np.float32)
    if fn(C.addressof(key), int(px), int(py), d.ctypes.data) != 0:
        raise ValueError("lumc_history_centre_ray_host refused its arguments")
    return d


def history_project_host(key, v):
    """lumc_history_project_host: (fx, fy) of a vector relative to the key's camera, or None where it lies behind it."""
    fn = _lib().lumc_history_project_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 4
    vv = np.ascontiguousarray(v, dtype=np.float32).reshape(3)
    fx, fy = C.c_float(), C.c_float()
    rc = fn(C.addressof(key), vv.ctypes.data, C.addressof(fx), C.addressof(fy))
    if rc == 1:
        raise ValueError("lumc_history_project_host refused its arguments")
    return None if rc == 2 else (np.float32(fx.value), np.float32(fy.value))


class HistoryMotionParams(C.Structure):
    """LumHistoryMotionParams"""
    _fields_ = [("enabled", C.c_uint32), ("motion_max_history", C.c_float)]


class HistoryMotionStats(C.Structure):
    """LumHistoryMotionStats"""
    _fields_ = [("motion_carries", C.c_uint64), ("bytes", C.c_uint64), ("instances_moved", C.c_uint32), ("instances_same", C.c_uint32), ("instances_void", C.c_uint32),
                ("last_moved_pixels", C.c_uint32), ("last_moved_carried", C.c_uint32), ("has_snapshot", C.c_uint32), ("has_owner", C.c_uint32), ("snapshot_instances", C.c_uint32),
                ("owner_ms", C.c_double), ("motion_ms", C.c_double), ("reproject_ms", C.c_double), ("owner_launches", C.c_uint32), ("motion_launches", C.c_uint32),
                ("reproject_launches", C.c_uint32), ("reserved", C.c_uint32)]


# LumHistoryMotionRecord (history.h HistoryMotion), 128 bytes per instance
HISTORY_MOTION_RECORD = np.dtype([("cls", np.uint32), ("t_new", np.float32, 3), ("t_old", np.float32, 3), ("L", np.float32, 9), ("NL", np.float32, 9), ("pad", np.uint32, 7)])


def _u32(a, shape, what):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.size != int(np.prod(shape)):
        raise ValueError("%s: %d words expected" % (what, int(np.prod(shape))))
    return a.reshape(shape)


def history_motion_records_host(old8, new8):
    """lumc_history_motion_records_host, no device needed: the twin of k_history_motion. old8, new8 [count, 8] float32 (the 8 words of each instance's transform as
    the scene view holds them). Returns (records [count] of HISTORY_MOTION_RECORD, (moved, same, void))."""
    fn = _lib().lumc_history_motion_records_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    o, n = np.ascontiguousarray(old8, np.float32).reshape(-1, 8), np.ascontiguousarray(new8, np.float32).reshape(-1, 8)
    if o.shape != n.shape:
        raise ValueError("old8 and new8 differ in shape")
    rec = np.zeros(o.shape[0], HISTORY_MOTION_RECORD)
    stats = (C.c_uint32 * 3)()
    if fn(o.ctypes.data, n.ctypes.data, o.shape[0], rec.ctypes.data, C.addressof(stats)) != 0:
        raise ValueError("lumc_history_motion_records_host refused its arguments")
    return rec, tuple(int(x) for x in stats)


def history_reproject_motion_host(now_key, old_key, params, motion_max_history, normal, depth, old_shown, old_weight, old_normal, old_depth, owner, old_owner, records):
    """lumc_history_reproject_motion_host, no device needed: the twin of k_history_reproject_motion. history_reproject_host's arguments, the cap of moved owners,
    owner [P] and old_owner [Q] (uint32), records [count] of HISTORY_MOTION_RECORD. Returns (carried [3, P], carried_weight [P], (carried, rejected, off, owner
    moved, owner moved and carried))."""
    fn = _lib().lumc_history_reproject_motion_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 9 + [C.c_uint32] + [C.c_void_p] * 3
    P, Q = now_key.width * now_key.height, old_key.width * old_key.height
    ins = [_f32(normal, (3, P), "normal"), _f32(depth, (P,), "depth"), _f32(old_shown, (3, Q), "old_shown"), _f32(old_weight, (Q,), "old_weight"),
           _f32(old_normal, (3, Q), "old_normal"), _f32(old_depth, (Q,), "old_depth"), _u32(owner, (P,), "owner"), _u32(old_owner, (Q,), "old_owner")]
    rec = np.ascontiguousarray(records, HISTORY_MOTION_RECORD).reshape(-1)
    carried, weight = np.zeros((3, P), np.float32), np.zeros(P, np.float32)
    stats = (C.c_uint32 * 5)()
    if fn(C.addressof(now_key), C.addressof(old_key), C.addressof(params), float(motion_max_history), *[a.ctypes.data for a in ins], rec.ctypes.data if rec.size else None, rec.size,
          carried.ctypes.data, weight.ctypes.data, C.addressof(stats)) != 0:
        raise ValueError("lumc_history_reproject_motion_host refused its arguments")
    return carried, weight, tuple(int(x) for x in stats)


class ShutterStats(C.Structure):
    """LumShutterStats"""
    _fields_ = [("slices", C.c_uint64), ("last_meshes", C.c_uint32), ("last_launches", C.c_uint32), ("last_bytes_uploaded", C.c_uint64), ("seconds", C.c_double)]


def shutter_host(open_records, close_records, t):
    """lumc_shutter_host, no device needed: the host twin of the shutter kernel over 16-byte vertex records [n, 4] (float32, or their uint32 words). Returns (records
    [n, 4] uint32, flags); raises ValueError where the twin refuses (a t outside [0, 1] or not finite)."""
    fn = _lib().lumc_shutter_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(open_records).view(np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(close_records).view(np.uint32).reshape(-1, 4)
    if a.shape != b.shape:
        raise ValueError("shutter_host: the keys differ in size")
    out = np.zeros_like(a)
    flags = C.c_uint32(0)
    if fn(a.ctypes.data, b.ctypes.data, len(a), float(t), out.ctypes.data, C.addressof(flags)) != 0:
        raise ValueError("lumc_shutter_host refused its arguments")
    return out, flags.value


class MeshMorphStats(C.Structure):
    """LumMeshMorphStats"""
    _fields_ = [("applied", C.c_uint64), ("rebuild_downloads", C.c_uint64), ("last_meshes", C.c_uint32), ("last_launches", C.c_uint32), ("last_bytes_uploaded", C.c_uint64),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_morph", C.c_double)]


def _morph_arrays(base_positions, base_normals, offsets, corners, delta_positions, delta_normals):
    p = np.ascontiguousarray(base_positions, dtype=np.float32).reshape(-1, 9)
    n = np.ascontiguousarray(base_normals, dtype=np.float32).reshape(-1, 9)
    o = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    c = np.ascontiguousarray(corners, dtype=np.uint32).reshape(-1)
    dp = np.ascontiguousarray(delta_positions, dtype=np.float32).reshape(-1, 3)
    dn = None if delta_normals is None else np.ascontiguousarray(delta_normals, dtype=np.float32).reshape(-1, 3)
    assert len(p) == len(n), "9 position floats and 9 normal floats per triangle"
    assert len(o) >= 2 and len(c) == len(dp) and (dn is None or len(dn) == len(dp)) and int(o.max()) <= len(c), "offsets [T + 1] into corners [E], deltas [E, 3]"
    return p, n, o, c, dp, dn


def _addr(a):
    return C.c_void_p(a.ctypes.data if a is not None and a.size else None)


def morph_host(base_positions, base_normals, offsets, corners, delta_positions, delta_normals, weights, bone_ids=None, skin_weights=None, bones=None):
    """lumc_morph_host, no device needed: the host twin of the morph kernel over triangles of base positions / normals [n, 9], sparse target-major deltas (offsets
    [T + 1] into corners [E], delta positions [E, 3], delta normals [E, 3] or None) and weights [T]; with bones [b, 12] also bone ids / skin weights [n, 12]: the
    combined result. Returns (positions [n, 9] float32, normals [n, 9] float32, packed normal words [n, 3] uint32)."""
    fn = _lib().lumc_morph_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.c_uint32] + [C.c_void_p] * 3
    p, n, o, c, dp, dn = _morph_arrays(base_positions, base_normals, offsets, corners, delta_positions, delta_normals)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    assert len(w) == len(o) - 1, "one weight per target"
    i = sw = b = None
    if bones is not None:
        i = np.ascontiguousarray(bone_ids, dtype=np.uint16).reshape(-1, 12)
        sw = np.ascontiguousarray(skin_weights, dtype=np.float32).reshape(-1, 12)
        b = np.ascontiguousarray(bones, dtype=np.float32).reshape(-1, 12)
        assert len(i) == len(sw) == len(p)
    op, on, pk = np.zeros_like(p), np.zeros_like(n), np.zeros((len(p), 3), np.uint32)
    if fn(p.ctypes.data, n.ctypes.data, len(p), len(w), o.ctypes.data, _addr(c), _addr(dp), _addr(dn), w.ctypes.data, _addr(i), _addr(sw), _addr(b), 0 if b is None else len(b),
          op.ctypes.data, on.ctypes.data, pk.ctypes.data) != 0:
        raise CoreError("lumc_morph_host refused its arguments (1 ... 1024 targets, offsets from 0 that do not decrease, corners of a target strictly increasing and below 3 n, finite deltas and weights)")
    return op, on, pk


class LightRefitPlan(C.Structure):
    """LumLightRefitPlan: what the last build of the light tree left behind for its refit (Host.light_refit_plan). fragments: [n, 8] uint32 words (instance, mesh,
    triangle, light id, transform, intensity and average intensity as float bits, 0); transforms: [t, 10] float32 (q, scale, offset); slots: [128 + 8 nodes, 2]."""
    _fields_ = [("fragments", C.c_void_p), ("transforms", C.c_void_p), ("transform_instances", C.c_void_p), ("slots", C.c_void_p), ("num_fragments", C.c_uint32),
                ("num_transforms", C.c_uint32), ("num_nodes", C.c_uint32), ("reserved", C.c_uint32), ("root_cost", C.c_double)]

    @classmethod
    def from_arrays(cls, fragments, transforms, transform_instances, slots, root_cost):
        """A plan over copies of the arrays (kept alive by the plan)."""
        f = np.ascontiguousarray(fragments, dtype=np.uint32).reshape(-1, 8).copy()
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 10).copy()
        ti = np.ascontiguousarray(transform_instances, dtype=np.uint32).reshape(-1).copy()
        sl = np.ascontiguousarray(slots, dtype=np.uint32).reshape(-1, 2).copy()
        assert len(sl) >= 128 and (len(sl) - 128) % 8 == 0 and len(t) == len(ti)
        plan = cls(f.ctypes.data, t.ctypes.data, ti.ctypes.data, sl.ctypes.data, len(f), len(t), (len(sl) - 128) // 8, 0, float(root_cost))
        plan._keepalive = (f, t, ti, sl)
        return plan

    def arrays(self):
        """Copies: (fragments [n, 8] uint32, transforms [t, 10] float32, transform_instances [t] uint32, slots [128 + 8 nodes, 2] uint32)."""
        def take(ptr, count, dtype, shape):
            if not ptr or not count:
                return np.zeros(shape, dtype)
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()
        n, t, s = self.num_fragments, self.num_transforms, 128 + 8 * self.num_nodes
        return (take(self.fragments, 8 * n, np.uint32, (n, 8)), take(self.transforms, 10 * t, np.float32, (t, 10)), take(self.transform_instances, t, np.uint32, (t,)),
                take(self.slots, 2 * s, np.uint32, (s, 2)))

    def copy(self):
        return LightRefitPlan.from_arrays(*self.arrays(), self.root_cost)


class LightRefitReport(C.Structure):
    """LumLightRefitReport"""
    _fields_ = [("refitted", C.c_uint32), ("flags", C.c_uint32), ("cost", C.c_double), ("cost_growth", C.c_double)]


class LightRefitStats(C.Structure):
    """LumLightRefitStats"""
    _fields_ = [("refits", C.c_uint64), ("fallbacks", C.c_uint64), ("last_launches", C.c_uint32), ("last_flags", C.c_uint32), ("last_bytes_uploaded", C.c_uint64),
                ("last_bytes_downloaded", C.c_uint64), ("seconds", C.c_double), ("seconds_fragments", C.c_double), ("seconds_stats", C.c_double), ("seconds_nodes", C.c_double),
                ("seconds_light_bvh", C.c_double), ("seconds_table", C.c_double), ("cost_growth", C.c_double)]


LIGHT_REFIT_ZERO_AREA, LIGHT_REFIT_NOT_FINITE = 1, 2


def light_refit_host(plan, vertices, mesh_tri_offset, root, root_children, nodes):
    """lumc_light_refit_host, no device needed: the host twin of the light tree's refit kernels - the definition of their bytes. vertices: the view's vertex records
    [corners, 4] (float32, or their uint32 words); root / root_children / nodes: the last build's arrays (copied, not changed). Returns a dict: root, root_children,
    nodes (uint8 / float32 / uint8 [n, 64]), light_bvh_tris [lights, 12] float32, slot_stats [slots, 8] float32, report (LightRefitReport). With report.refitted == 0
    the arrays are the inputs."""
    fn = _lib().lumc_light_refit_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 9
    v = np.ascontiguousarray(vertices)
    assert v.dtype.itemsize == 4 and v.size % 12 == 0
    off = np.ascontiguousarray(mesh_tri_offset, dtype=np.uint32)
    r = np.ascontiguousarray(root, dtype=np.uint8).reshape(-1).copy()
    rc = np.ascontiguousarray(root_children, dtype=np.float32).reshape(-1).copy()
    nd = np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1, 64).copy()
    tris = np.zeros((plan.num_fragments, 12), np.float32)
    stats = np.zeros((128 + 8 * plan.num_nodes, 8), np.float32)
    report = LightRefitReport()
    if fn(C.addressof(plan), v.ctypes.data, off.ctypes.data, _addr(r), _addr(rc), _addr(nd), _addr(tris), stats.ctypes.data, C.addressof(report)) != 0:
        raise CoreError("lumc_light_refit_host refused its arguments")
    return {"root": r, "root_children": rc, "nodes": nd, "light_bvh_tris": tris, "slot_stats": stats, "report": report}


def light_refit_ceil_log2(x):
    """lumc_light_refit_ceil_log2: the exact ceil(log2(x)) of a finite float32 x > 0, as the refit's quantiser takes it."""
    fn = _lib().lumc_light_refit_ceil_log2
    fn.restype = C.c_int
    fn.argtypes = [C.c_float]
    return int(fn(float(np.float32(x))))


def light_root_children(root):
    """The float table of a root's children as an upload makes it (64 floats per section + 16): mean = byte * 2^e + base per axis, sigma = byte * 2^e_sigma, power."""
    root = np.ascontiguousarray(root, dtype=np.uint8).reshape(-1)
    sections = int(root[10])
    base = (root[:6].view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    e = root[12:16].view(np.int8).astype(np.int32)
    table = np.zeros(sections * 64 + 16, np.float32)
    for s in range(sections):
        sec = root[16 + 48 * s:16 + 48 * (s + 1)]
        for c in range(8):
            o = (s * 8 + c) * 8
            for a in range(3):
                table[o + a] = np.float32(np.float32(sec[8 * a + c]) * np.ldexp(np.float32(1), e[a])) + base[a]
            table[o + 3] = np.float32(sec[24 + c]) * np.ldexp(np.float32(1), e[3])
            table[o + 4] = np.float32(sec[32 + 2 * c:34 + 2 * c].view(np.uint16)[0])
    return table


def instance_boxes_probe(view, mesh_boxes, on_gpu=False):
    """lumc_instance_boxes_probe: (rows [n, 3, 4] float32, boxes [n, 6] float32, hittable [n] uint32) of the instances of `view` over the meshes' object-space
    boxes mesh_boxes [num_meshes, 6], by the host's functions or by the device's kernel."""
    fn = _lib().lumc_instance_boxes_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    mb = np.ascontiguousarray(mesh_boxes, dtype=np.float32).reshape(-1, 6)
    assert mb.shape[0] == view.num_meshes
    n = view.num_instances
    rows, boxes, hittable = np.zeros((n, 3, 4), np.float32), np.zeros((n, 6), np.float32), np.zeros(n, np.uint32)
    if fn(C.addressof(view), mb.ctypes.data, int(bool(on_gpu)), rows.ctypes.data, boxes.ctypes.data, hittable.ctypes.data) != 0:
        raise CoreError("lumc_instance_boxes_probe failed")
    return rows, boxes, hittable


def host_bvh_nodes_probe(boxes, max_leaf=1, max_depth=16):
    """lumc_host_bvh_nodes_probe: the host builder's tree over boxes [n, 6]: (nodes [nodes, 32] uint32 words, prims [n] uint32, 4-wide levels)."""
    fn = _lib().lumc_host_bvh_nodes_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    n = b.shape[0]
    sizes = (C.c_uint64 * 3)()
    nodes, prims = np.zeros((max(n, 1), 32), np.uint32), np.zeros(max(n, 1), np.uint32)
    if fn(b.ctypes.data, n, max_leaf, max_depth, sizes, nodes.ctypes.data, prims.ctypes.data) != 0:
        raise CoreError("lumc_host_bvh_nodes_probe failed")
    return nodes[:sizes[0]].copy(), prims[:sizes[1]].copy(), int(sizes[2])


def bvh_refit_probe(built_boxes, refit_boxes, builder="sah", on_gpu=False):
    """lumc_bvh_refit_probe: a tree over built_boxes [n, 6] by `builder`, refitted to refit_boxes [m, 6] on the host or on the device. Returns a dict: built / refit
    (node arrays as [nodes, 32] uint32 words: 24 box floats, 4 child words, 4 of padding; refit None when the tree cannot be refitted), host_refit (the host's refit of
    the same tree), prims, cost (built, refit, host refit), valid."""
    lib = _lib()
    fn = lib.lumc_bvh_refit_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    a = np.ascontiguousarray(built_boxes, dtype=np.float32)
    b = np.ascontiguousarray(refit_boxes, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] == 6 and b.ndim == 2 and b.shape[1] == 6
    n = a.shape[0]
    sizes, cost, valid = (C.c_uint64 * 3)(), (C.c_double * 3)(), C.c_uint64()
    built, refit, host_refit, prims = np.zeros((n, 32), np.uint32), np.zeros((n, 32), np.uint32), np.zeros((n, 32), np.uint32), np.zeros(n, np.uint32)
    if fn(a.ctypes.data, b.ctypes.data, n, b.shape[0], BVH_BUILDERS[builder], int(bool(on_gpu)), sizes, built.ctypes.data, refit.ctypes.data, host_refit.ctypes.data, prims.ctypes.data, cost, C.byref(valid)) != 0:
        raise CoreError("lumc_bvh_refit_probe failed (builder %s)" % builder)
    return {"built": built[:sizes[0]].copy(), "refit": refit[:sizes[2]].copy() if sizes[2] else None, "host_refit": host_refit[:sizes[0]].copy() if b.shape[0] == sizes[1] else None,
            "prims": prims[:sizes[1]].copy(), "cost": (cost[0], cost[1], cost[2]),
            "valid": int(valid.value)}


class Core:
    def __init__(self, device=0):
        self._lib = _lib()
        self._ctx = C.c_void_p()
        self._lib.lumc_context_create.restype = C.c_int
        rc = self._lib.lumc_context_create(C.c_int(device), C.byref(self._ctx))
        if rc != 0:
            msg = self._lib.lumc_last_error(self._ctx).decode() if self._ctx else "context allocation failed"
            if self._ctx:
                self._lib.lumc_context_destroy(self._ctx)
                self._ctx = C.c_void_p()
            raise CoreError("lumc_context_create failed (no CPU fallback exists): " + msg)
        self.num_pixels = 0

    @property
    def flavour(self):
        """'fast' or 'exact': the arithmetic flavour of the wavefront kernels this context launches (lumc_get_flavour)."""
        fn = getattr(self._lib, "lumc_get_flavour", None)
        if fn is None:
            return "exact"
        fn.restype = C.c_int
        return "fast" if fn(self._ctx) == 1 else "exact"

    # ---- multi-GPU (lumc_comm_*, lumc_frame_*) ----
    @staticmethod
    def device_count():
        return int(_lib().lumc_device_count())

    @staticmethod
    def tile_pixels(width, height, rank, world, tile=32):
        """The C ABI's tile deal (== luminary_amd.distributed.tile_pixels)."""
        lib = _lib()
        n = C.c_uint32()
        if lib.lumc_tile_pixels(C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(world), C.c_uint32(tile), C.c_void_p(0), C.byref(n)):
            raise CoreError("lumc_tile_pixels: bad arguments")
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        lib.lumc_tile_pixels(C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(world), C.c_uint32(tile), out.ctypes.data_as(C.c_void_p), C.byref(n))
        return out[:n.value]

    @staticmethod
    def comm_unique_id():
        """128 bytes identifying a new RCCL communicator (made on one rank, handed to all)."""
        buf = (C.c_uint8 * 128)()
        if _lib().lumc_comm_unique_id(buf):
            raise CoreError("lumc_comm_unique_id failed")
        return bytes(buf)

    def comm_init_rank(self, world, rank, unique_id):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._call("lumc_comm_init_rank", C.c_int(world), C.c_int(rank), buf)

    def frame_assemble(self, frame_pixels, root=0, stream=0):
        """This rank's accumulators scattered into its [4][frame_pixels] frame and reduced (RCCL SUM) to `root`; returns the device pointer of
        this rank's frame (complete on root)."""
        ptr = C.c_void_p()
        self._call("lumc_frame_assemble", C.c_uint32(frame_pixels), C.c_int(root), C.c_void_p(stream), C.byref(ptr))
        return ptr.value

    def frame_gather(self, width, height, root=0, stream=0):
        """The frame by a gather of the ranks' own pixels (this context holds its share of the 32x32 tile deal): pack, ONE ncclGather to `root`, scatter there.
        Returns the device pointer of the assembled frame on root, None elsewhere (lumc_frame_gather)."""
        ptr = C.c_void_p()
        self._call("lumc_frame_gather", C.c_uint32(width), C.c_uint32(height), C.c_int(root), C.c_void_p(stream), C.byref(ptr))
        return ptr.value

    def frame_download(self, frame_pixels):
        fm = np.zeros(3 * frame_pixels, dtype=np.float32)
        sm = np.zeros(frame_pixels, dtype=np.float32)
        self._call("lumc_frame_download", C.c_uint32(frame_pixels), fm.ctypes.data_as(C.c_void_p), sm.ctypes.data_as(C.c_void_p))
        return fm.reshape(3, -1), sm

    @property
    def ray_sorting(self):
        fn = self._lib.lumc_get_ray_sorting
        fn.restype = C.c_int
        return int(fn(self._ctx))

    def set_ray_sorting(self, mode):
        """0 queue order, 1 closest-hit rays of depth >= 1 sorted by (origin cell, direction octant), 2 visibility rays too."""
        self._call("lumc_set_ray_sorting", C.c_int(mode))

    def set_fused_resolve(self, on):
        """Fast flavour with the ambient reuse: the resolve of a depth rides in the next depth's shading kernel (lumc_set_fused_resolve; default on)."""
        self._call("lumc_set_fused_resolve", C.c_int(int(on)))  # (2: with k_resolve_ended as a kernel of its own)

    def set_sobol_table(self, on):
        """The shading kernel reads a pass's Sobol / Owen pairs from a table written once per pass instead of hashing (lumc_set_sobol_table; default on; bit-identical)."""
        self._call("lumc_set_sobol_table", C.c_int(1 if on else 0))

    def set_ambient_reuse(self, mode):
        """-1 by flavour (fast: on, exact: off), 0 off, 1 on - in the exact flavour the reuse then only takes what it can prove and stays bit-identical (lumc_set_ambient_reuse)"""
        self._call("lumc_set_ambient_reuse", C.c_int(mode))

    @property
    def ambient_reuse(self):
        """does the next render answer ambient samples from the closest-hit rays (lumc_get_ambient_reuse: by mode, flavour and scene)?"""
        fn = self._lib.lumc_get_ambient_reuse
        fn.restype = C.c_int
        return bool(fn(self._ctx))

    def set_single_level(self, mode):
        """-1 auto, 0 never, 1 when eligible: the ray kernels walk a scene of one hittable instance from its mesh root (lumc_set_single_level; bit-identical)"""
        self._call("lumc_set_single_level", C.c_int(mode))

    def get_single_level(self):
        """1 when the next ray-kernel launch takes the single-level form for the uploaded scene (lumc_get_single_level: by mode and scene), else 0"""
        fn = self._lib.lumc_get_single_level
        fn.restype = C.c_int
        return int(fn(self._ctx))

    def set_plain_form(self, mode):
        """-1 auto, 0 never, 1 when eligible: the shading kernel's form without refraction, light-tree descent and textured lights (lumc_set_plain_form)"""
        self._call("lumc_set_plain_form", C.c_int(mode))

    def get_plain_form(self):
        """1 when the next launch of the shading kernel takes the plain form for the uploaded scene (lumc_get_plain_form: by mode and scene), else 0"""
        fn = self._lib.lumc_get_plain_form
        fn.restype = C.c_int
        return int(fn(self._ctx))

    def set_overlap_light_query(self, mode):
        """-1 auto, 0 never, 1 when allowed: a depth's light queries run on the context's side stream beside the next depth's closest-hit pass
        (lumc_set_overlap_light_query; bit-identical)"""
        self._call("lumc_set_overlap_light_query", C.c_int(mode))

    def get_overlap_light_query(self):
        """1 when the next pass takes the overlapped order for the uploaded scene (lumc_get_overlap_light_query: by mode, scheme, scene and registers), else 0"""
        fn = self._lib.lumc_get_overlap_light_query
        fn.restype = C.c_int
        return int(fn(self._ctx))

    def set_pixel_major(self, mode):
        """-1 auto, 0 sample-major, 1 pixel-major: the order of render()'s path slots (lumc_set_pixel_major; bit-identical)"""
        self._call("lumc_set_pixel_major", C.c_int(mode))

    def get_pixel_major(self):
        """1 when the next render() numbers its path slots pixel-major (lumc_get_pixel_major), else 0"""
        fn = self._lib.lumc_get_pixel_major
        fn.restype = C.c_int
        return int(fn(self._ctx))

    def set_coherent_first_hits(self, mode):
        """-1 auto, 0 never, 1 when eligible (then for trace_closest too): the depth-0 closest-hit launch visits a node once per wave where its lanes agree
        (lumc_set_coherent_first_hits; bit-identical)"""
        self._call("lumc_set_coherent_first_hits", C.c_int(mode))

    def get_coherent_first_hits(self):
        """1 when the next render()'s depth-0 launch takes the coherent form at a batch of 64 (lumc_get_coherent_first_hits: by mode, slots and scene), else 0"""
        fn = self._lib.lumc_get_coherent_first_hits
        fn.restype = C.c_int
        return int(fn(self._ctx))

    @staticmethod
    def overlap_registers_fit(ray_kernel_regs, light_query_regs):
        """lumc_overlap_registers_fit: does one wave of the light queries fit beside the ray kernel's four on a SIMD (no device needed)?"""
        fn = _lib().lumc_overlap_registers_fit
        fn.restype = C.c_int
        return bool(fn(C.c_uint32(ray_kernel_regs), C.c_uint32(light_query_regs)))

    def set_physical_camera(self, camera):
        """lumc_set_physical_camera: a PhysicalCamera, or None for the scene's thin lens"""
        self._call("lumc_set_physical_camera", C.byref(camera) if camera is not None else C.c_void_p(0))

    def camera_rays(self, pixels, first_sample, samples):
        """lumc_camera_rays: every camera ray of the sample ids x pixels, sample-major: origins [N, 3], directions [N, 3], weights [N] (0: invalid)"""
        px = np.ascontiguousarray(pixels, dtype=np.uint32)
        n = px.size * samples
        o = np.zeros((n, 3), dtype=np.float32)
        d = np.zeros((n, 3), dtype=np.float32)
        w = np.zeros(n, dtype=np.float32)
        self._call("lumc_camera_rays", px.ctypes.data_as(C.c_void_p), C.c_uint32(px.size), C.c_uint32(first_sample), C.c_uint32(samples),
                   o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
        return o, d, w

    def pixel_query(self, x, y, sample_id=0):
        """lumc_pixel_query: (instance id, triangle id, t, direction [3])"""
        out = (C.c_uint32 * 6)()
        self._call("lumc_pixel_query", C.c_uint32(x), C.c_uint32(y), C.c_uint32(sample_id), out)
        a = np.array(list(out), dtype=np.uint32)
        return int(a[0]), int(a[1]), float(a[2:3].view(np.float32)[0]), a[3:6].view(np.float32).copy()

    def set_flavour(self, name):
        self._call("lumc_set_flavour", C.c_int({"exact": 0, "fast": 1}[name]))

    def _call(self, name, *args):
        fn = getattr(self._lib, name)
        fn.restype = C.c_int
        if fn(self._ctx, *args) != 0:
            raise CoreError("%s failed: %s" % (name, self._lib.lumc_last_error(self._ctx).decode()))

    def close(self):
        if self._ctx:
            self._lib.lumc_context_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, view):
        self._view_keepalive = view
        self._call("lumc_scene_upload", C.byref(view))
        self.width, self.height = view.width, view.height

    def update(self, view, dirty):
        """lumc_scene_update: takes over only the parts of `view` named by `dirty` (DIRTY_* below); the accumulation is not touched."""
        self._view_keepalive = view
        self._call("lumc_scene_update", C.byref(view), C.c_uint(dirty))
        self.width, self.height = view.width, view.height

    def generate_output(self, params, first_moment=None, want_float=False):
        """ARGB8 image [dst_height, dst_width] (uint32 words b | g<<8 | r<<16 | a<<24). `first_moment`: None = the context's own
        accumulators, an int = device pointer to a planar [3*P] first moment, a numpy array = host data (uploaded). Optionally also
        returns the display-referred float planes [3, src_height, src_width]."""
        out = np.zeros((params.dst_height, params.dst_width), dtype=np.uint32)
        planes = np.zeros(params.output_planes_shape(), dtype=np.float32) if want_float else None
        pl = planes.ctypes.data_as(C.c_void_p) if want_float else C.c_void_p(0)
        if isinstance(first_moment, np.ndarray):
            fm = np.ascontiguousarray(first_moment, dtype=np.float32)
            self._call("lumc_generate_output_from_host", C.byref(params), fm.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), pl)
        else:
            ptr = C.c_void_p(0) if first_moment is None else C.c_void_p(int(first_moment))
            self._call("lumc_generate_output_host", C.byref(params), ptr, out.ctypes.data_as(C.c_void_p), pl)
        return (out, planes) if want_float else out

    def download_luts(self):
        out = {"conductor": np.zeros(1024, np.uint16), "glossy": np.zeros(1024, np.uint16), "dielectric": np.zeros(32768, np.uint16),
               "dielectric_inv": np.zeros(32768, np.uint16)}
        self._call("lumc_download_luts", *[out[k].ctypes.data_as(C.c_void_p) for k in ("conductor", "glossy", "dielectric", "dielectric_inv")])
        return out

    def download_sky_luts(self):
        """The procedural sky's transmittance and multiscattering tables as flat float32 arrays (2*64*256*4 and 2*32*32*4)."""
        tm = np.zeros(2 * 64 * 256 * 4, dtype=np.float32)
        ms = np.zeros(2 * 32 * 32 * 4, dtype=np.float32)
        self._call("lumc_download_sky_luts", tm.ctypes.data_as(C.c_void_p), ms.ctypes.data_as(C.c_void_p))
        return tm, ms

    def cloud_noise_generate(self, seed):
        """The clouds' noise textures as the core generates them: (shape [128^3], detail [32^3], weather [1024^2]) as uint32 RGBA8."""
        shape, detail, weather = np.zeros(128 ** 3, np.uint32), np.zeros(32 ** 3, np.uint32), np.zeros(1024 ** 2, np.uint32)
        self._call("lumc_cloud_noise_generate", C.c_uint32(seed), shape.ctypes.data_as(C.c_void_p), detail.ctypes.data_as(C.c_void_p),
                   weather.ctypes.data_as(C.c_void_p))
        return shape, detail, weather

    def sky_hdri_build(self, origin, dim, samples):
        """Bakes the procedural sky seen from `origin` (world space) and returns it as [dim, dim, 4] float32."""
        o = (C.c_float * 3)(*[float(x) for x in origin])
        self._call("lumc_sky_hdri_build", o, C.c_uint32(dim), C.c_uint32(samples))
        out = np.zeros((dim, dim, 4), dtype=np.float32)
        self._call("lumc_sky_hdri_download", out.ctypes.data_as(C.c_void_p), C.c_void_p(0))
        return out

    def sky_hdri_download(self):
        """The panorama the context holds (baked at upload in sky mode HDRI, or by sky_hdri_build), [dim, dim, 4] float32."""
        dim = C.c_uint32()
        self._call("lumc_sky_hdri_download", C.c_void_p(0), C.byref(dim))
        out = np.zeros((dim.value, dim.value, 4), dtype=np.float32)
        self._call("lumc_sky_hdri_download", out.ctypes.data_as(C.c_void_p), C.byref(dim))
        return out

    def set_pixels(self, pixels=None):
        if pixels is None:
            self._call("lumc_set_pixels", C.c_void_p(0), C.c_uint32(0))
            self.num_pixels = self.width * self.height
        else:
            px = np.ascontiguousarray(pixels, dtype=np.uint32)
            self._call("lumc_set_pixels", px.ctypes.data_as(C.c_void_p), C.c_uint32(px.size))
            self.num_pixels = int(px.size)

    def render(self, first_sample, num_samples, samples_per_pass=1, first_moment_ptr=0, second_moment_ptr=0, stream=0):
        self._call("lumc_render", C.c_uint32(first_sample), C.c_uint32(num_samples), C.c_uint32(samples_per_pass), C.c_void_p(first_moment_ptr),
                   C.c_void_p(second_moment_ptr), C.c_void_p(stream))

    def synchronize(self):
        self._call("lumc_synchronize")

    def clear(self):
        self._call("lumc_clear_accumulators")

    def accumulators(self):
        fm = np.zeros(3 * self.num_pixels, dtype=np.float32)
        sm = np.zeros(self.num_pixels, dtype=np.float32)
        self._call("lumc_download_accumulators", fm.ctypes.data_as(C.c_void_p), sm.ctypes.data_as(C.c_void_p))
        return fm.reshape(3, -1), sm

    def counters(self):
        out = (C.c_uint64 * CNT_COUNT)()
        self._call("lumc_counters", out)
        return [int(x) for x in out]

    def query_counters(self):
        """counters() with the visibility entry as QUERIES answered - rays traced plus the ambient samples the closest-hit rays answered (minus those traced
        after all): what a renderer that traces every visibility ray counts, e.g. the oracle."""
        c = self.counters()
        c[CNT_SHADOW] += c[CNT_AMBIENT_DEFERRED] - c[CNT_AMBIENT_FALLBACK]
        return c

    def reset_counters(self):
        self._call("lumc_reset_counters")

    def set_profiling(self, on):
        self._call("lumc_set_profiling", C.c_int(1 if on else 0))

    def kernel_times(self):
        """{kernel: (ms, launches)} since set_profiling(True). Under the overlapped schedule (set_overlap_light_query) the light queries run beside the closest-hit
        pass, so the times no longer add up to the step's."""
        ms =(C.c_double * len(KERNELS))()
        n = (C.c_uint32 * len(KERNELS))()
        self._call("lumc_kernel_times", ms, n)
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(KERNELS)}

    # ---- adaptive sampling (lumc_adaptive_*) ----
    def adaptive_begin(self, max_rate, avg_rate, update_interval, exposure=0.0, tone=None):
        p = AdaptiveParams()
        p.max_sampling_rate, p.avg_sampling_rate, p.update_interval, p.exposure = max_rate, avg_rate, update_interval, exposure
        if tone is not None:
            p.tone = tone
        self._call("lumc_adaptive_begin", C.byref(p))

    def adaptive_render(self, executions, stream=0):
        self._call("lumc_adaptive_render", C.c_uint32(executions), C.c_void_p(stream))

    def adaptive_info(self):
        info = AdaptiveInfo()
        self._call("lumc_adaptive_info", C.byref(info))
        return {"stage_id": int(info.stage_id), "executions": [int(x) for x in info.executions], "num_blocks": int(info.num_blocks),
                "blocks": (int(info.blocks_x), int(info.blocks_y)), "tasks_per_execution": int(info.tasks_per_execution),
                "variance_total": float(info.variance_total), "build_pending": bool(info.build_pending)}

    @staticmethod
    def adaptive_info_of(ctx):
        """adaptive_info of a context owned by somebody else (Host.core_context())."""
        info = AdaptiveInfo()
        if _lib().lumc_adaptive_info(C.c_void_p(ctx), C.byref(info)):
            raise CoreError("lumc_adaptive_info failed")
        return {"stage_id": int(info.stage_id), "executions": [int(x) for x in info.executions]}

    def adaptive_download(self):
        n = self.adaptive_info()["num_blocks"]
        counts = np.zeros(n, dtype=np.uint32)
        variance = np.zeros(n, dtype=np.float32)
        self._call("lumc_adaptive_download", counts.ctypes.data_as(C.c_void_p), variance.ctypes.data_as(C.c_void_p))
        return counts, variance

    def adaptive_set_partition(self, block_mask):
        """Blocks (4x4 pixels, row-major) this context renders: uint8 array of num_blocks entries."""
        m = np.ascontiguousarray(block_mask, dtype=np.uint8)
        assert m.size == self.adaptive_info()["num_blocks"]
        self._call("lumc_adaptive_set_partition", m.ctypes.data_as(C.c_void_p))

    def adaptive_variance(self):
        v = np.zeros(self.adaptive_info()["num_blocks"], dtype=np.float32)
        self._call("lumc_adaptive_variance", v.ctypes.data_as(C.c_void_p))
        return v

    def adaptive_build_from(self, block_variance):
        v = np.ascontiguousarray(block_variance, dtype=np.float32)
        self._call("lumc_adaptive_build_from", v.ctypes.data_as(C.c_void_p))

    def adaptive_end(self):
        self._call("lumc_adaptive_end")

    def generate_result(self, mode=0, local_error_minimization=False, uniform_samples=0, exposure=1.0, tone=None):
        """Mean-radiance / diagnostic image [3, H, W] of the context's full-frame accumulators (lumc_generate_result_host)."""
        out = np.zeros((3, self.height, self.width), dtype=np.float32)
        tp = C.byref(tone) if tone is not None else C.c_void_p(0)
        self._call("lumc_generate_result_host", C.c_uint32(mode), C.c_uint32(1 if local_error_minimization else 0), C.c_uint32(uniform_samples),
                   C.c_float(exposure), tp, out.ctypes.data_as(C.c_void_p))
        return out

    def post_bloom(self, image, full_width, full_height, blend, stage=0):
        """Bloom of a planar result image [3, H >> stage, W >> stage] (host array); returns the processed copy."""
        img = np.ascontiguousarray(image, dtype=np.float32).copy()
        self._call("lumc_post_bloom_host", img.ctypes.data_as(C.c_void_p), C.c_uint32(full_width), C.c_uint32(full_height), C.c_uint32(stage), C.c_float(blend))
        return img

    # ---- denoiser (lumc_render_guides, lumc_denoise) ----
    def render_guides(self, num_samples=4, stream=0):
        """First-hit guides of the whole frame from sample ids [0, num_samples); returns (albedo [3, H, W], normal [3, H, W], depth [H, W], -1 = nothing hit)."""
        self._call("lumc_render_guides", C.c_uint32(num_samples), C.c_void_p(stream))
        return self.guides()

    def guides(self):
        a, n, d = (np.zeros((3, self.height, self.width), np.float32), np.zeros((3, self.height, self.width), np.float32), np.zeros((self.height, self.width), np.float32))
        self._call("lumc_download_guides", a.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
        return a, n, d

    def set_denoise_form(self, lds):
        """a-trous iterations with taps 1 and 2 apart: tile and halo staged in LDS (True, default) or every tap loaded directly; same bits"""
        self._call("lumc_set_denoise_form", C.c_int(1 if lds else 0))

    def denoise(self, image=None, params=None, **fields):
        """lumc_denoise on a planar image [3, H, W] (host array; returns the filtered copy) or, with image None, in place on the context's result image
        (returns it). `params`: DenoiseParams, or the defaults with `fields` changed."""
        p = params if params is not None else default_denoise_params(**fields)
        if image is None:
            self._call("lumc_denoise", C.byref(p), C.c_void_p(0), C.c_void_p(0))
            out = np.zeros((3, self.height, self.width), dtype=np.float32)
            self._call("lumc_download_result_image", out.ctypes.data_as(C.c_void_p))
            return out
        img = np.ascontiguousarray(image, dtype=np.float32).copy()
        self._call("lumc_denoise_host", C.byref(p), img.ctypes.data_as(C.c_void_p))
        return img

    def render_undersampled(self, stage, iteration, stream=0):
        """Adds sample 0 of the pixels of one undersampling iteration to the full-frame accumulators (lumc_render_undersampled)."""
        self._call("lumc_render_undersampled", C.c_uint32(stage), C.c_uint32(iteration), C.c_void_p(stream))

    def generate_result_undersampled(self, stage, iteration):
        """The compact preview image [3, H >> stage, W >> stage] of the pixels rendered so far."""
        out = np.zeros((3, self.height >> stage, self.width >> stage), dtype=np.float32)
        self._call("lumc_generate_result_undersampled_host", C.c_uint32(stage), C.c_uint32(iteration), out.ctypes.data_as(C.c_void_p))
        return out

    def adaptive_note_first_sample(self):
        self._call("lumc_adaptive_note_first_sample", C.c_void_p(0))

    def set_bvh_builder(self, name):
        """'sah' (host, default), 'lbvh', 'ploc' or 'sah_gpu' (the GPU builders) for the next upload."""
        self._call("lumc_set_bvh_builder", C.c_int({"sah": 0, "lbvh": 1, "ploc": 2, "sah_gpu": 3}[name]))

    def comm_count(self):
        """Ranks of the RCCL communicator this context belongs to (ncclCommCount; 1 without one)."""
        fn = self._lib.lumc_comm_count
        fn.restype = C.c_int
        return int(fn(self._ctx))

    def lds_stack_bytes(self):
        """Bytes of a ray workgroup's LDS that hold traversal stack entries (build-time constant of the library)."""
        fn = self._lib.lumc_lds_stack_bytes
        fn.restype = C.c_uint
        return int(fn())

    def set_mesh_refit(self, mode=0, max_cost_growth=0.0):
        """lumc_set_mesh_refit: how DIRTY_MESH_POSITIONS updates take a moved mesh over: 0 refit, 1 build again; max_cost_growth > 0: build again beyond it."""
        self._call("lumc_set_mesh_refit", C.c_uint32(mode), C.c_float(max_cost_growth))

    def mesh_refit_stats(self):
        out = MeshRefitStats()
        self._call("lumc_mesh_refit_stats", C.byref(out))
        return out

    def set_instance_update(self, mode=0):
        """lumc_set_instance_update: how DIRTY_INSTANCE_TRANSFORMS updates are taken over: 0 on the device, 1 as DIRTY_INSTANCES (the host assembles the scene tree)."""
        self._call("lumc_set_instance_update", C.c_uint32(mode))

    def instance_update_stats(self):
        out = InstanceUpdateStats()
        self._call("lumc_instance_update_stats", C.byref(out))
        return out

    def set_mesh_refit_in_place(self, on=1):
        """lumc_set_mesh_refit_in_place: 1 = DIRTY_MESH_POSITIONS updates (alone or with DIRTY_INSTANCE_TRANSFORMS) refit in the resident node array and keep its layout."""
        self._call("lumc_set_mesh_refit_in_place", C.c_uint32(on))

    def resident_refit_stats(self):
        out = ResidentRefitStats()
        self._call("lumc_resident_refit_stats", C.byref(out))
        return out

    def mesh_skin_bind(self, mesh, rest_positions, rest_normals, bone_ids, weights, bone_count):
        """lumc_mesh_skin_bind: rest positions / normals [n, 9], bone ids / weights [n, 12] of a mesh of the scene on the device become resident."""
        p, n, i, w = _skin_arrays(rest_positions, rest_normals, bone_ids, weights)
        self._call("lumc_mesh_skin_bind", C.c_uint32(mesh), C.c_void_p(p.ctypes.data), C.c_void_p(n.ctypes.data), C.c_void_p(i.ctypes.data), C.c_void_p(w.ctypes.data),
                   C.c_uint32(len(p)), C.c_uint32(bone_count))

    def mesh_skin_unbind(self, mesh):
        self._call("lumc_mesh_skin_unbind", C.c_uint32(mesh))

    def mesh_skin_pose(self, mesh, bones):
        """lumc_mesh_skin_pose: bones [b, 12]; pending until the next update with DIRTY_MESH_SKIN."""
        b = np.ascontiguousarray(bones, dtype=np.float32).reshape(-1, 12)
        self._call("lumc_mesh_skin_pose", C.c_uint32(mesh), C.c_void_p(b.ctypes.data), C.c_uint32(len(b)))

    def mesh_skin_stats(self):
        out = MeshSkinStats()
        self._call("lumc_mesh_skin_stats", C.byref(out))
        return out

    def mesh_morph_bind(self, mesh, base_positions, base_normals, offsets, corners, delta_positions, delta_normals=None):
        """lumc_mesh_morph_bind: base positions / normals [n, 9] and sparse target-major deltas (offsets [T + 1] into corners [E], delta positions / normals [E, 3])
        of a mesh of the scene on the device become resident, all weights 0."""
        p, n, o, c, dp, dn = _morph_arrays(base_positions, base_normals, offsets, corners, delta_positions, delta_normals)
        self._call("lumc_mesh_morph_bind", C.c_uint32(mesh), C.c_void_p(p.ctypes.data), C.c_void_p(n.ctypes.data), C.c_uint32(len(p)), C.c_uint32(len(o) - 1),
                   C.c_void_p(o.ctypes.data), _addr(c), _addr(dp), _addr(dn))

    def mesh_morph_unbind(self, mesh):
        self._call("lumc_mesh_morph_unbind", C.c_uint32(mesh))

    def mesh_morph_weights(self, mesh, weights):
        """lumc_mesh_morph_weights: weights [T]; pending until the next update with DIRTY_MESH_SKIN."""
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        self._call("lumc_mesh_morph_weights", C.c_uint32(mesh), C.c_void_p(w.ctypes.data), C.c_uint32(len(w)))

    def mesh_morph_stats(self):
        out = MeshMorphStats()
        self._call("lumc_mesh_morph_stats", C.byref(out))
        return out

    # ---- firefly rejection (lumc_set_firefly_buckets, lumc_firefly_resolve) ----
    def set_firefly_buckets(self, buckets):
        """lumc_set_firefly_buckets: 0 off (default), 4 ... 16 median-of-means buckets beside the accumulators (12 bytes per pixel each); clears the accumulators."""
        self._call("lumc_set_firefly_buckets", C.c_uint32(buckets))
        self._firefly_buckets = int(buckets)

    def buckets(self):
        """lumc_download_buckets: (sums [K, 3, num_pixels] float32, counts [K] uint32)."""
        K = getattr(self, "_firefly_buckets", 0)
        sums = np.zeros((max(K, 1), 3, self.num_pixels), dtype=np.float32)
        counts = np.zeros(max(K, 1), dtype=np.uint32)
        self._call("lumc_download_buckets", sums.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p))
        return sums, counts

    def upload_buckets(self, sums=None, counts=None):
        """lumc_upload_buckets: the inverse of buckets(); either part may be None."""
        K = getattr(self, "_firefly_buckets", 0)
        s = None if sums is None else np.ascontiguousarray(sums, dtype=np.float32)
        n = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        if (s is not None and s.size != K * 3 * self.num_pixels) or (n is not None and n.size != K):
            raise ValueError("upload_buckets: sums [K, 3, num_pixels], counts [K]")
        self._call("lumc_upload_buckets", C.c_void_p(0 if s is None else s.ctypes.data), C.c_void_p(0 if n is None else n.ctypes.data))

    def firefly_resolve(self):
        """lumc_firefly_resolve in place on the context's result image (generate_result wrote it); returns it, [3, H, W]."""
        self._call("lumc_firefly_resolve", C.c_void_p(0), C.c_void_p(0))
        out = np.zeros((3, self.height, self.width), dtype=np.float32)
        self._call("lumc_download_result_image", out.ctypes.data_as(C.c_void_p))
        return out

    def firefly_stats(self):
        out = FireflyStats()
        self._call("lumc_firefly_stats", C.byref(out))
        return out

    # ---- ID mattes (lumc_render_first_hits, lumc_download_mattes, lumc_matte_mask) ----
    def render_first_hits(self, num_samples=4, what=FIRST_HIT_GUIDES | FIRST_HIT_MATTES, layers=MATTE_INSTANCE | MATTE_MATERIAL, stream=0):
        """lumc_render_first_hits: one closest-hit pass per sample id of the whole frame into the denoiser's guides, the ID mattes, or both from the same rays."""
        self._call("lumc_render_first_hits", C.c_uint32(num_samples), C.c_uint32(what), C.c_uint32(layers), C.c_void_p(stream))

    def render_mattes(self, num_samples=4, layers=MATTE_INSTANCE | MATTE_MATERIAL):
        self.render_first_hits(num_samples, FIRST_HIT_MATTES, layers)

    def mattes(self, layer, ranks=MATTE_SLOTS):
        """lumc_download_mattes of one layer (MATTE_INSTANCE or MATTE_MATERIAL): (ids [ranks, P] uint32, coverage [ranks, P] float32, dropped [P], rays [P])."""
        P, R = self.width * self.height, max(min(int(ranks), MATTE_SLOTS), 1)
        ids, cov, dropped, rays = np.zeros((R, P), np.uint32), np.zeros((R, P), np.float32), np.zeros(P, np.uint32), np.zeros(P, np.uint32)
        self._call("lumc_download_mattes", C.c_uint32(layer), C.c_uint32(ranks), *[C.c_void_p(a.ctypes.data) for a in (ids, cov, dropped, rays)])
        return ids, cov, dropped, rays

    def matte_tables(self, layer):
        """lumc_download_matte_tables: the raw slots (slots_id [8, P], slots_count [8, P], dropped [P])."""
        P = self.width * self.height
        si, sc, dropped = np.zeros((MATTE_SLOTS, P), np.uint32), np.zeros((MATTE_SLOTS, P), np.uint32), np.zeros(P, np.uint32)
        self._call("lumc_download_matte_tables", C.c_uint32(layer), *[C.c_void_p(a.ctypes.data) for a in (si, sc, dropped)])
        return si, sc, dropped

    def matte_mask(self, layer, ids):
        """lumc_matte_mask_host: the coverage [P] float32 of up to 16 ids per pixel."""
        want = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        mask = np.zeros(self.width * self.height, np.float32)
        self._call("lumc_matte_mask_host", C.c_uint32(layer), C.c_void_p(want.ctypes.data if want.size else None), C.c_uint32(want.size), C.c_void_p(mask.ctypes.data))
        return mask

    def has_mattes(self):
        fn = self._lib.lumc_has_mattes
        fn.restype = C.c_int
        return bool(fn(self._ctx))

    def has_guides(self):
        fn = self._lib.lumc_has_guides
        fn.restype = C.c_int
        return bool(fn(self._ctx))

    def matte_release(self):
        self._call("lumc_matte_release")

    def matte_stats(self):
        out = MatteStats()
        self._call("lumc_matte_stats", C.byref(out))
        return out

    # ---- image history (lumc_set_history, lumc_history_carry, lumc_history_blend) ----
    def set_history(self, params):
        self._call("lumc_set_history", C.byref(params))

    def history_carry(self, stream=0):
        self._call("lumc_history_carry", C.c_void_p(stream))

    def history_blend(self, uniform_samples, d_image=None, stream=0):
        self._call("lumc_history_blend", C.c_uint32(uniform_samples), C.c_void_p(d_image), C.c_void_p(stream))

    def history_drop(self, why=b"dropped by the caller"):
        self._history_why = why if isinstance(why, bytes) else str(why).encode()  # (kept by pointer)
        self._call("lumc_history_drop", C.c_char_p(self._history_why))

    def history_release(self):
        self._call("lumc_history_release")

    def history_stats(self):
        out = HistoryStats()
        self._call("lumc_history_stats", C.byref(out))
        return out

    def history_keys(self):
        """(the state's key, the context's camera as a key)"""
        a, b = HistoryKey(), HistoryKey()
        self._call("lumc_history_key", C.byref(a), C.byref(b))
        return a, b

    def download_history(self):
        """lumc_download_history: (shown [3, P], weight [P], carried [3, P], carried_weight [P])"""
        P = self.width * self.height
        shown, weight, carried, cw = np.zeros((3, P), np.float32), np.zeros(P, np.float32), np.zeros((3, P), np.float32), np.zeros(P, np.float32)
        self._call("lumc_download_history", *[C.c_void_p(a.ctypes.data) for a in (shown, weight, carried, cw)])
        return shown, weight, carried, cw

    def history_kernels(self, now_key, old_key, params, uniform_samples, image, normal, depth, old_shown, old_weight, old_normal, old_depth):
        """lumc_history_kernels_host: k_history_reproject and k_history_blend on host planes (as the twins take them). Returns a dict: image, carried, carried_weight,
        stats, shown, weight, state_normal, state_depth."""
        P, Q = now_key.width * now_key.height, old_key.width * old_key.height
        ins = [_f32(normal, (3, P), "normal"), _f32(depth, (P,), "depth"), _f32(old_shown, (3, Q), "old_shown"), _f32(old_weight, (Q,), "old_weight"),
               _f32(old_normal, (3, Q), "old_normal"), _f32(old_depth, (Q,), "old_depth")]
        out = {"image": _f32(image, (3, P), "image").copy(), "carried": np.zeros((3, P), np.float32), "carried_weight": np.zeros(P, np.float32), "shown": np.zeros((3, P), np.float32),
               "weight": np.zeros(P, np.float32), "state_normal": np.zeros((3, P), np.float32), "state_depth": np.zeros(P, np.float32)}
        stats = (C.c_uint32 * 3)()
        self._call("lumc_history_kernels_host", C.byref(now_key), C.byref(old_key), C.byref(params), C.c_uint32(uniform_samples),
                   *[C.c_void_p(a.ctypes.data) for a in ins], C.c_void_p(out["image"].ctypes.data), C.c_void_p(out["carried"].ctypes.data),
                   C.c_void_p(out["carried_weight"].ctypes.data), stats, C.c_void_p(out["shown"].ctypes.data), C.c_void_p(out["weight"].ctypes.data),
                   C.c_void_p(out["state_normal"].ctypes.data), C.c_void_p(out["state_depth"].ctypes.data))
        out["stats"] = tuple(int(x) for x in stats)
        return out

    # ---- image history, motion (lumc_set_history_motion) ----
    def set_history_motion(self, enabled=True, motion_max_history=8.0):
        p = HistoryMotionParams(1 if enabled else 0, motion_max_history)
        self._call("lumc_set_history_motion", C.byref(p))

    def has_history_snapshot(self):
        fn = self._lib.lumc_has_history_snapshot
        fn.restype = C.c_int
        return bool(fn(self._ctx))

    def history_motion_stats(self):
        out = HistoryMotionStats()
        self._call("lumc_history_motion_stats", C.byref(out))
        return out

    def download_history_owner(self, state=True, current=True):
        """lumc_download_history_owner: (the state's owner plane or None, the current one or None), uint32 [P]"""
        P = self.width * self.height
        a, b = (np.zeros(P, np.uint32) if state else None), (np.zeros(P, np.uint32) if current else None)
        self._call("lumc_download_history_owner", C.c_void_p(a.ctypes.data if state else None), C.c_void_p(b.ctypes.data if current else None))
        return a, b

    def download_history_transforms(self, instances):
        """lumc_download_history_transforms: (the state's snapshot [count, 8] or None where none is held, the scene's current transforms [instances, 8])"""
        count = C.c_uint32()
        self._call("lumc_download_history_transforms", C.c_void_p(None), C.c_void_p(None), C.byref(count))
        snap, cur = np.zeros((count.value, 8), np.float32), np.zeros((int(instances), 8), np.float32)
        self._call("lumc_download_history_transforms", C.c_void_p(snap.ctypes.data if count.value else None), C.c_void_p(cur.ctypes.data if instances else None), C.byref(count))
        return (snap if count.value else None), cur

    def history_motion_kernels(self, now_key, old_key, params, motion_max_history, normal, depth, old_shown, old_weight, old_normal, old_depth, owner, old_owner, old8, new8, hit_ids=None):
        """lumc_history_motion_kernels_host: k_history_owner (where hit_ids [paths, 4] uint32 is given; `owner` is ignored then), k_history_motion and
        k_history_reproject_motion on host planes. Returns a dict: owner, records, motion_stats, carried, carried_weight, stats."""
        P, Q = now_key.width * now_key.height, old_key.width * old_key.height
        ins = [_f32(normal, (3, P), "normal"), _f32(depth, (P,), "depth"), _f32(old_shown, (3, Q), "old_shown"), _f32(old_weight, (Q,), "old_weight"),
               _f32(old_normal, (3, Q), "old_normal"), _f32(old_depth, (Q,), "old_depth")]
        hits = None if hit_ids is None else np.ascontiguousarray(hit_ids, np.uint32).reshape(-1, 4)
        own = None if owner is None else _u32(owner, (P,), "owner")
        oown = _u32(old_owner, (Q,), "old_owner")
        o8, n8 = np.ascontiguousarray(old8, np.float32).reshape(-1, 8), np.ascontiguousarray(new8, np.float32).reshape(-1, 8)
        if o8.shape != n8.shape:
            raise ValueError("old8 and new8 differ in shape")
        count = o8.shape[0]
        out = {"owner": np.zeros(P, np.uint32), "records": np.zeros(count, HISTORY_MOTION_RECORD), "carried": np.zeros((3, P), np.float32), "carried_weight": np.zeros(P, np.float32)}
        ms, st = (C.c_uint32 * 3)(), (C.c_uint32 * 5)()
        ptr = lambda a: C.c_void_p(None if a is None or a.size == 0 else a.ctypes.data)
        self._call("lumc_history_motion_kernels_host", C.byref(now_key), C.byref(old_key), C.byref(params), C.c_float(motion_max_history), *[ptr(a) for a in ins],
                   ptr(hits), C.c_uint32(0 if hits is None else hits.shape[0]), ptr(own), ptr(oown), ptr(o8), ptr(n8), C.c_uint32(count), ptr(out["owner"]), ptr(out["records"]), ms,
                   ptr(out["carried"]), ptr(out["carried_weight"]), st)
        out["motion_stats"], out["stats"] = tuple(int(x) for x in ms), tuple(int(x) for x in st)
        return out

    def mesh_shutter_key(self, mesh, which):
        """lumc_mesh_shutter_key: the mesh's vertices as the device holds them become its open (0) or close (1) key."""
        self._call("lumc_mesh_shutter_key", C.c_uint32(mesh), C.c_uint32(which))

    def mesh_shutter_drop(self, mesh):
        self._call("lumc_mesh_shutter_drop", C.c_uint32(mesh))

    def shutter_time(self, t):
        """lumc_shutter_time: t in [0, 1] for every mesh that holds both keys; pending until the next update with DIRTY_MESH_SHUTTER."""
        self._call("lumc_shutter_time", C.c_float(t))

    def shutter_stats(self):
        out = ShutterStats()
        self._call("lumc_shutter_stats", C.byref(out))
        return out

    def set_light_refit(self, max_cost_growth=0.0):
        """lumc_set_light_refit: DIRTY_LIGHT_POSITIONS updates leave the lights alone (needs_rebuild) beyond this growth of the root's cost; 0: never for quality."""
        self._call("lumc_set_light_refit", C.c_float(max_cost_growth))

    def light_refit_bind(self, plan):
        """lumc_light_refit_bind: right after an update that took DIRTY_LIGHTS, the plan of the light tree it uploaded (Host.light_refit_plan)."""
        self._call("lumc_light_refit_bind", C.byref(plan))

    def light_refit_transforms(self, transforms):
        """lumc_light_refit_transforms: the plan's transform table again [t, 10] (moved instances); pending until the next DIRTY_LIGHT_POSITIONS update."""
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 10)
        self._call("lumc_light_refit_transforms", C.c_void_p(t.ctypes.data), C.c_uint32(len(t)))

    def light_refit_needs_rebuild(self):
        fn = self._lib.lumc_light_refit_needs_rebuild
        fn.restype = C.c_int
        return bool(fn(self._ctx))

    def light_refit_stats(self):
        out = LightRefitStats()
        self._call("lumc_light_refit_stats", C.byref(out))
        return out

    def light_arrays_probe(self):
        """lumc_light_arrays_probe: the light structures as the device holds them: a dict of root (uint8), root_children (float32), nodes (uint8 [n, 64]), table
        ([lights, 16] uint32 words), bvh_nodes ([n, 32] uint32 words), bvh_tris ([n, 12] uint32 words)."""
        sizes = (C.c_uint64 * 6)()
        null = C.c_void_p(0)
        self._call("lumc_light_arrays_probe", sizes, null, null, null, null, null, null)
        out = {"root": np.zeros(int(sizes[0]), np.uint8), "root_children": np.zeros(int(sizes[1]), np.float32), "nodes": np.zeros((int(sizes[2]) // 64, 64), np.uint8),
               "table": np.zeros((int(sizes[3]) // 4, 16), np.uint32), "bvh_nodes": np.zeros((int(sizes[4]), 32), np.uint32), "bvh_tris": np.zeros((int(sizes[5]), 12), np.uint32)}
        self._call("lumc_light_arrays_probe", sizes, *[_addr(out[k]) for k in ("root", "root_children", "nodes", "table", "bvh_nodes", "bvh_tris")])
        return out

    def mesh_vertices_probe(self, mesh, triangles):
        """lumc_mesh_vertices_probe: the mesh's [3 * triangles, 4] vertex records as uint32 words, from the device."""
        out = np.zeros((3 * triangles, 4), np.uint32)
        self._call("lumc_mesh_vertices_probe", C.c_uint32(mesh), C.c_void_p(out.ctypes.data))
        return out

    def resident_mesh_nodes_probe(self):
        """lumc_resident_mesh_nodes_probe: the nodes of [C, C + M) of the resident layout as [M, 32] uint32 words (24 box floats, 4 child words, 4 of padding)."""
        sizes = (C.c_uint64 * 5)()
        self._call("lumc_resident_tree_probe", sizes, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
        nodes = np.zeros((int(sizes[1]), 32), np.uint32)
        self._call("lumc_resident_mesh_nodes_probe", nodes.ctypes.data_as(C.c_void_p))
        return nodes

    def resident_tree_probe(self, num_instances, num_meshes):
        """lumc_resident_tree_probe: a dict of the resident layout after a device update: C, M, T, depth, top [C, 32] uint32 words (24 box floats, 4 child words, 4 of
        padding), leaves [records, 4, 4] uint32 words (one record of padding included), mesh_root [num_meshes], mesh_hash."""
        sizes, h = (C.c_uint64 * 5)(), C.c_uint64()
        self._call("lumc_resident_tree_probe", sizes, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
        top, leaves = np.zeros((int(sizes[0]), 32), np.uint32), np.zeros((num_instances + 1, 4, 4), np.uint32)
        roots = np.zeros(max(num_meshes, 1), np.uint32)
        self._call("lumc_resident_tree_probe", sizes, top.ctypes.data_as(C.c_void_p), leaves.ctypes.data_as(C.c_void_p), roots.ctypes.data_as(C.c_void_p), C.byref(h))
        return {"C": int(sizes[0]), "M": int(sizes[1]), "T": int(sizes[2]), "depth": int(sizes[4]), "top": top, "leaves": leaves[:int(sizes[3])].copy(),
                "mesh_root": roots[:num_meshes].copy(), "mesh_hash": int(h.value)}

    def bvh_build_seconds(self):
        fn = self._lib.lumc_bvh_build_seconds
        fn.restype = C.c_double
        return float(fn(self._ctx))

    def bvh_meshes_by_builder(self):
        out = (C.c_uint32 * 2)()
        self._call("lumc_bvh_meshes_by_builder", out)
        return {"sah": int(out[0]), "lbvh": int(out[1])}

    def bvh_stats(self):
        out = (C.c_uint64 * 4)()
        self._call("lumc_bvh_stats", out)
        return [int(x) for x in out]

    def trace_closest_host(self, origins, dirs, ignore=None):
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        n = origins.shape[0]
        out = np.zeros((n, 3), dtype=np.uint32)
        ip = C.c_void_p(0)
        if ignore is not None:
            ignore = np.ascontiguousarray(ignore, dtype=np.uint32)
            ip = ignore.ctypes.data_as(C.c_void_p)
        self._call("lumc_trace_closest_host", C.c_uint32(n), origins.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p), ip,
                   out.ctypes.data_as(C.c_void_p))
        return out

    def trace_visibility_host(self, origins, dirs, dist, ids, order=None):
        """Visibility rays through the active flavour's k_shadow_rays: [n, 3] float32 transparency products (0 = blocked; NaN = a ray nobody answered).
        ids [n, 4]: target instance, target triangle, self instance, self triangle (0xFFFFFFFF: none); order: the item every work slot traces, or None."""
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        dist = np.ascontiguousarray(dist, dtype=np.float32)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n = origins.shape[0]
        assert origins.shape == dirs.shape == (n, 3) and dist.shape == (n,) and ids.shape == (n, 4)
        out = np.zeros((n, 3), dtype=np.float32)
        op = C.c_void_p(0)
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            assert order.shape == (n,)
            op = order.ctypes.data_as(C.c_void_p)
        self._call("lumc_trace_visibility_host", C.c_uint32(n), origins.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p),
                   ids.ctypes.data_as(C.c_void_p), op, out.ctypes.data_as(C.c_void_p))
        return out

    def last_pass_path_counts(self, depths=64):
        """The number of paths every depth of the last pass held (lumc_last_pass_path_counts): a list, depth 0 first, 0 beyond the scene's depth limit"""
        out = (C.c_uint32 * depths)()
        self._call("lumc_last_pass_path_counts", C.c_uint32(depths), out)
        return [int(x) for x in out]

    PARTICLE_PROBE_UNTOUCHED = 0xFFFFFFFF

    def trace_particles_probe(self, origins, dirs, tmax, states, pixel_samples):
        """Caller-made queue entries through the active flavour's k_trace_particles (lumc_trace_particles_probe_host): world origins and directions [n, 3],
        tmax [n], state words [n] (bit 0: a delta path - the others are not traced), pixel x, pixel y and sample id [n, 3]. Returns (t [n] float32: tmax where
        nothing nearer was hit; hit [n] uint32: PARTICLE_PROBE_UNTOUCHED, or 0x80000000 + the particle's index)."""
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        states = np.ascontiguousarray(states, dtype=np.uint32)
        pixel_samples = np.ascontiguousarray(pixel_samples, dtype=np.uint32)
        n = origins.shape[0]
        assert origins.shape == dirs.shape == pixel_samples.shape == (n, 3) and tmax.shape == states.shape == (n,)
        t, hit = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint32)
        self._call("lumc_trace_particles_probe_host", C.c_uint32(n), origins.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p), tmax.ctypes.data_as(C.c_void_p),
                   states.ctypes.data_as(C.c_void_p), pixel_samples.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), hit.ctypes.data_as(C.c_void_p))
        return t, hit

    def light_query_host(self, origins, dirs, self_handles, randoms):
        """The light-BVH query of BSDF-sampled directions on plain rays: (light ids [n] uint32, 0xFFFFFFFF = none; num_hits [n] uint32)."""
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        self_handles = np.ascontiguousarray(self_handles, dtype=np.uint32)
        randoms = np.ascontiguousarray(randoms, dtype=np.float32)
        n = origins.shape[0]
        assert origins.shape == dirs.shape == (n, 3) and self_handles.shape == (n, 2) and randoms.shape == (n,)
        ids, hits = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._call("lumc_light_query_host", C.c_uint32(n), origins.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p), self_handles.ctypes.data_as(C.c_void_p),
                   randoms.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p))
        return ids, hits

    LIGHT_PROBE_VERTEX_WORDS, LIGHT_PROBE_WORDS = 20, 154
    LIGHT_PROBE_FORMS = {"general": 0, "plain": 1, "unstaged": 2}

    def light_sample_probe_host(self, vertices, first_sample, samples, form="general"):
        """sample_light on caller-made vertices (lumc_light_sample_probe_host): vertices [V, 20] uint32 words, out [V, samples, 154] uint32 words - the sample, the
        root pass and the eight lanes' stages as include/lum_core.h lays them out."""
        vertices = np.ascontiguousarray(vertices, dtype=np.uint32)
        nv = vertices.shape[0]
        assert vertices.shape == (nv, self.LIGHT_PROBE_VERTEX_WORDS)
        out = np.zeros((nv, samples, self.LIGHT_PROBE_WORDS), dtype=np.uint32)
        self._call("lumc_light_sample_probe_host", C.c_uint32(nv), vertices.ctypes.data_as(C.c_void_p), C.c_uint32(first_sample), C.c_uint32(samples),
                   C.c_int(self.LIGHT_PROBE_FORMS[form]), out.ctypes.data_as(C.c_void_p))
        return out

    BOUNCE_PROBE_WORDS, BOUNCE_PROBE_HEAD_WORDS, BOUNCE_PROBE_TECH_WORDS, BOUNCE_PROBE_LIGHT_DIR_WORDS = 143, 44, 24, 27

    def bounce_probe_host(self, vertices, first_sample, samples):
        """sample_bounce and sample_light_direction on caller-made vertices (lumc_bounce_probe_host): vertices [V, 20] uint32 words, out [V, samples, 143] uint32
        words - the two samples, the shading frame and the stages of every technique as include/lum_core.h lays them out."""
        vertices = np.ascontiguousarray(vertices, dtype=np.uint32)
        nv = vertices.shape[0]
        assert vertices.shape == (nv, self.LIGHT_PROBE_VERTEX_WORDS)
        out = np.zeros((nv, samples, self.BOUNCE_PROBE_WORDS), dtype=np.uint32)
        self._call("lumc_bounce_probe_host", C.c_uint32(nv), vertices.ctypes.data_as(C.c_void_p), C.c_uint32(first_sample), C.c_uint32(samples),
                   out.ctypes.data_as(C.c_void_p))
        return out

    SKY_PROBE_RAY_WORDS, SKY_PROBE_WORDS, SKY_PROBE_HEAD_WORDS, SKY_PROBE_STEP_WORDS, SKY_PROBE_MAX_STEPS = 12, 628, 40, 49, 12

    def sky_probe(self, rays):
        """sky_get_color / sky_trace_inscattering on caller-made rays (lumc_sky_probe_host): rays [N, 12] uint32 words, out [N, 628] uint32 words - the path, the
        march's stages, the celestial bodies' hits and the colour as include/lum_core.h lays them out."""
        rays = np.ascontiguousarray(rays, dtype=np.uint32)
        n = rays.shape[0]
        assert rays.shape == (n, self.SKY_PROBE_RAY_WORDS)
        out = np.zeros((n, self.SKY_PROBE_WORDS), dtype=np.uint32)
        self._call("lumc_sky_probe_host", C.c_uint32(n), rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out

    SUN_PROBE_WORDS = 64

    def sun_probe(self, vertices, first_sample, samples):
        """sample_sun on caller-made vertices (lumc_sun_probe_host): vertices [V, 20] uint32 words, out [V, samples, 64] uint32 words as include/lum_core.h lays them out"""
        vertices = np.ascontiguousarray(vertices, dtype=np.uint32)
        nv = vertices.shape[0]
        assert vertices.shape == (nv, self.LIGHT_PROBE_VERTEX_WORDS)
        out = np.zeros((nv, samples, self.SUN_PROBE_WORDS), dtype=np.uint32)
        self._call("lumc_sun_probe_host", C.c_uint32(nv), vertices.ctypes.data_as(C.c_void_p), C.c_uint32(first_sample), C.c_uint32(samples), out.ctypes.data_as(C.c_void_p))
        return out

    def sky_math_probe(self, op, x):
        """v_exp_f32 ("exp2"), v_sin_f32 ("sin") or v_cos_f32 ("cos") of float32 arguments (lumc_sky_math_probe_host); sin and cos take revolutions"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.zeros_like(x)
        self._call("lumc_sky_math_probe_host", C.c_uint32({"exp2": 0, "sin": 1, "cos": 2}[op]), C.c_uint32(x.size), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p))
        return y

    def trace_closest_device(self, n, origins_ptr, dirs_ptr, ignore_ptr, out_ptr, stream=0):
        self._call("lumc_trace_closest", C.c_uint32(n), C.c_void_p(origins_ptr), C.c_void_p(dirs_ptr), C.c_void_p(ignore_ptr), C.c_void_p(out_ptr),
                   C.c_void_p(stream))


def scene_view_sizeof():
    fn = _lib().lumc_scene_view_sizeof
    fn.restype = C.c_uint32
    return fn()


def undersampling_schedule(undersampling):
    """(stage, iteration) of every render iteration of the first sample, in order (device.c:392-420, :1298-1307): stage N four
    times (iterations 3, 2, 1, 0), every finer stage three times (2, 1, 0). Empty for undersampling 0."""
    out = []
    for stage in range(undersampling, 0, -1):
        out += [(stage, it) for it in ((3, 2, 1, 0) if stage == undersampling else (2, 1, 0))]
    return out
