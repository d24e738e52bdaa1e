"""luminary_amd - Python host-side mirror of the Luminary C host API for the MI355X path-tracing core.

The product is libluminary_amd.so (HIP kernels + C ABI, see include/luminary_amd.h and include/lum_core.h). This package is a
thin ctypes binding with the same names and argument meaning as the reference's `luminary_host_*` functions
(/root/reference/include/luminary/host.h:29-129) plus the additive `luminary_ext_*` functions. There is no CPU rendering path:
rendering calls raise `LuminaryError` when no HIP device is usable.
"""
import ctypes as C
import os

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
# LUM_LIB: an experiment variant built here with `python -m luminary_amd.build --variant NAME` (luminary_amd/lib/variants/NAME/), for A/B runs on the GPU box
LIB_PATH = os.environ.get("LUM_LIB") or os.path.join(_HERE, "lib", "libluminary_amd.so")


class LuminaryError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__("%s failed: %s (code %d)" % (what, _lib().luminary_result_to_string(C.c_uint64(code)).decode(), code & 0xFFFF))


# ---- PODs (include/luminary_amd.h; reference include/luminary/structs.h:29-391) ----
class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class RGBF(C.Structure):
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float)]


class RGBAF(C.Structure):
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("a", C.c_float)]


class HostCreateInfo(C.Structure):
    _fields_ = [("device_mask", C.c_uint32)]


class RendererSettings(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_ray_depth", C.c_uint32), ("bridge_max_num_vertices", C.c_uint32),
                ("undersampling", C.c_uint32), ("supersampling", C.c_uint32), ("enable_adaptive_sampling", C.c_bool),
                ("adaptive_sampling_max_sampling_rate", C.c_uint32), ("adaptive_sampling_avg_sampling_rate", C.c_uint32),
                ("adaptive_sampling_update_interval", C.c_uint32), ("adaptive_sampling_exposure_aware", C.c_bool),
                ("adaptive_sampling_output_mode", C.c_int), ("shading_mode", C.c_int), ("region_x", C.c_float), ("region_y", C.c_float),
                ("region_width", C.c_float), ("region_height", C.c_float)]


class _ThinLens(C.Structure):
    _fields_ = [("fov", C.c_float), ("aperture_size", C.c_float)]


class _Physical(C.Structure):
    _fields_ = [("allow_reflections", C.c_bool), ("use_spectral_rendering", C.c_bool)] + [(n, C.c_float) for n in (
        "focal_length", "front_focal_point", "back_focal_point", "front_principal_point", "back_principal_point", "aperture_point",
        "aperture_diameter", "exit_pupil_point", "exit_pupil_diameter", "image_plane_distance", "sensor_width")]


class Camera(C.Structure):
    _fields_ = [("pos", Vec3), ("rotation", Vec3), ("aperture_shape", C.c_int), ("aperture_blade_count", C.c_uint32), ("exposure", C.c_float),
                ("tonemap", C.c_int), ("agx_custom_slope", C.c_float), ("agx_custom_power", C.c_float), ("agx_custom_saturation", C.c_float),
                ("filter", C.c_int), ("use_local_error_minimization", C.c_bool), ("bloom_blend", C.c_float), ("dithering", C.c_bool),
                ("purkinje", C.c_bool), ("purkinje_kappa1", C.c_float), ("purkinje_kappa2", C.c_float), ("wasd_speed", C.c_float),
                ("mouse_speed", C.c_float), ("smooth_movement", C.c_bool), ("smoothing_factor", C.c_float),
                ("russian_roulette_threshold", C.c_float), ("use_color_correction", C.c_bool), ("color_correction", RGBF),
                ("film_grain", C.c_float), ("camera_scale", C.c_float), ("object_distance", C.c_float), ("use_physical_camera", C.c_bool),
                ("thin_lens", _ThinLens), ("physical", _Physical)]


LENS_MAX_INTERFACES = 24  # LUMINARY_CAMERA_LENS_MAX_INTERFACES


class LensInterface(C.Structure):
    _fields_ = [("radius", C.c_float), ("vertex", C.c_float), ("cylindrical_radius", C.c_float)]


class LensMedium(C.Structure):
    _fields_ = [("design_ior", C.c_float), ("abbe", C.c_float), ("cylindrical_radius", C.c_float)]


class CameraLens(C.Structure):
    """include/luminary_amd.h LuminaryCameraLens: the physical camera's interfaces (sensor side first) and the num_interfaces + 1 media around them."""
    _fields_ = [("num_interfaces", C.c_uint32), ("interfaces", LensInterface * LENS_MAX_INTERFACES), ("media", LensMedium * (LENS_MAX_INTERFACES + 1))]


class DenoiserSettings(C.Structure):
    """include/luminary_amd.h LuminaryDenoiserSettings (defaults: off, 4 guide samples, 5 iterations, sigmas 4 / 128 / 1)."""
    _fields_ = [("enabled", C.c_bool), ("guide_samples", C.c_uint32), ("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float)]


class Sky(C.Structure):
    _fields_ = [("geometry_offset", Vec3)] + [(n, C.c_float) for n in ("azimuth", "altitude", "moon_azimuth", "moon_altitude", "moon_tex_offset",
                                                                       "sun_strength", "base_density")] + \
               [("ozone_absorption", C.c_bool), ("steps", C.c_uint32), ("stars_count", C.c_uint32), ("stars_seed", C.c_uint32)] + \
               [(n, C.c_float) for n in ("stars_intensity", "rayleigh_density", "mie_density", "ozone_density", "rayleigh_falloff", "mie_falloff",
                                         "mie_diameter", "ground_visibility", "ozone_layer_thickness", "multiscattering_factor")] + \
               [("hdri_dim", C.c_uint32), ("hdri_samples", C.c_uint32), ("aerial_perspective", C.c_bool), ("constant_color", RGBF), ("mode", C.c_int)]


class Fog(C.Structure):
    """LuminaryFog (include/luminary_amd.h): a homogeneous scattering volume around the camera (fog.c:6-16 for the defaults)."""
    _fields_ = [("active", C.c_bool), ("density", C.c_float), ("droplet_diameter", C.c_float), ("height", C.c_float), ("dist", C.c_float)]


class Ocean(C.Structure):
    """LuminaryOcean (include/luminary_amd.h; defaults ocean.c:6-22)."""
    _fields_ = [("active", C.c_bool), ("height", C.c_float), ("amplitude", C.c_float), ("frequency", C.c_float), ("refractive_index", C.c_float),
                ("water_type", C.c_int), ("caustics_active", C.c_bool), ("caustics_ris_sample_count", C.c_uint32), ("caustics_domain_scale", C.c_float),
                ("multiscattering", C.c_bool), ("triangle_light_contribution", C.c_bool)]


class CloudLayer(C.Structure):
    _fields_ = [("active", C.c_bool), ("height_max", C.c_float), ("height_min", C.c_float), ("coverage", C.c_float), ("coverage_min", C.c_float),
                ("type", C.c_float), ("type_min", C.c_float), ("wind_speed", C.c_float), ("wind_angle", C.c_float)]


class Cloud(C.Structure):
    """LuminaryCloud (include/luminary_amd.h; defaults cloud.c:6-52)."""
    _fields_ = [("active", C.c_bool), ("initialized", C.c_bool), ("atmosphere_scattering", C.c_bool), ("low", CloudLayer), ("mid", CloudLayer),
                ("top", CloudLayer), ("offset_x", C.c_float), ("offset_z", C.c_float), ("density", C.c_float), ("seed", C.c_uint32),
                ("droplet_diameter", C.c_float), ("steps", C.c_uint32), ("shadow_steps", C.c_uint32), ("noise_shape_scale", C.c_float),
                ("noise_detail_scale", C.c_float), ("noise_weather_scale", C.c_float), ("mipmap_bias", C.c_float), ("octaves", C.c_uint32)]


class Particles(C.Structure):
    """LuminaryParticles (include/luminary_amd.h; defaults particles.c:6-24)."""
    _fields_ = [("active", C.c_bool), ("seed", C.c_uint32), ("count", C.c_uint32), ("albedo", RGBF), ("speed", C.c_float), ("direction_altitude", C.c_float),
                ("direction_azimuth", C.c_float), ("phase_diameter", C.c_float), ("scale", C.c_float), ("size", C.c_float), ("size_variation", C.c_float)]


class Material(C.Structure):
    _fields_ = [("id", C.c_uint32), ("base_substrate", C.c_int), ("albedo", RGBAF), ("emission", RGBF), ("emission_scale", C.c_float),
                ("roughness", C.c_float), ("roughness_clamp", C.c_float), ("refraction_index", C.c_float), ("emission_active", C.c_bool),
                ("thin_walled", C.c_bool), ("metallic", C.c_bool), ("colored_transparency", C.c_bool), ("roughness_as_smoothness", C.c_bool),
                ("normal_map_is_compressed", C.c_bool), ("bidirectional_emission", C.c_bool), ("albedo_tex", C.c_uint16),
                ("luminance_tex", C.c_uint16), ("roughness_tex", C.c_uint16), ("metallic_tex", C.c_uint16), ("normal_tex", C.c_uint16)]


class PixelQueryResult(C.Structure):
    _fields_ = [("pixel_query_is_valid", C.c_bool), ("instance_id", C.c_uint32), ("material_id", C.c_uint16), ("depth", C.c_float), ("rel_hit_pos", Vec3)]


class DeviceInfo(C.Structure):
    _fields_ = [("is_main_device", C.c_bool), ("is_unavailable", C.c_bool), ("is_enabled", C.c_bool), ("name", C.c_char * 256), ("memory_size", C.c_size_t),
                ("allocated_memory_size", C.c_size_t)]


class OutputProperties(C.Structure):
    _fields_ = [("enabled", C.c_bool), ("width", C.c_uint32), ("height", C.c_uint32)]


class OutputRequestProperties(C.Structure):
    _fields_ = [("sample_count", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class Image(C.Structure):
    _fields_ = [("buffer", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("ld", C.c_size_t), ("time", C.c_float), ("sample_count", C.c_uint32)]


OUTPUT_HANDLE_INVALID = 0xFFFFFFFF


class MeshRefitStats(C.Structure):
    """LuminaryMeshRefitStats"""
    _fields_ = [("refits", C.c_uint64), ("rebuilds", C.c_uint64), ("last_refits", C.c_uint32), ("last_rebuilds", C.c_uint32), ("max_cost_growth", C.c_double),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_refit", C.c_double), ("seconds_rebuild", C.c_double), ("seconds_assemble", C.c_double),
                ("seconds_hash", C.c_double), ("seconds_download", C.c_double), ("seconds_lights", C.c_double)]


class InstanceUpdateStats(C.Structure):
    """LuminaryInstanceUpdateStats"""
    _fields_ = [("device_updates", C.c_uint64), ("fallbacks", C.c_uint64), ("relayouts", C.c_uint64), ("tlas_nodes", C.c_uint32), ("tlas_depth", C.c_uint32),
                ("tlas_capacity", C.c_uint32), ("hittable", C.c_uint32), ("seconds", C.c_double), ("seconds_relayout", C.c_double), ("seconds_upload", C.c_double),
                ("seconds_boxes", C.c_double), ("seconds_build", C.c_double), ("seconds_leaves", C.c_double)]


class ResidentRefitStats(C.Structure):
    """LuminaryResidentRefitStats"""
    _fields_ = [("updates", C.c_uint64), ("fallbacks", C.c_uint64), ("last_meshes", C.c_uint32), ("last_launches", C.c_uint32), ("last_bytes_downloaded", C.c_uint64),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_hash", C.c_double), ("seconds_refit", C.c_double), ("seconds_cost", C.c_double),
                ("seconds_top_level", C.c_double)]


class LightRefitStats(C.Structure):
    """LuminaryLightRefitStats"""
    _fields_ = [("refits", C.c_uint64), ("fallbacks", C.c_uint64), ("last_launches", C.c_uint32), ("last_flags", C.c_uint32), ("last_bytes_uploaded", C.c_uint64),
                ("last_bytes_downloaded", C.c_uint64), ("seconds", C.c_double), ("seconds_fragments", C.c_double), ("seconds_stats", C.c_double), ("seconds_nodes", C.c_double),
                ("seconds_light_bvh", C.c_double), ("seconds_table", C.c_double), ("cost_growth", C.c_double), ("host_rebuilds", C.c_uint64)]


class MeshSkinStats(C.Structure):
    """LuminaryMeshSkinStats"""
    _fields_ = [("poses", C.c_uint64), ("rebuild_downloads", C.c_uint64), ("last_meshes", C.c_uint32), ("last_launches", C.c_uint32), ("last_bytes_uploaded", C.c_uint64),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_skin", C.c_double), ("host_materialisations", C.c_uint64)]


class MeshMorphStats(C.Structure):
    """LuminaryMeshMorphStats"""
    _fields_ = [("applied", C.c_uint64), ("rebuild_downloads", C.c_uint64), ("last_meshes", C.c_uint32), ("last_launches", C.c_uint32), ("last_bytes_uploaded", C.c_uint64),
                ("seconds", C.c_double), ("seconds_upload", C.c_double), ("seconds_morph", C.c_double), ("host_materialisations", C.c_uint64)]


class FireflySettings(C.Structure):
    """include/luminary_amd.h LuminaryFireflySettings (defaults: off, 8 buckets)."""
    _fields_ = [("enabled", C.c_bool), ("buckets", C.c_uint32)]


class FireflyStats(C.Structure):
    """LuminaryFireflyStats"""
    _fields_ = [("frames_resolved", C.c_uint64), ("frames_skipped", C.c_uint64), ("last_rewritten", C.c_uint32), ("last_trimmed", C.c_uint32),
                ("last_nonfinite", C.c_uint32), ("buckets", C.c_uint32), ("bytes", C.c_uint64)]


class MatteStats(C.Structure):
    """LuminaryMatteStats"""
    _fields_ = [("renders", C.c_uint64), ("bytes", C.c_uint64), ("valid", C.c_uint32), ("samples", C.c_uint32), ("layers", C.c_uint32),
                ("dropped_pixels", C.c_uint32 * 2), ("reserved", C.c_uint32), ("seconds", C.c_double)]


class HistorySettings(C.Structure):
    """include/luminary_amd.h LuminaryHistorySettings (defaults: off, 32, 0.02, 0.9, no clamp)."""
    _fields_ = [("enabled", C.c_bool), ("max_history", C.c_float), ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("clamp_sigma", C.c_float)]


class HistoryStats(C.Structure):
    """LuminaryHistoryStats"""
    _fields_ = [("frames_carried", C.c_uint64), ("frames_dropped", C.c_uint64), ("frames_skipped", C.c_uint64), ("last_carried", C.c_uint32), ("last_rejected", C.c_uint32),
                ("last_off", C.c_uint32), ("valid", C.c_uint32), ("bytes", C.c_uint64), ("seconds", C.c_double), ("last_drop", C.c_char * 96)]


class HistoryMotionSettings(C.Structure):
    """include/luminary_amd.h LuminaryHistoryMotionSettings (defaults: off, 8)."""
    _fields_ = [("enabled", C.c_bool), ("motion_max_history", C.c_float)]


class HistoryMotionStats(C.Structure):
    """LuminaryHistoryMotionStats"""
    _fields_ = [("frames_carried", C.c_uint64), ("bytes", C.c_uint64), ("instances_moved", C.c_uint32), ("instances_same", C.c_uint32), ("instances_void", C.c_uint32),
                ("last_moved_pixels", C.c_uint32), ("last_moved_carried", C.c_uint32), ("valid", C.c_uint32), ("owner_seconds", C.c_double), ("motion_seconds", C.c_double),
                ("reproject_seconds", C.c_double)]


MATTE_LAYER_INSTANCE, MATTE_LAYER_MATERIAL = 1, 2  # LUMINARY_MATTE_LAYER_*
MATTE_ID_EMPTY, MATTE_ID_MISS, MATTE_ID_OCEAN, MATTE_ID_PARTICLE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC  # LUMINARY_MATTE_ID_*


class ShutterStats(C.Structure):
    """LuminaryShutterStats"""
    _fields_ = [("renders", C.c_uint64), ("slices", C.c_uint64), ("last_moved_meshes", C.c_uint32), ("last_moved_instances", C.c_uint32), ("last_camera_moved", C.c_uint32),
                ("last_slices", C.c_uint32), ("seconds_update", C.c_double), ("seconds_render", C.c_double)]


class Instance(C.Structure):
    _fields_ = [("id", C.c_uint32), ("mesh_id", C.c_uint32), ("position", Vec3), ("rotation", Vec3), ("scale", Vec3)]


class DeviceSceneView(C.Structure):
    """include/lum_core.h LumDeviceSceneView == oracle/oracle.h OracleScene."""
    _fields_ = [("num_meshes", C.c_uint32), ("num_instances", C.c_uint32), ("num_materials", C.c_uint32), ("num_lights", C.c_uint32),
                ("mesh_tri_offset", C.c_void_p), ("vertices", C.c_void_p), ("tri_tex", C.c_void_p), ("instance_mesh_ids", C.c_void_p),
                ("instance_transforms", C.c_void_p), ("materials", C.c_void_p), ("light_tree_root", C.c_void_p), ("light_tree_nodes", C.c_void_p),
                ("light_tri_handles", C.c_void_p), ("light_bvh_tris", C.c_void_p), ("num_light_tree_nodes", C.c_uint32), ("num_textures", C.c_uint32),
                ("bluenoise_2d", C.c_void_p), ("lut_conductor", C.c_void_p), ("lut_glossy", C.c_void_p), ("lut_dielectric", C.c_void_p),
                ("lut_dielectric_inv", C.c_void_p), ("texture_table", C.c_void_p), ("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("max_ray_depth", C.c_uint32),
                ("shading_mode", C.c_uint32), ("cam_pos", C.c_float * 3), ("cam_rotation", C.c_float * 4), ("cam_fov", C.c_float),
                ("cam_aperture_size", C.c_float), ("cam_object_distance", C.c_float), ("cam_scale", C.c_float), ("cam_rr_threshold", C.c_float),
                ("cam_aperture_shape", C.c_uint32), ("cam_aperture_blade_count", C.c_uint32), ("sky_mode", C.c_uint32),
                ("sky_constant_color", C.c_float * 3),
                ("sky_steps", C.c_uint32), ("sky_ozone_absorption", C.c_uint32), ("sky_geometry_offset", C.c_float * 3), ("sky_sun_strength", C.c_float),
                ("sky_base_density", C.c_float), ("sky_rayleigh_density", C.c_float), ("sky_mie_density", C.c_float), ("sky_ozone_density", C.c_float),
                ("sky_rayleigh_falloff", C.c_float), ("sky_mie_falloff", C.c_float), ("sky_ground_visibility", C.c_float),
                ("sky_ozone_layer_thickness", C.c_float), ("sky_multiscattering_factor", C.c_float), ("sky_sun_pos", C.c_float * 3),
                ("sky_mie_phase", C.c_float * 4), ("sky_lut_transmittance", C.c_void_p), ("sky_lut_multiscattering", C.c_void_p),
                ("sky_moon_pos", C.c_float * 3), ("sky_moon_tex_offset", C.c_float), ("sky_moon_albedo_tex", C.c_uint32), ("sky_moon_normal_tex", C.c_uint32),
                ("sky_stars_intensity", C.c_float), ("sky_stars_count", C.c_uint32), ("sky_stars", C.c_void_p), ("sky_stars_offsets", C.c_void_p),
                ("sky_hdri", C.c_void_p), ("sky_hdri_dim", C.c_uint32), ("sky_hdri_samples", C.c_uint32), ("sky_hdri_origin", C.c_float * 3), ("sky_aerial_perspective", C.c_uint32),
                ("fog_active", C.c_uint32), ("fog_density", C.c_float), ("fog_dist", C.c_float), ("fog_height", C.c_float), ("fog_phase", C.c_float * 4),
                ("bridge_lut", C.c_void_p), ("bridge_max_num_vertices", C.c_uint32),
                ("particles_active", C.c_uint32), ("particles_count", C.c_uint32), ("particles_scale", C.c_float), ("particles_speed", C.c_float),
                ("particles_albedo", C.c_float * 3), ("particles_direction", C.c_float * 3), ("particles_phase", C.c_float * 4),
                ("particle_vertices", C.c_void_p), ("particle_normals", C.c_void_p),
                ("ocean_active", C.c_uint32), ("ocean_height", C.c_float), ("ocean_amplitude", C.c_float), ("ocean_frequency", C.c_float),
                ("ocean_refractive_index", C.c_float), ("ocean_scattering", C.c_float * 3), ("ocean_absorption", C.c_float * 3),
                ("ocean_molecular_weight", C.c_float), ("ocean_caustics_active", C.c_uint32), ("ocean_caustics_ris_sample_count", C.c_uint32),
                ("ocean_caustics_domain_scale", C.c_float), ("ocean_multiscattering", C.c_uint32), ("ocean_triangle_light_contribution", C.c_uint32),
                ("cloud_active", C.c_uint32), ("cloud_atmosphere_scattering", C.c_uint32), ("cloud_steps", C.c_uint32), ("cloud_shadow_steps", C.c_uint32),
                ("cloud_octaves", C.c_uint32), ("cloud_seed", C.c_uint32), ("cloud_offset_x", C.c_float), ("cloud_offset_z", C.c_float),
                ("cloud_density", C.c_float), ("cloud_noise_shape_scale", C.c_float), ("cloud_noise_detail_scale", C.c_float),
                ("cloud_noise_weather_scale", C.c_float), ("cloud_phase", C.c_float * 4), ("cloud_layers", (C.c_float * 10) * 3),
                ("cloud_noise_shape", C.c_void_p), ("cloud_noise_detail", C.c_void_p), ("cloud_noise_weather", C.c_void_p)]


SKY_MODE_DEFAULT, SKY_MODE_HDRI, SKY_MODE_CONSTANT_COLOR = 0, 1, 2
SUBSTRATE_OPAQUE, SUBSTRATE_TRANSLUCENT = 0, 1

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            _build.build()
        lib = C.CDLL(LIB_PATH)
        lib.luminary_result_to_string.restype = C.c_char_p
        lib.luminary_result_to_string.argtypes = [C.c_uint64]
        lib.luminary_ext_get_core_context.restype = C.c_void_p
        lib.lumc_last_error.restype = C.c_char_p
        lib.lumc_last_error.argtypes = [C.c_void_p]
        for name in dir(lib):
            pass
        _LIB = lib
    return _LIB


def _call(name, *args):
    fn = getattr(_lib(), name)
    fn.restype = C.c_uint64
    code = fn(*args)
    if code != 0:
        raise LuminaryError(code, name)


def _core_call(ctx, name, *args):
    fn = getattr(_lib(), name)
    fn.restype = C.c_int
    if fn(C.c_void_p(ctx), *args) != 0:
        raise RuntimeError("%s failed: %s" % (name, _lib().lumc_last_error(C.c_void_p(ctx)).decode()))


class Host:
    """Mirror of LuminaryHost (reference: src/luminary/host/host.c)."""

    def __init__(self, device_mask=0xFFFFFFFF):
        _lib().luminary_init()
        self._h = C.c_void_p()
        _call("luminary_host_create", C.byref(self._h), HostCreateInfo(device_mask))

    def close(self):
        if self._h:
            _call("luminary_host_destroy", C.byref(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _path(self, s):
        p = C.c_void_p()
        _call("luminary_path_create", C.byref(p))
        _call("luminary_path_set_from_string", p, s.encode())
        return p

    def load_lum_file(self, path):
        p = self._path(path)
        try:
            _call("luminary_host_load_lum_file", self._h, p)
        finally:
            _call("luminary_path_destroy", C.byref(p))

    def load_obj_file(self, path):
        p = self._path(path)
        try:
            _call("luminary_host_load_obj_file", self._h, p)
        finally:
            _call("luminary_path_destroy", C.byref(p))

    def _get(self, name, typ):
        v = typ()
        _call("luminary_host_get_" + name, self._h, C.byref(v))
        return v

    def get_settings(self):
        return self._get("settings", RendererSettings)

    def set_settings(self, s):
        _call("luminary_host_set_settings", self._h, C.byref(s))

    def get_camera(self):
        return self._get("camera", Camera)

    def set_camera(self, c):
        _call("luminary_host_set_camera", self._h, C.byref(c))

    def get_camera_lens(self):
        """luminary_ext_get_camera_lens: the physical camera's lens (default: the reference's double-Gauss prescription)"""
        lens = CameraLens()
        _call("luminary_ext_get_camera_lens", self._h, C.byref(lens))
        return lens

    def set_camera_lens(self, lens):
        """luminary_ext_set_camera_lens: restarts the integration while the camera is physical"""
        _call("luminary_ext_set_camera_lens", self._h, C.byref(lens))

    def get_sky(self):
        return self._get("sky", Sky)

    def set_sky(self, s):
        _call("luminary_host_set_sky", self._h, C.byref(s))

    def get_fog(self):
        return self._get("fog", Fog)

    def set_fog(self, f):
        _call("luminary_host_set_fog", self._h, C.byref(f))

    def get_ocean(self):
        return self._get("ocean", Ocean)

    def set_ocean(self, o):
        _call("luminary_host_set_ocean", self._h, C.byref(o))

    def get_cloud(self):
        return self._get("cloud", Cloud)

    def set_cloud(self, c):
        _call("luminary_host_set_cloud", self._h, C.byref(c))

    def get_particles(self):
        return self._get("particles", Particles)

    def set_particles(self, p):
        _call("luminary_host_set_particles", self._h, C.byref(p))

    def get_material(self, i):
        m = Material()
        _call("luminary_host_get_material", self._h, C.c_uint16(i), C.byref(m))
        return m

    def set_material(self, i, m):
        _call("luminary_host_set_material", self._h, C.c_uint16(i), C.byref(m))

    def new_instance(self, mesh_id, position=(0, 0, 0), rotation=(0, 0, 0), scale=(1, 1, 1)):
        inst = Instance()
        _call("luminary_host_new_instance", self._h, C.byref(inst))
        inst.mesh_id = mesh_id
        inst.position = Vec3(*position)
        inst.rotation = Vec3(*rotation)
        inst.scale = Vec3(*scale)
        _call("luminary_host_set_instance", self._h, C.byref(inst))
        return inst.id

    def get_instance(self, i):
        inst = Instance()
        _call("luminary_host_get_instance", self._h, C.c_uint32(i), C.byref(inst))
        return inst

    def set_instance(self, inst):
        _call("luminary_host_set_instance", self._h, C.byref(inst))

    def counts(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _call("luminary_host_get_num_meshes", self._h, C.byref(a))
        _call("luminary_host_get_num_materials", self._h, C.byref(b))
        _call("luminary_host_get_num_instances", self._h, C.byref(c))
        return a.value, b.value, c.value

    def get_pixel_info(self, x, y):
        r = PixelQueryResult()
        _call("luminary_host_get_pixel_info", self._h, C.c_uint16(x), C.c_uint16(y), C.byref(r))
        return r

    # ---- output chain ----
    def set_output_properties(self, width, height, enabled=True):
        _call("luminary_host_set_output_properties", self._h, OutputProperties(enabled, width, height))

    def request_output(self, sample_count, width, height):
        h = C.c_uint32()
        _call("luminary_host_request_output", self._h, OutputRequestProperties(sample_count, width, height), C.byref(h))
        return h.value

    def try_await_output(self, promise):
        h = C.c_uint32()
        _call("luminary_host_try_await_output", self._h, C.c_uint32(promise), C.byref(h))
        return None if h.value == OUTPUT_HANDLE_INVALID else h.value

    def acquire_output(self):
        h = C.c_uint32()
        _call("luminary_host_acquire_output", self._h, C.byref(h))
        return None if h.value == OUTPUT_HANDLE_INVALID else h.value

    def get_image(self, handle):
        """(ARGB8 words [height, width] as a copy, sample_count, time) of an acquired output."""
        import numpy as np
        img = Image()
        _call("luminary_host_get_image", self._h, C.c_uint32(handle), C.byref(img))
        words = np.ctypeslib.as_array(C.cast(img.buffer, C.POINTER(C.c_uint32)), shape=(img.height, img.ld))[:, :img.width].copy()
        return words, img.sample_count, img.time

    def release_output(self, handle):
        _call("luminary_host_release_output", self._h, C.c_uint32(handle))

    def save_png(self, handle, path):
        p = self._path(path)
        try:
            _call("luminary_host_save_png", self._h, C.c_uint32(handle), p)
        finally:
            _call("luminary_path_destroy", C.byref(p))

    def start_new_render(self):
        """Restarts the accumulation and starts the library's render thread (reference host.c:406-414); poll try_await_output /
        acquire_output for images."""
        _call("luminary_host_start_new_render", self._h)

    def get_num_meshes(self):
        n = C.c_uint32()
        _call("luminary_host_get_num_meshes", self._h, C.byref(n))
        return int(n.value)

    def get_num_materials(self):
        n = C.c_uint32()
        _call("luminary_host_get_num_materials", self._h, C.byref(n))
        return int(n.value)

    def get_num_instances(self):
        n = C.c_uint32()
        _call("luminary_host_get_num_instances", self._h, C.byref(n))
        return int(n.value)

    def get_device_count(self):
        n = C.c_uint32()
        _call("luminary_host_get_device_count", self._h, C.byref(n))
        return int(n.value)

    def get_device_info(self, device_id):
        info = DeviceInfo()
        _call("luminary_host_get_device_info", self._h, C.c_uint32(device_id), C.byref(info))
        return info

    def set_device_enable(self, device_id, enable):
        _call("luminary_host_set_device_enable", self._h, C.c_uint32(device_id), C.c_bool(enable))

    def stop_render(self):
        _call("luminary_ext_stop_render", self._h)

    def is_rendering(self):
        """(render thread active, samples accumulated so far)"""
        r, n = C.c_bool(), C.c_uint32()
        _call("luminary_ext_is_rendering", self._h, C.byref(r), C.byref(n))
        return bool(r.value), int(n.value)

    def queue_workers(self):
        """[(name, current task or None, seconds)] of the library's queue workers (reference host.c:615-703)."""
        n = C.c_uint32()
        _call("luminary_host_get_num_queue_workers", self._h, C.byref(n))
        out = []
        for i in range(n.value):
            name, string, t = C.c_char_p(), C.c_char_p(), C.c_double()
            _call("luminary_host_get_queue_worker_name", self._h, C.c_uint32(i), C.byref(name))
            _call("luminary_host_get_queue_worker_string", self._h, C.c_uint32(i), C.byref(string))
            _call("luminary_host_get_queue_worker_time", self._h, C.c_uint32(i), C.byref(t))
            out.append((name.value.decode() if name.value else None, string.value.decode() if string.value else None, float(t.value)))
        return out

    # ---- additive extension ----
    def add_mesh(self, positions, material_ids, normals=None, uvs=None):
        import numpy as np
        positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        material_ids = np.ascontiguousarray(material_ids, dtype=np.uint16).reshape(-1)
        n = material_ids.size
        assert positions.size == 9 * n
        npt = C.c_void_p(0)
        upt = C.c_void_p(0)
        if normals is not None:
            normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1)
            npt = normals.ctypes.data_as(C.c_void_p)
        if uvs is not None:
            uvs = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1)
            upt = uvs.ctypes.data_as(C.c_void_p)
        mid = C.c_uint32()
        _call("luminary_ext_add_mesh", self._h, positions.ctypes.data_as(C.c_void_p), npt, upt, material_ids.ctypes.data_as(C.c_void_p),
              C.c_uint32(n), C.byref(mid))
        return mid.value

    def set_mesh_positions(self, mesh_id, positions, normals=None):
        """luminary_ext_set_mesh_positions: new positions [n, 9] (and normals [n, 9], or None = face normals) for a mesh the host holds; the devices refit its tree."""
        import numpy as np
        positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        npt = C.c_void_p(0)
        if normals is not None:
            normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1)
            assert normals.size == positions.size
            npt = normals.ctypes.data_as(C.c_void_p)
        _call("luminary_ext_set_mesh_positions", self._h, C.c_uint32(mesh_id), positions.ctypes.data_as(C.c_void_p), npt, C.c_uint32(positions.size // 9))

    def set_mesh_refit(self, mode=0, max_cost_growth=0.0):
        """luminary_ext_set_mesh_refit: 0 = refit a moved mesh's tree, 1 = build it again; max_cost_growth > 0: build again when the cost grew beyond this factor."""
        _call("luminary_ext_set_mesh_refit", self._h, C.c_uint32(mode), C.c_float(max_cost_growth))

    def mesh_refit_stats(self):
        """luminary_ext_get_mesh_refit_stats of the main device: a dict of refits, rebuilds, last_refits, last_rebuilds, max_cost_growth and the seconds."""
        s = MeshRefitStats()
        _call("luminary_ext_get_mesh_refit_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def set_instance_transforms(self, instances):
        """luminary_ext_set_instance_transforms: new position / rotation / scale for existing instances, in bulk: a sequence of Instance (id and mesh_id as the
        host holds them); the devices rebuild the top-level tree, the mesh trees stay."""
        instances = list(instances)
        arr = (Instance * max(len(instances), 1))()
        for k, inst in enumerate(instances):
            arr[k] = inst
        _call("luminary_ext_set_instance_transforms", self._h, arr, C.c_uint32(len(instances)))

    def set_instance_update(self, mode=0):
        """luminary_ext_set_instance_update: 0 = moved instances are taken over on the device, 1 = the scene tree is assembled on the host and uploaded."""
        _call("luminary_ext_set_instance_update", self._h, C.c_uint32(mode))

    def instance_update_stats(self):
        """luminary_ext_get_instance_update_stats of the main device: a dict of device_updates, fallbacks, relayouts, the last top level's sizes and the seconds."""
        s = InstanceUpdateStats()
        _call("luminary_ext_get_instance_update_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def set_mesh_refit_in_place(self, on=1):
        """luminary_ext_set_mesh_refit_in_place: 1 = moved vertices, alone or in one frame with moved instances, are refitted in the devices' node arrays, which keep
        their layout; 0 (default) = in a copy of the mesh's tree, and the host assembles and uploads the node array again."""
        _call("luminary_ext_set_mesh_refit_in_place", self._h, C.c_uint32(on))

    def resident_refit_stats(self):
        """luminary_ext_get_resident_refit_stats of the main device: a dict of updates, fallbacks, the last update's meshes, launches, bytes downloaded and seconds."""
        s = ResidentRefitStats()
        _call("luminary_ext_get_resident_refit_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def bind_mesh_skin(self, mesh_id, bone_ids, weights, bone_count):
        """luminary_ext_bind_mesh_skin: bone ids and weights [n, 12] (four slots per corner) over bone_count bones; the rest pose is the host mesh as it is now."""
        import numpy as np
        ids = np.ascontiguousarray(bone_ids, dtype=np.uint16).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        assert ids.size == w.size and ids.size % 12 == 0
        _call("luminary_ext_bind_mesh_skin", self._h, C.c_uint32(mesh_id), ids.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), C.c_uint32(ids.size // 12), C.c_uint32(bone_count))

    def unbind_mesh_skin(self, mesh_id):
        """luminary_ext_unbind_mesh_skin: the host mesh becomes the current pose, and plain again."""
        _call("luminary_ext_unbind_mesh_skin", self._h, C.c_uint32(mesh_id))

    def set_mesh_pose(self, mesh_id, bones):
        """luminary_ext_set_mesh_pose: bones [b, 12], row-major 3 x 4; the devices pose the bound mesh's vertices and refit its tree."""
        import numpy as np
        b = np.ascontiguousarray(bones, dtype=np.float32).reshape(-1)
        assert b.size % 12 == 0
        _call("luminary_ext_set_mesh_pose", self._h, C.c_uint32(mesh_id), b.ctypes.data_as(C.c_void_p), C.c_uint32(b.size // 12))

    def mesh_skin_stats(self):
        """luminary_ext_get_mesh_skin_stats: the main device's skinning stats and host_materialisations, as a dict."""
        s = MeshSkinStats()
        _call("luminary_ext_get_mesh_skin_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def bind_mesh_morph(self, mesh_id, triangle_count, offsets, corners, delta_positions, delta_normals=None):
        """luminary_ext_bind_mesh_morph: sparse target-major deltas - offsets [T + 1] into corners [E], delta positions [E, 3], delta normals [E, 3] or None - over the
        host mesh of triangle_count triangles as it is now (or over the rest shape it shares with a bound skin); all weights 0."""
        import numpy as np
        o = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        c = np.ascontiguousarray(corners, dtype=np.uint32).reshape(-1)
        dp = np.ascontiguousarray(delta_positions, dtype=np.float32).reshape(-1)
        dn = None if delta_normals is None else np.ascontiguousarray(delta_normals, dtype=np.float32).reshape(-1)
        assert o.size >= 2 and dp.size == 3 * c.size and (dn is None or dn.size == dp.size) and int(o.max()) <= c.size
        _call("luminary_ext_bind_mesh_morph", self._h, C.c_uint32(mesh_id), C.c_uint32(triangle_count), C.c_uint32(o.size - 1), o.ctypes.data_as(C.c_void_p),
              c.ctypes.data_as(C.c_void_p), dp.ctypes.data_as(C.c_void_p), dn.ctypes.data_as(C.c_void_p) if dn is not None else C.c_void_p(0))

    def unbind_mesh_morph(self, mesh_id):
        """luminary_ext_unbind_mesh_morph: drops the targets; with no skin bound the host mesh becomes the current shape, and plain again."""
        _call("luminary_ext_unbind_mesh_morph", self._h, C.c_uint32(mesh_id))

    def set_mesh_weights(self, mesh_id, weights):
        """luminary_ext_set_mesh_weights: weights [T]; the devices blend the bound mesh's vertices and refit its tree."""
        import numpy as np
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        _call("luminary_ext_set_mesh_weights", self._h, C.c_uint32(mesh_id), w.ctypes.data_as(C.c_void_p), C.c_uint32(w.size))

    def mesh_morph_stats(self):
        """luminary_ext_get_mesh_morph_stats: the main device's morph stats and host_materialisations, as a dict."""
        s = MeshMorphStats()
        _call("luminary_ext_get_mesh_morph_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def get_mesh(self, mesh_id):
        """luminary_ext_get_mesh: the host-level mesh (copies): positions [n, 9], normals [n, 9], uvs [n, 6], material ids [n]."""
        import numpy as np
        p, nrm, uv, mat = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint16)()
        n = C.c_uint32()
        _call("luminary_ext_get_mesh", self._h, C.c_uint32(mesh_id), C.byref(p), C.byref(nrm), C.byref(uv), C.byref(mat), C.byref(n))
        n = n.value
        if n == 0:
            return np.zeros((0, 9), np.float32), np.zeros((0, 9), np.float32), np.zeros((0, 6), np.float32), np.zeros(0, np.uint16)
        return (np.ctypeslib.as_array(p, shape=(n, 9)).copy(), np.ctypeslib.as_array(nrm, shape=(n, 9)).copy(), np.ctypeslib.as_array(uv, shape=(n, 6)).copy(),
                np.ctypeslib.as_array(mat, shape=(n,)).copy())

    def add_texture(self, rgba8, gamma=1.0):
        """rgba8: uint8 array [height, width, 4]; returns the texture id for Material.albedo_tex / roughness_tex / normal_tex."""
        import numpy as np
        img = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert img.ndim == 3 and img.shape[2] == 4
        i = C.c_uint16()
        _call("luminary_ext_add_texture", self._h, img.ctypes.data_as(C.c_void_p), C.c_uint32(img.shape[1]), C.c_uint32(img.shape[0]), C.c_float(gamma),
              C.byref(i))
        return i.value

    def add_material(self, m):
        i = C.c_uint16()
        _call("luminary_ext_add_material", self._h, C.byref(m), C.byref(i))
        return i.value

    def device_scene(self):
        """Scene in the device format (valid until the next scene edit). Needs no GPU."""
        p = C.POINTER(DeviceSceneView)()
        _call("luminary_ext_build_device_scene", self._h, C.byref(p))
        view = p.contents
        view._owner = self  # the buffers behind the pointers live in the host
        return view

    def set_light_refit(self, on=1, max_cost_growth=0.0):
        """luminary_ext_set_light_refit: 1 = edits that move an emissive triangle refit the light tree on the devices instead of building it again on the host;
        max_cost_growth > 0: build again when the root's cost grew beyond this factor."""
        _call("luminary_ext_set_light_refit", self._h, C.c_uint32(on), C.c_float(max_cost_growth))

    def light_refit_stats(self):
        """luminary_ext_get_light_refit_stats: the main device's refit stats and host_rebuilds, as a dict."""
        s = LightRefitStats()
        _call("luminary_ext_get_light_refit_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def light_refit_plan(self):
        """luminary_ext_get_light_refit_plan: the core.LightRefitPlan of the light arrays of device_scene() (its pointers are valid until the host builds the light
        tree again; .copy() gives one that owns its arrays). Needs no GPU."""
        from .core import LightRefitPlan
        plan = LightRefitPlan()
        _call("luminary_ext_get_light_refit_plan", self._h, C.byref(plan))
        plan._owner = self
        return plan

    def render_samples(self, first_sample, num_samples, pixels=None, samples_per_pass=1):
        import numpy as np
        if pixels is None:
            _call("luminary_ext_render_samples", self._h, C.c_void_p(0), C.c_uint32(0), C.c_uint32(first_sample), C.c_uint32(num_samples),
                  C.c_uint32(samples_per_pass))
        else:
            px = np.ascontiguousarray(pixels, dtype=np.uint32)
            _call("luminary_ext_render_samples", self._h, px.ctypes.data_as(C.c_void_p), C.c_uint32(px.size), C.c_uint32(first_sample),
                  C.c_uint32(num_samples), C.c_uint32(samples_per_pass))

    def shutter_open(self):
        """luminary_ext_shutter_open: the scene as it stands is the open key of a motion-blurred render; moved vertices, poses, weights, instance transforms and
        camera pos / rotation set from now on define the close key."""
        _call("luminary_ext_shutter_open", self._h)

    def shutter_cancel(self):
        """luminary_ext_shutter_cancel"""
        _call("luminary_ext_shutter_cancel", self._h)

    def render_shutter(self, slices, samples_per_slice, samples_per_pass=1):
        """luminary_ext_render_shutter: `slices` temporal samples between the keys, `samples_per_slice` sample ids each, into the same accumulators."""
        _call("luminary_ext_render_shutter", self._h, C.c_uint32(slices), C.c_uint32(samples_per_slice), C.c_uint32(samples_per_pass))

    def shutter_stats(self):
        """luminary_ext_get_shutter_stats, as a dict."""
        s = ShutterStats()
        _call("luminary_ext_get_shutter_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def render(self, num_samples):
        """The reference's render loop for `num_samples` more sample allocations (adaptive sampling per the renderer settings)."""
        _call("luminary_ext_render", self._h, C.c_uint32(num_samples))

    def accumulators(self):
        import numpy as np
        n = C.c_uint32()
        _call("luminary_ext_get_accumulators", self._h, C.c_void_p(0), C.c_void_p(0), C.byref(n))
        fm = np.zeros(3 * n.value, dtype=np.float32)
        sm = np.zeros(n.value, dtype=np.float32)
        _call("luminary_ext_get_accumulators", self._h, fm.ctypes.data_as(C.c_void_p), sm.ctypes.data_as(C.c_void_p), C.byref(n))
        return fm.reshape(3, -1), sm

    def get_denoiser(self):
        """luminary_ext_get_denoiser"""
        d = DenoiserSettings()
        _call("luminary_ext_get_denoiser", self._h, C.byref(d))
        return d

    def set_denoiser(self, settings=None, **fields):
        """luminary_ext_set_denoiser: the given settings, or the current ones with `fields` changed (set_denoiser(enabled=True)). Does not restart the integration."""
        d = settings if settings is not None else self.get_denoiser()
        for k, v in fields.items():
            setattr(d, k, v)
        _call("luminary_ext_set_denoiser", self._h, C.byref(d))

    def denoised(self, width, height):
        """luminary_ext_get_denoised: the denoised mean radiance [H, W, 3] of the accumulated frame."""
        import numpy as np
        out = np.zeros((height, width, 3), dtype=np.float32)
        _call("luminary_ext_get_denoised", self._h, out.ctypes.data_as(C.c_void_p), C.c_uint32(width), C.c_uint32(height))
        return out

    def get_firefly_rejection(self):
        """luminary_ext_get_firefly_rejection"""
        f = FireflySettings()
        _call("luminary_ext_get_firefly_rejection", self._h, C.byref(f))
        return f

    def set_firefly_rejection(self, settings=None, **fields):
        """luminary_ext_set_firefly_rejection: the given settings, or the current ones with `fields` changed (set_firefly_rejection(enabled=True)). A change restarts
        the integration."""
        f = settings if settings is not None else self.get_firefly_rejection()
        for k, v in fields.items():
            setattr(f, k, v)
        _call("luminary_ext_set_firefly_rejection", self._h, C.byref(f))

    def robust_radiance(self, width, height):
        """luminary_ext_get_robust_radiance: the mean radiance [H, W, 3] of the accumulated frame after the firefly resolve."""
        import numpy as np
        out = np.zeros((height, width, 3), dtype=np.float32)
        _call("luminary_ext_get_robust_radiance", self._h, out.ctypes.data_as(C.c_void_p), C.c_uint32(width), C.c_uint32(height))
        return out

    def firefly_stats(self):
        """luminary_ext_get_firefly_stats, as a dict."""
        s = FireflyStats()
        _call("luminary_ext_get_firefly_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def get_history(self):
        """luminary_ext_get_history"""
        f = HistorySettings()
        _call("luminary_ext_get_history", self._h, C.byref(f))
        return f

    def set_history(self, settings=None, **fields):
        """luminary_ext_set_history: the given settings, or the current ones with `fields` changed (set_history(enabled=True)). Does not restart the integration."""
        f = settings if settings is not None else self.get_history()
        for k, v in fields.items():
            setattr(f, k, v)
        _call("luminary_ext_set_history", self._h, C.byref(f))

    def history_image(self, width, height):
        """luminary_ext_get_history_image: (the image as last shown before bloom [H, W, 3], its weight plane [H, W]) float32."""
        import numpy as np
        rgb, weight = np.zeros((height, width, 3), dtype=np.float32), np.zeros((height, width), dtype=np.float32)
        _call("luminary_ext_get_history_image", self._h, rgb.ctypes.data_as(C.c_void_p), weight.ctypes.data_as(C.c_void_p), C.c_uint32(width), C.c_uint32(height))
        return rgb, weight

    def history_stats(self):
        """luminary_ext_get_history_stats, as a dict."""
        s = HistoryStats()
        _call("luminary_ext_get_history_stats", self._h, C.byref(s))
        return {name: (getattr(s, name).decode() if name == "last_drop" else getattr(s, name)) for name, _ in s._fields_}

    def get_history_motion(self):
        """luminary_ext_get_history_motion"""
        f = HistoryMotionSettings()
        _call("luminary_ext_get_history_motion", self._h, C.byref(f))
        return f

    def set_history_motion(self, settings=None, **fields):
        """luminary_ext_set_history_motion: the given settings, or the current ones with `fields` changed (set_history_motion(enabled=True)). Restarts and drops nothing."""
        f = settings if settings is not None else self.get_history_motion()
        for k, v in fields.items():
            setattr(f, k, v)
        _call("luminary_ext_set_history_motion", self._h, C.byref(f))

    def history_motion_stats(self):
        """luminary_ext_get_history_motion_stats, as a dict."""
        s = HistoryMotionStats()
        _call("luminary_ext_get_history_motion_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def instance_change_carries_history(self, instances):
        """luminary_ext_instance_change_carries_history: would set_instance_transforms(instances) keep the image history as the host stands?"""
        instances = list(instances)
        arr = (Instance * max(len(instances), 1))()
        for k, inst in enumerate(instances):
            arr[k] = inst
        out = C.c_bool()
        _call("luminary_ext_instance_change_carries_history", self._h, arr, C.c_uint32(len(instances)), C.byref(out))
        return out.value

    def history_owner(self, width, height, shown=True, current=True):
        """luminary_ext_get_history_owner: (the shown frame's owner plane [H, W] uint32 or None, the current guides' or None)."""
        import numpy as np
        a, b = (np.zeros((height, width), np.uint32) if shown else None), (np.zeros((height, width), np.uint32) if current else None)
        _call("luminary_ext_get_history_owner", self._h, C.c_void_p(a.ctypes.data if shown else None), C.c_void_p(b.ctypes.data if current else None), C.c_uint32(width), C.c_uint32(height))
        return a, b

    def history_transforms(self, instances):
        """luminary_ext_get_history_transforms: (the transforms the shown frame was shown with [instances, 8] float32, the current ones, how many the shown frame
        holds), 8 words each as the device holds them. Raises (invalid argument) where `instances` is not the count of both."""
        import numpy as np
        a, b = np.zeros((instances, 8), np.float32), np.zeros((instances, 8), np.float32)
        held = C.c_uint32()
        _call("luminary_ext_get_history_transforms", self._h, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_uint32(instances), C.byref(held))
        return a, b, held.value

    def render_mattes(self, samples=4, layers=MATTE_LAYER_INSTANCE | MATTE_LAYER_MATERIAL):
        """luminary_ext_render_mattes: ID mattes of the whole frame from `samples` first-hit passes on the main device; the accumulation is not touched."""
        _call("luminary_ext_render_mattes", self._h, C.c_uint32(samples), C.c_uint32(layers))

    def matte(self, layer, ranks, width, height):
        """luminary_ext_get_matte: (ids [ranks, H, W] uint32, coverage [ranks, H, W] float32) of one layer, rank 0 the id with most samples."""
        import numpy as np
        r = max(min(int(ranks), 8), 1)
        ids, cov = np.zeros((r, height, width), dtype=np.uint32), np.zeros((r, height, width), dtype=np.float32)
        _call("luminary_ext_get_matte", self._h, C.c_uint32(layer), C.c_uint32(ranks), ids.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p), C.c_uint32(width),
              C.c_uint32(height))
        return ids, cov

    def matte_mask(self, layer, ids, width, height):
        """luminary_ext_get_matte_mask: [H, W] float32, the share of every pixel's samples whose id is among `ids` (at most 16)."""
        import numpy as np
        want = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        mask = np.zeros((height, width), dtype=np.float32)
        _call("luminary_ext_get_matte_mask", self._h, C.c_uint32(layer), C.c_void_p(want.ctypes.data if want.size else None), C.c_uint32(want.size),
              mask.ctypes.data_as(C.c_void_p), C.c_uint32(width), C.c_uint32(height))
        return mask

    def matte_stats(self):
        """luminary_ext_get_matte_stats, as a dict."""
        s = MatteStats()
        _call("luminary_ext_get_matte_stats", self._h, C.byref(s))
        return {name: (list(getattr(s, name)) if name == "dropped_pixels" else getattr(s, name)) for name, _ in s._fields_}

    def first_hit_guides(self, width, height):
        """luminary_ext_get_first_hit_guides: (albedo [3, H, W], normal [3, H, W], depth [H, W]) float32, the denoiser's guides of the frame."""
        import numpy as np
        a, n, d = np.zeros((3, height, width), np.float32), np.zeros((3, height, width), np.float32), np.zeros((height, width), np.float32)
        _call("luminary_ext_get_first_hit_guides", self._h, a.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_uint32(width),
              C.c_uint32(height))
        return a, n, d

    def ray_counters(self):
        out = (C.c_uint64 * 8)()
        _call("luminary_ext_get_ray_counters", self._h, out)
        return list(out)

    def request_sky_hdri_build(self):
        """luminary_host_request_sky_hdri_build: the sky panorama of HDRI mode is baked again, from the camera's current position."""
        _call("luminary_host_request_sky_hdri_build", self._h)

    def core_sky_hdri(self):
        """The panorama the GPU core last baked for this host, [dim, dim, 4] float32."""
        import numpy as np
        lib, ctx = _lib(), C.c_void_p(self.core_context())
        dim = C.c_uint32()
        lib.lumc_sky_hdri_download.restype = C.c_int
        if lib.lumc_sky_hdri_download(ctx, C.c_void_p(0), C.byref(dim)):
            raise RuntimeError("no baked sky")
        out = np.zeros((dim.value, dim.value, 4), dtype=np.float32)
        if lib.lumc_sky_hdri_download(ctx, out.ctypes.data_as(C.c_void_p), C.byref(dim)):
            raise RuntimeError("lumc_sky_hdri_download failed")
        return out

    def core_context(self):
        ctx = _lib().luminary_ext_get_core_context(self._h)
        if not ctx:
            raise RuntimeError("no usable HIP device (libluminary_amd has no CPU path)")
        return ctx


def default_material():
    """material.c:5-29"""
    m = Material()
    m.base_substrate = SUBSTRATE_OPAQUE
    m.albedo = RGBAF(0.9, 0.9, 0.9, 0.9)
    m.emission = RGBF(0, 0, 0)
    m.emission_scale = 1.0
    m.roughness = 0.7
    m.roughness_clamp = 0.25
    m.refraction_index = 1.0
    m.normal_map_is_compressed = True
    m.albedo_tex = m.luminance_tex = m.roughness_tex = m.metallic_tex = m.normal_tex = 0xFFFF
    return m
