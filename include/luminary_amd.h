/*
 * luminary_amd.h - the Luminary C host API as exported by libluminary_amd.so.
 *
 * Drop-in boundary: every type and function below has the name, field order, argument meaning and error behaviour of
 * the reference's public headers, so a frontend written against <luminary/luminary.h> (e.g. Mandarin Duck) links against
 * this library unchanged. Source of each declaration (paths under /root/reference/include/luminary/):
 *   vectors / colours          api_utils.h:27-51
 *   result codes               error.h:24-101
 *   settings ... instance PODs structs.h:29-391
 *   path                       path.h:24-31
 *   host functions             host.h:29-129
 *   init / shutdown            luminary.h:44-49
 * A frontend's own includes - <luminary/luminary.h>, <luminary/host.h>, <luminary/structs.h>, ... - are served by the forwarding headers in
 * include/luminary/, which all lead here: compile the frontend with -I<this repo>/include and link it with -lluminary_amd.
 * Scope of this implementation: the triangle / BSDF / NEE path with the thin-lens camera under every sky mode
 * (constant colour, procedural atmosphere with sun, moon and stars, baked panorama), the fog volume (scattering events, light scattered in
 * from sun, sky and - over multi-vertex bridges - emissive triangles), particles, the ocean (ray-marched height field, Jerlov water volume,
 * sun and sky light through the surface with caustics), clouds (three ray-marched layers over generated noise textures, procedural sky
 * mode, baked into the panorama in HDRI mode; their shadow in the aerial perspective), textures, adaptive sampling, the undersampling preview, the display chain with bloom,
 * and the debug shading modes. Rendering runs on the library's own "Device" thread once luminary_host_start_new_render was called,
 * like the reference's. The physical camera (use_physical_camera) traces the camera rays through a lens of spherical interfaces, the
 * reference's double-Gauss prescription unless luminary_ext_set_camera_lens gives another; its spectral rendering
 * (physical.use_spectral_rendering) is out of scope and refused.
 *
 * Additive extension (the reference only returns tone-mapped ARGB8): the luminary_ext_* functions at the
 * end give access to float radiance, ray counters and batch rendering. Existing symbols are untouched.
 */
#ifndef LUMINARY_AMD_H
#define LUMINARY_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LUMINARY_API

/* ---- api_utils.h ---- */
typedef struct LuminaryVec3 { float x, y, z; } LuminaryVec3;
typedef struct LuminaryRGBF { float r, g, b; } LuminaryRGBF;
typedef struct LuminaryRGBAF { float r, g, b, a; } LuminaryRGBAF;
typedef struct LuminaryARGB8 { uint8_t b, g, r, a; } LuminaryARGB8;

/* ---- error.h ---- */
typedef uint64_t LuminaryResult;
#define LUMINARY_SUCCESS (0ull)
#define LUMINARY_ERROR_ARGUMENT_NULL (1ull)
#define LUMINARY_ERROR_NOT_IMPLEMENTED (2ull)
#define LUMINARY_ERROR_INVALID_API_ARGUMENT (3ull)
#define LUMINARY_ERROR_MEMORY_LEAK (4ull)
#define LUMINARY_ERROR_OUT_OF_MEMORY (5ull)
#define LUMINARY_ERROR_C_STD (6ull)
#define LUMINARY_ERROR_API_EXCEPTION (7ull)
#define LUMINARY_ERROR_CUDA (8ull)  /* kept for ABI compatibility: raised for HIP runtime failures */
#define LUMINARY_ERROR_OPTIX (9ull) /* kept for ABI compatibility: raised for acceleration-structure failures */
#define LUMINARY_ERROR_PREVIOUS_ERROR (10ull)
#define LUMINARY_ERROR_DEBUG_ASSERT (11ull)
#define LUMINARY_ERROR_MISSING_DATA (12ull)
#define LUMINARY_ERROR_INVALID_DEVICE (13ull)
#define LUMINARY_ERROR_PROPAGATED (0x8000000000000000ull)
LUMINARY_API const char* luminary_result_to_string(LuminaryResult result);

/* ---- structs.h ---- */
#define LUMINARY_HOST_CREATE_INFO_DEVICE_MASK_ALL_DEVICES (0xFFFFFFFF)
typedef struct LuminaryHostCreateInfo { uint32_t device_mask; } LuminaryHostCreateInfo;

typedef enum LuminaryShadingMode {
  LUMINARY_SHADING_MODE_DEFAULT = 0, LUMINARY_SHADING_MODE_ALBEDO = 1, LUMINARY_SHADING_MODE_DEPTH = 2, LUMINARY_SHADING_MODE_NORMAL = 3,
  LUMINARY_SHADING_MODE_IDENTIFICATION = 4, LUMINARY_SHADING_MODE_LIGHTS = 5, LUMINARY_SHADING_MODE_COUNT
} LuminaryShadingMode;
typedef enum LuminaryAdaptiveSamplingOutputMode {
  LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_BEAUTY = 0, LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_VARIANCE = 1,
  LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_ERROR = 2, LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_SAMPLE_DISTRIBUTION = 3,
  LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_COUNT
} LuminaryAdaptiveSamplingOutputMode;

typedef struct LuminaryRendererSettings {
  uint32_t width, height, max_ray_depth, bridge_max_num_vertices, undersampling, supersampling;
  bool enable_adaptive_sampling;
  uint32_t adaptive_sampling_max_sampling_rate, adaptive_sampling_avg_sampling_rate, adaptive_sampling_update_interval;
  bool adaptive_sampling_exposure_aware;
  LuminaryAdaptiveSamplingOutputMode adaptive_sampling_output_mode;
  LuminaryShadingMode shading_mode;
  float region_x, region_y, region_width, region_height;
} LuminaryRendererSettings;

typedef struct LuminaryDeviceInfo {
  bool is_main_device, is_unavailable, is_enabled;
  char name[256];
  size_t memory_size, allocated_memory_size;
} LuminaryDeviceInfo;

typedef struct LuminaryOutputProperties { bool enabled; uint32_t width, height; } LuminaryOutputProperties;
#define LUMINARY_OUTPUT_HANDLE_INVALID 0xFFFFFFFF
typedef uint32_t LuminaryOutputHandle;
typedef struct LuminaryOutputRequestProperties { uint32_t sample_count, width, height; } LuminaryOutputRequestProperties;
typedef uint32_t LuminaryOutputPromiseHandle;
typedef struct LuminaryPixelQueryResult {
  bool pixel_query_is_valid;
  uint32_t instance_id;
  uint16_t material_id;
  float depth;
  LuminaryVec3 rel_hit_pos;
} LuminaryPixelQueryResult;
typedef struct LuminaryImage {
  uint8_t* buffer;
  uint32_t width, height;
  size_t ld;
  struct { float time; uint32_t sample_count; } meta_data;
} LuminaryImage;

typedef enum LuminaryFilter {
  LUMINARY_FILTER_NONE = 0, LUMINARY_FILTER_GRAY = 1, LUMINARY_FILTER_SEPIA = 2, LUMINARY_FILTER_GAMEBOY = 3, LUMINARY_FILTER_2BITGRAY = 4,
  LUMINARY_FILTER_CRT = 5, LUMINARY_FILTER_BLACKWHITE = 6, LUMINARY_FILTER_COUNT
} LuminaryFilter;
typedef enum LuminaryToneMap {
  LUMINARY_TONEMAP_NONE = 0, LUMINARY_TONEMAP_ACES = 1, LUMINARY_TONEMAP_REINHARD = 2, LUMINARY_TONEMAP_UNCHARTED2 = 3, LUMINARY_TONEMAP_AGX = 4,
  LUMINARY_TONEMAP_AGX_PUNCHY = 5, LUMINARY_TONEMAP_AGX_CUSTOM = 6, LUMINARY_TONEMAP_COUNT
} LuminaryToneMap;
typedef enum LuminaryApertureShape { LUMINARY_APERTURE_ROUND = 0, LUMINARY_APERTURE_BLADED = 1, LUMINARY_APERTURE_COUNT } LuminaryApertureShape;

typedef struct LuminaryCamera {
  LuminaryVec3 pos, rotation;
  LuminaryApertureShape aperture_shape;
  uint32_t aperture_blade_count;
  float exposure;
  LuminaryToneMap tonemap;
  float agx_custom_slope, agx_custom_power, agx_custom_saturation;
  LuminaryFilter filter;
  bool use_local_error_minimization;
  float bloom_blend;
  bool dithering, purkinje;
  float purkinje_kappa1, purkinje_kappa2, wasd_speed, mouse_speed;
  bool smooth_movement;
  float smoothing_factor, russian_roulette_threshold;
  bool use_color_correction;
  LuminaryRGBF color_correction;
  float film_grain, camera_scale, object_distance;
  bool use_physical_camera;
  struct { float fov, aperture_size; } thin_lens;
  struct {
    bool allow_reflections, use_spectral_rendering;
    float focal_length, front_focal_point, back_focal_point, front_principal_point, back_principal_point, aperture_point, aperture_diameter,
      exit_pupil_point, exit_pupil_diameter, image_plane_distance, sensor_width;
  } physical;
} LuminaryCamera;

typedef enum LuminaryJerlovWaterType {
  LUMINARY_JERLOV_WATER_TYPE_I = 0, LUMINARY_JERLOV_WATER_TYPE_IA = 1, LUMINARY_JERLOV_WATER_TYPE_IB = 2, LUMINARY_JERLOV_WATER_TYPE_II = 3,
  LUMINARY_JERLOV_WATER_TYPE_III = 4, LUMINARY_JERLOV_WATER_TYPE_1C = 5, LUMINARY_JERLOV_WATER_TYPE_3C = 6, LUMINARY_JERLOV_WATER_TYPE_5C = 7,
  LUMINARY_JERLOV_WATER_TYPE_7C = 8, LUMINARY_JERLOV_WATER_TYPE_9C = 9, LUMINARY_JERLOV_WATER_TYPE_COUNT
} LuminaryJerlovWaterType;
typedef struct LuminaryOcean {
  bool active;
  float height, amplitude, frequency, refractive_index;
  LuminaryJerlovWaterType water_type;
  bool caustics_active;
  uint32_t caustics_ris_sample_count;
  float caustics_domain_scale;
  bool multiscattering, triangle_light_contribution;
} LuminaryOcean;

typedef enum LuminarySkyMode { LUMINARY_SKY_MODE_DEFAULT = 0, LUMINARY_SKY_MODE_HDRI = 1, LUMINARY_SKY_MODE_CONSTANT_COLOR = 2, LUMINARY_SKY_MODE_COUNT } LuminarySkyMode;
typedef struct LuminarySky {
  LuminaryVec3 geometry_offset;
  float azimuth, altitude, moon_azimuth, moon_altitude, moon_tex_offset, sun_strength, base_density;
  bool ozone_absorption;
  uint32_t steps, stars_count, stars_seed;
  float stars_intensity, rayleigh_density, mie_density, ozone_density, rayleigh_falloff, mie_falloff, mie_diameter, ground_visibility,
    ozone_layer_thickness, multiscattering_factor;
  uint32_t hdri_dim, hdri_samples;
  bool aerial_perspective;
  LuminaryRGBF constant_color;
  LuminarySkyMode mode;
} LuminarySky;

typedef struct LuminaryCloudLayer {
  bool active;
  float height_max, height_min, coverage, coverage_min, type, type_min, wind_speed, wind_angle;
} LuminaryCloudLayer;
typedef struct LuminaryCloud {
  bool active, initialized, atmosphere_scattering;
  LuminaryCloudLayer low, mid, top;
  float offset_x, offset_z, density;
  uint32_t seed;
  float droplet_diameter;
  uint32_t steps, shadow_steps;
  float noise_shape_scale, noise_detail_scale, noise_weather_scale, mipmap_bias;
  uint32_t octaves;
} LuminaryCloud;
typedef struct LuminaryFog { bool active; float density, droplet_diameter, height, dist; } LuminaryFog;
typedef struct LuminaryParticles {
  bool active;
  uint32_t seed, count;
  LuminaryRGBF albedo;
  float speed, direction_altitude, direction_azimuth, phase_diameter, scale, size, size_variation;
} LuminaryParticles;

typedef enum LuminaryMaterialBaseSubstrate {
  LUMINARY_MATERIAL_BASE_SUBSTRATE_OPAQUE, LUMINARY_MATERIAL_BASE_SUBSTRATE_TRANSLUCENT, LUMINARY_MATERIAL_BASE_SUBSTRATE_COUNT
} LuminaryMaterialBaseSubstrate;
typedef struct LuminaryMaterial {
  uint32_t id;
  LuminaryMaterialBaseSubstrate base_substrate;
  LuminaryRGBAF albedo;
  LuminaryRGBF emission;
  float emission_scale, roughness, roughness_clamp, refraction_index;
  bool emission_active, thin_walled, metallic, colored_transparency, roughness_as_smoothness, normal_map_is_compressed, bidirectional_emission;
  uint16_t albedo_tex, luminance_tex, roughness_tex, metallic_tex, normal_tex;
} LuminaryMaterial;
typedef struct LuminaryInstance { uint32_t id, mesh_id; LuminaryVec3 position, rotation, scale; } LuminaryInstance;

/* ---- path.h ---- */
typedef struct LuminaryPath LuminaryPath;
LUMINARY_API LuminaryResult luminary_path_create(LuminaryPath** path);
LUMINARY_API LuminaryResult luminary_path_set_from_string(LuminaryPath* path, const char* string);
LUMINARY_API LuminaryResult luminary_path_destroy(LuminaryPath** path);

/* ---- luminary.h ---- */
LUMINARY_API void luminary_init(void);
LUMINARY_API void luminary_shutdown(void);

/* ---- host.h ---- */
typedef struct LuminaryHost LuminaryHost;
LUMINARY_API LuminaryResult luminary_host_create(LuminaryHost** host, LuminaryHostCreateInfo info);
LUMINARY_API LuminaryResult luminary_host_destroy(LuminaryHost** host);
LUMINARY_API LuminaryResult luminary_host_start_new_render(LuminaryHost* host);
LUMINARY_API LuminaryResult luminary_host_get_device_count(LuminaryHost* host, uint32_t* device_count);
LUMINARY_API LuminaryResult luminary_host_get_device_info(LuminaryHost* host, uint32_t device_id, LuminaryDeviceInfo* info);
LUMINARY_API LuminaryResult luminary_host_set_device_enable(LuminaryHost* host, uint32_t device_id, bool enable);
LUMINARY_API LuminaryResult luminary_host_start_device(LuminaryHost* host, uint32_t index);
LUMINARY_API LuminaryResult luminary_host_shutdown_device(LuminaryHost* host, uint32_t index);
LUMINARY_API LuminaryResult luminary_host_load_lum_file(LuminaryHost* host, LuminaryPath* path);
LUMINARY_API LuminaryResult luminary_host_load_obj_file(LuminaryHost* host, LuminaryPath* path);
LUMINARY_API LuminaryResult luminary_host_get_current_sample_time(LuminaryHost* host, double* time);
LUMINARY_API LuminaryResult luminary_host_get_num_queue_workers(const LuminaryHost* host, uint32_t* num_queue_workers);
LUMINARY_API LuminaryResult luminary_host_get_queue_worker_name(const LuminaryHost* host, uint32_t queue_worker_id, const char** string);
LUMINARY_API LuminaryResult luminary_host_get_queue_worker_string(const LuminaryHost* host, uint32_t queue_worker_id, const char** string);
LUMINARY_API LuminaryResult luminary_host_get_queue_worker_time(const LuminaryHost* host, uint32_t queue_worker_id, double* time);
LUMINARY_API LuminaryResult luminary_host_set_output_properties(LuminaryHost* host, LuminaryOutputProperties properties);
LUMINARY_API LuminaryResult luminary_host_request_output(LuminaryHost* host, LuminaryOutputRequestProperties properties, LuminaryOutputPromiseHandle* handle);
LUMINARY_API LuminaryResult luminary_host_try_await_output(LuminaryHost* host, LuminaryOutputPromiseHandle handle, LuminaryOutputHandle* output_handle);
LUMINARY_API LuminaryResult luminary_host_acquire_output(LuminaryHost* host, LuminaryOutputHandle* output_handle);
LUMINARY_API LuminaryResult luminary_host_get_image(LuminaryHost* host, LuminaryOutputHandle output_handle, LuminaryImage* image);
LUMINARY_API LuminaryResult luminary_host_release_output(LuminaryHost* host, LuminaryOutputHandle output_handle);
LUMINARY_API LuminaryResult luminary_host_get_pixel_info(LuminaryHost* host, uint16_t x, uint16_t y, LuminaryPixelQueryResult* result);
LUMINARY_API LuminaryResult luminary_host_get_settings(LuminaryHost* host, LuminaryRendererSettings* settings);
LUMINARY_API LuminaryResult luminary_host_set_settings(LuminaryHost* host, const LuminaryRendererSettings* settings);
LUMINARY_API LuminaryResult luminary_host_get_camera(LuminaryHost* host, LuminaryCamera* camera);
LUMINARY_API LuminaryResult luminary_host_set_camera(LuminaryHost* host, const LuminaryCamera* camera);
LUMINARY_API LuminaryResult luminary_host_get_ocean(LuminaryHost* host, LuminaryOcean* ocean);
LUMINARY_API LuminaryResult luminary_host_set_ocean(LuminaryHost* host, const LuminaryOcean* ocean);
LUMINARY_API LuminaryResult luminary_host_get_sky(LuminaryHost* host, LuminarySky* sky);
LUMINARY_API LuminaryResult luminary_host_set_sky(LuminaryHost* host, const LuminarySky* sky);
LUMINARY_API LuminaryResult luminary_host_get_cloud(LuminaryHost* host, LuminaryCloud* cloud);
LUMINARY_API LuminaryResult luminary_host_set_cloud(LuminaryHost* host, const LuminaryCloud* cloud);
LUMINARY_API LuminaryResult luminary_host_get_fog(LuminaryHost* host, LuminaryFog* fog);
LUMINARY_API LuminaryResult luminary_host_set_fog(LuminaryHost* host, const LuminaryFog* fog);
LUMINARY_API LuminaryResult luminary_host_get_particles(LuminaryHost* host, LuminaryParticles* particles);
LUMINARY_API LuminaryResult luminary_host_set_particles(LuminaryHost* host, const LuminaryParticles* particles);
LUMINARY_API LuminaryResult luminary_host_get_material(LuminaryHost* host, uint16_t id, LuminaryMaterial* material);
LUMINARY_API LuminaryResult luminary_host_set_material(LuminaryHost* host, uint16_t id, const LuminaryMaterial* material);
LUMINARY_API LuminaryResult luminary_host_get_instance(LuminaryHost* host, uint32_t id, LuminaryInstance* instance);
LUMINARY_API LuminaryResult luminary_host_set_instance(LuminaryHost* host, const LuminaryInstance* instance);
LUMINARY_API LuminaryResult luminary_host_new_instance(LuminaryHost* host, LuminaryInstance* instance);
LUMINARY_API LuminaryResult luminary_host_get_num_meshes(LuminaryHost* host, uint32_t* num_meshes);
LUMINARY_API LuminaryResult luminary_host_get_num_materials(LuminaryHost* host, uint32_t* num_materials);
LUMINARY_API LuminaryResult luminary_host_get_num_instances(LuminaryHost* host, uint32_t* num_instances);
LUMINARY_API LuminaryResult luminary_host_save_png(LuminaryHost* host, LuminaryOutputHandle handle, LuminaryPath* path);
LUMINARY_API LuminaryResult luminary_host_request_sky_hdri_build(LuminaryHost* host);

/* ---- additive extension (not in the reference) ---- */
struct LumDeviceSceneView;
struct LumLightRefitPlan;
/* ---- "extra utils" frontends link against: reference include/luminary/{host_memory,array,queue,ringbuffer,thread_status,log,name_strings}.h ---- */
#define host_malloc(ptr, size) _host_malloc((void**) (ptr), (size), (const char*) #ptr, (const char*) __func__, __LINE__)
#define host_realloc(ptr, size) _host_realloc((void**) (ptr), (size), (const char*) #ptr, (const char*) __func__, __LINE__)
#define host_free(ptr) _host_free((void**) (ptr), (const char*) #ptr, (const char*) __func__, __LINE__)
LUMINARY_API LuminaryResult _host_malloc(void** ptr, size_t size, const char* buf_name, const char* func, uint32_t line);   /* host_memory.h:28 */
LUMINARY_API LuminaryResult _host_realloc(void** ptr, size_t size, const char* buf_name, const char* func, uint32_t line);  /* host_memory.h:29 */
LUMINARY_API LuminaryResult _host_free(void** ptr, const char* buf_name, const char* func, uint32_t line);                  /* host_memory.h:30 */

#define array_create(array, size_of_element, num_elements) \
  _array_create((void**) (array), (size_of_element), (num_elements), (const char*) #array, (const char*) __func__, __LINE__)
#define array_resize(array, size) _array_resize((void**) (array), (size), (const char*) #array, (const char*) __func__, __LINE__)
#define array_push(array, object) _array_push((void**) (array), (void*) (object), (const char*) #array, (const char*) __func__, __LINE__)
#define array_copy(dst, src) _array_copy((void**) (dst), (void**) (src), (const char*) #dst, (const char*) __func__, __LINE__)
#define array_append(dst, src) _array_append((void**) (dst), (const void*) (src), (const char*) #dst, (const char*) __func__, __LINE__)
#define array_set_num_elements(array, num_elements) \
  _array_set_num_elements((void**) (array), (num_elements), (const char*) #array, (const char*) __func__, __LINE__)
#define array_destroy(array) _array_destroy((void**) (array), (const char*) #array, (const char*) __func__, __LINE__)
LUMINARY_API LuminaryResult _array_create(void** array, size_t size_of_element, uint32_t num_elements, const char* buf_name, const char* func, uint32_t line); /* array.h:34 */
LUMINARY_API LuminaryResult _array_resize(void** array, size_t size, const char* buf_name, const char* func, uint32_t line);
LUMINARY_API LuminaryResult _array_push(void** array, void* object, const char* buf_name, const char* func, uint32_t line);
LUMINARY_API LuminaryResult _array_copy(void** dst, const void* src, const char* buf_name, const char* func, uint32_t line);
LUMINARY_API LuminaryResult _array_append(void** dst, const void* src, const char* buf_name, const char* func, uint32_t line);
LUMINARY_API LuminaryResult _array_destroy(void** array, const char* buf_name, const char* func, uint32_t line);
LUMINARY_API LuminaryResult array_clear(void* array);
LUMINARY_API LuminaryResult array_get_size(const void* array, size_t* size);
LUMINARY_API LuminaryResult array_get_num_elements(const void* array, uint32_t* num_elements);
LUMINARY_API LuminaryResult _array_set_num_elements(void** array, uint32_t num_elements, const char* buf_name, const char* func, uint32_t line);

typedef struct LuminaryQueue LuminaryQueue;          /* queue.h:25-40 */
typedef bool (*LuminaryEqOp)(void* lhs, void* rhs);
#define queue_create(queue, size_of_element, num_elements) \
  _queue_create((queue), (size_of_element), (num_elements), (const char*) #queue, (const char*) __func__, __LINE__)
#define queue_destroy(queue) _queue_destroy((queue), (const char*) #queue, (const char*) __func__, __LINE__)
LUMINARY_API LuminaryResult _queue_create(LuminaryQueue** queue, size_t size_of_element, size_t num_elements, const char* buf_name, const char* func, uint32_t line);
LUMINARY_API LuminaryResult queue_push(LuminaryQueue* queue, void* object);
LUMINARY_API LuminaryResult queue_push_unique(LuminaryQueue* queue, void* object, LuminaryEqOp equal_operator, bool* already_queued);
LUMINARY_API LuminaryResult queue_pop(LuminaryQueue* queue, void* object, bool* success);
LUMINARY_API LuminaryResult queue_pop_blocking(LuminaryQueue* queue, void* object, bool* success);
LUMINARY_API LuminaryResult queue_set_is_blocking(LuminaryQueue* queue, bool is_blocking);
LUMINARY_API LuminaryResult _queue_destroy(LuminaryQueue** queue, const char* buf_name, const char* func, uint32_t line);

typedef struct LuminaryRingBuffer LuminaryRingBuffer;  /* ringbuffer.h:25-34 */
#define ringbuffer_create(buffer, size) _ringbuffer_create((buffer), (size), (const char*) #buffer, (const char*) __func__, __LINE__)
#define ringbuffer_destroy(buffer) _ringbuffer_destroy((buffer), (const char*) #buffer, (const char*) __func__, __LINE__)
LUMINARY_API LuminaryResult _ringbuffer_create(LuminaryRingBuffer** buffer, size_t size, const char* buf_name, const char* func, uint32_t line);
LUMINARY_API LuminaryResult ringbuffer_allocate_entry(LuminaryRingBuffer* buffer, size_t entry_size, void** entry);
LUMINARY_API LuminaryResult ringbuffer_release_entry(LuminaryRingBuffer* buffer, size_t entry_size);
LUMINARY_API LuminaryResult _ringbuffer_destroy(LuminaryRingBuffer** buffer, const char* buf_name, const char* func, uint32_t line);

typedef struct LuminaryThreadStatus LuminaryThreadStatus;  /* thread_status.h:25-34 */
LUMINARY_API LuminaryResult thread_status_create(LuminaryThreadStatus** thread_status);
LUMINARY_API LuminaryResult thread_status_set_worker_name(LuminaryThreadStatus* thread_status, const char* name);
LUMINARY_API LuminaryResult thread_status_get_worker_name(LuminaryThreadStatus* thread_status, const char** name);
LUMINARY_API LuminaryResult thread_status_start(LuminaryThreadStatus* thread_status, const char* string);
LUMINARY_API LuminaryResult thread_status_get_time(LuminaryThreadStatus* thread_status, double* time);
LUMINARY_API LuminaryResult thread_status_get_string(LuminaryThreadStatus* thread_status, const char** string);
LUMINARY_API LuminaryResult thread_status_stop(LuminaryThreadStatus* thread_status);
LUMINARY_API LuminaryResult thread_status_destroy(LuminaryThreadStatus** thread_status);

#define log_message(fmt, ...) luminary_print_log("[%s:%d] " fmt, __func__, __LINE__, ##__VA_ARGS__)   /* log.h:23-31 */
#define warn_message(fmt, ...) luminary_print_warn("[%s:%d] " fmt, __func__, __LINE__, ##__VA_ARGS__)
#define error_message(fmt, ...) luminary_print_error("[%s:%d] " fmt, __func__, __LINE__, ##__VA_ARGS__)
#define crash_message(fmt, ...) luminary_print_crash("[%s:%d] " fmt, __func__, __LINE__, ##__VA_ARGS__)
LUMINARY_API void luminary_print_log(const char* format, ...);
LUMINARY_API void luminary_print_info(bool log, const char* format, ...);
LUMINARY_API void luminary_print_info_inline(bool log, const char* format, ...);
LUMINARY_API void luminary_print_warn(const char* format, ...);
LUMINARY_API void luminary_print_error(const char* format, ...);
LUMINARY_API void luminary_print_crash(const char* format, ...);
LUMINARY_API void luminary_write_log(void);

extern const char* const luminary_strings_shading_mode[LUMINARY_SHADING_MODE_COUNT];   /* name_strings.h:22-29 */
extern const char* const luminary_strings_adaptive_sampling_output_mode[LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_COUNT];
extern const char* const luminary_strings_filter[LUMINARY_FILTER_COUNT];
extern const char* const luminary_strings_tonemap[LUMINARY_TONEMAP_COUNT];
extern const char* const luminary_strings_aperture[LUMINARY_APERTURE_COUNT];
extern const char* const luminary_strings_jerlov_water_type[LUMINARY_JERLOV_WATER_TYPE_COUNT];
extern const char* const luminary_strings_sky_mode[LUMINARY_SKY_MODE_COUNT];
extern const char* const luminary_strings_material_base_substrate[LUMINARY_MATERIAL_BASE_SUBSTRATE_COUNT];

/* Adds an RGBA8 texture (byte order r, g, b, a; rows top to bottom as in a PNG) and returns the id materials refer to through
 * albedo_tex / roughness_tex / normal_tex (luminance and metallic textures are not evaluated, the latter like in the reference). `gamma` is
 * applied to r, g, b on fetch (1 = none; PNG files carry 100000 / gAMA). */
LUMINARY_API LuminaryResult luminary_ext_add_texture(LuminaryHost* host, const uint8_t* rgba8, uint32_t width, uint32_t height, float gamma, uint16_t* texture_id);

/* Embedded data files by name, as the reference's Ceb-generated accessor (device/device_embedded.c:1075-1093): "bluenoise_1D.bin",
 * "bluenoise_2D.bin"; *info = 0 on success, non-zero for an unknown name (frontend assets such as fonts are not part of this library). */
LUMINARY_API void ceb_access(const char* name, void** ptr, int64_t* lmem, uint64_t* info);

/* additive: RGBA8 PNG of an ARGB8 image (words b | g << 8 | r << 16 | a << 24; `ld` = words per row), as luminary_host_save_png writes */
LUMINARY_API LuminaryResult luminary_ext_write_png(const char* path, const uint32_t* argb8, uint32_t width, uint32_t height, size_t ld);
/* additive: bytes currently held through _host_malloc, and the text luminary_write_log would write */
LUMINARY_API LuminaryResult luminary_ext_host_memory_in_use(uint64_t* bytes);
LUMINARY_API LuminaryResult luminary_ext_get_log(const char** text, size_t* length);

/* Adds a mesh from flat per-triangle arrays (reference Mesh layout, mesh.h:8-14): 9 position floats, 9 normal floats, 6 uv floats and one
 * material id per triangle. Materials are added with luminary_ext_add_material. Returns the new ids. */
LUMINARY_API LuminaryResult luminary_ext_add_mesh(
  LuminaryHost* host, const float* positions, const float* normals, const float* uvs, const uint16_t* material_ids, uint32_t triangle_count, uint32_t* mesh_id);
LUMINARY_API LuminaryResult luminary_ext_add_material(LuminaryHost* host, const LuminaryMaterial* material, uint16_t* material_id);
/* The host-level mesh back (borrowed pointers into the host's store, valid until the mesh list changes): what an independent encoder starts from. */
LUMINARY_API LuminaryResult luminary_ext_get_mesh(LuminaryHost* host, uint32_t mesh_id, const float** positions, const float** normals, const float** uvs,
                                                  const uint16_t** material_ids, uint32_t* triangle_count);
/* Deformable meshes. New positions (9 floats per triangle) and normals (9 per triangle, or NULL = face normals by the loader's rule for a file without normals)
 * for a mesh the host already holds. triangle_count must equal the mesh's; order, uvs and material ids stay. The host mesh is overwritten in place (the
 * luminary_ext_get_mesh pointers stay valid). Restarts the integration. LUMINARY_ERROR_INVALID_API_ARGUMENT, and nothing changes: a mesh id the host does not have,
 * another triangle count, NULL positions, a position that is not finite. On the devices only the vertices are uploaded and the mesh's tree is refitted there
 * (luminary_ext_set_mesh_refit_in_place: in the scene's node array itself, which then keeps its layout). */
LUMINARY_API LuminaryResult luminary_ext_set_mesh_positions(LuminaryHost* host, uint32_t mesh_id, const float* positions, const float* normals, uint32_t triangle_count);
/* mode 0 (default): refit the mesh's tree; 1: build it again. max_cost_growth > 0: in mode 0, build again when the tree's cost (the sum over all nodes and occupied
 * child slots of the child box's half surface area) has grown beyond this factor of its cost when it was last BUILT; 0 = never. No default threshold is built in:
 * the stats report the growth. Images do not depend on any of it. */
LUMINARY_API LuminaryResult luminary_ext_set_mesh_refit(LuminaryHost* host, uint32_t mode, float max_cost_growth);
typedef struct LuminaryMeshRefitStats {
  uint64_t refits, rebuilds;           /* meshes refitted / built again by the main device's context since it was created (uploads do not reset them) */
  uint32_t last_refits, last_rebuilds; /* ... by the last update */
  double max_cost_growth;              /* largest cost growth among the meshes the last update refitted (0: none) */
  double seconds;                      /* the last update's mesh part on the main device */
  double seconds_upload, seconds_refit, seconds_rebuild, seconds_assemble;
  double seconds_hash, seconds_download, seconds_lights; /* as LumMeshRefitStats (include/lum_core.h) */
} LuminaryMeshRefitStats;
LUMINARY_API LuminaryResult luminary_ext_get_mesh_refit_stats(LuminaryHost* host, LuminaryMeshRefitStats* out);
/* Rigidly moving instances, in bulk. For each of the `count` entries: `id` names an existing, active instance (one that points at a mesh the host holds), `mesh_id`
 * must equal its current mesh (changing the mesh stays luminary_host_set_instance's job), position, rotation and scale must be finite. Restarts the integration.
 * LUMINARY_ERROR_INVALID_API_ARGUMENT, and nothing changes - not for the entries before the offending one either: NULL instances with a count, an unknown id, an
 * inactive instance, another mesh_id, a value that is not finite. On the devices only the 32-byte transforms are uploaded: rows, world boxes, the top-level tree
 * and its leaf records are derived from them there, the mesh trees stay where they are (luminary_ext_set_instance_update). */
LUMINARY_API LuminaryResult luminary_ext_set_instance_transforms(LuminaryHost* host, const LuminaryInstance* instances, uint32_t count);
/* mode 0 (default): moved instances are taken over on the device; 1: as luminary_host_set_instance's edits are - the scene tree is assembled on the host and
 * uploaded (for comparison; also what a single update falls back to when the device path cannot take it). Images do not depend on it. */
LUMINARY_API LuminaryResult luminary_ext_set_instance_update(LuminaryHost* host, uint32_t mode);
typedef struct LuminaryInstanceUpdateStats {
  uint64_t device_updates, fallbacks, relayouts; /* moved-instance updates of the main device's context that ran on the device / fell back to the host's path / laid
                                                    the node array out anew, since it was created */
  uint32_t tlas_nodes, tlas_depth, tlas_capacity, hittable; /* the last device update's top level: nodes, 4-wide levels, the node slots reserved for it, instances that can be hit */
  double seconds;                                /* the last update's instance part on the main device */
  double seconds_relayout, seconds_upload, seconds_boxes, seconds_build, seconds_leaves; /* as LumInstanceUpdateStats (include/lum_core.h) */
} LuminaryInstanceUpdateStats;
LUMINARY_API LuminaryResult luminary_ext_get_instance_update_stats(LuminaryHost* host, LuminaryInstanceUpdateStats* out);
/* Deformable meshes under moving instances. on = 0 (default): moved vertices are refitted in a copy of the mesh's tree and the host assembles and uploads the scene's
 * node array again. on = 1: with luminary_ext_set_mesh_refit in mode 0 and luminary_ext_set_instance_update in mode 0, moved vertices - alone or in the same frame as
 * moved instances - are refitted where the nodes live on the device: only the vertices (and the 32-byte transforms) go up, a few dozen bytes come back, the node
 * array keeps its layout and only the top level is rebuilt. An update the device path cannot take (a mesh built with spatial splits, fewer than two instances that
 * can be hit, a failed allocation, a cost growth beyond max_cost_growth) takes the other path, counted as a fallback. LUMINARY_ERROR_INVALID_API_ARGUMENT for another
 * value. Images do not depend on it. */
LUMINARY_API LuminaryResult luminary_ext_set_mesh_refit_in_place(LuminaryHost* host, uint32_t on);
typedef struct LuminaryResidentRefitStats {
  uint64_t updates, fallbacks;          /* moved-vertices updates of the main device's context that ran in place / fell back, since it was created */
  uint32_t last_meshes, last_launches;  /* the last in-place update: meshes refitted, kernels launched for them */
  uint64_t last_bytes_downloaded;       /* ... bytes that came back for the meshes and the instances' bounds */
  double seconds;                       /* ... from the vertex upload to the finished top level on the main device */
  double seconds_upload, seconds_hash, seconds_refit, seconds_cost, seconds_top_level; /* as LumResidentRefitStats (include/lum_core.h) */
} LuminaryResidentRefitStats;
LUMINARY_API LuminaryResult luminary_ext_get_resident_refit_stats(LuminaryHost* host, LuminaryResidentRefitStats* out);
/* Skinned meshes: the host takes bones, the devices pose the vertices (include/lum_core.h lumc_mesh_skin_bind).
 *   luminary_ext_bind_mesh_skin    binds a mesh the host holds to four bone ids and four weights per corner (12 of each per triangle, corner-major; a slot of weight 0
 *                                  is skipped) over bone_count (1 ... 1024) bones. The rest pose is the host mesh as it is now, copied. While a mesh is bound,
 *                                  luminary_ext_set_mesh_positions on it is refused. Binding again replaces (the rest pose is then the current pose).
 *   luminary_ext_set_mesh_pose     12 floats per bone, row-major 3 x 4, all finite; bone_count the binding's. Restarts the integration. The devices get 48 bytes per
 *                                  bone and write the mesh's vertices themselves: linear blend skinning in binary32, normals through the bones' 3 x 3 part as it is
 *                                  (right for rotations and uniform scale only), normalised. A mesh with an emissive triangle is also posed on the host at once and
 *                                  the light tree rebuilt; for any other mesh the host mesh is brought up to date - by the same function on the CPU, the same
 *                                  bytes - only when something reads it: luminary_ext_get_mesh, luminary_ext_build_device_scene, a change of the mesh list,
 *                                  a light tree build, the unbind. A pose whose result is not finite fails the next render (LUMINARY_ERROR_CUDA).
 *   luminary_ext_unbind_mesh_skin  the host mesh becomes the current pose, and plain again.
 * LUMINARY_ERROR_INVALID_API_ARGUMENT, and nothing changes: a mesh id the host does not have, another triangle count, NULL arrays, a weight that is negative or not
 * finite, an id >= bone_count, bone_count 0 or above 1024, a pose or an unbind for a mesh that is not bound, another bone_count, a matrix entry that is not finite. */
LUMINARY_API LuminaryResult luminary_ext_bind_mesh_skin(LuminaryHost* host, uint32_t mesh_id, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count,
                                                        uint32_t bone_count);
LUMINARY_API LuminaryResult luminary_ext_unbind_mesh_skin(LuminaryHost* host, uint32_t mesh_id);
LUMINARY_API LuminaryResult luminary_ext_set_mesh_pose(LuminaryHost* host, uint32_t mesh_id, const float* bones, uint32_t bone_count);
typedef struct LuminaryMeshSkinStats {
  uint64_t poses, rebuild_downloads;    /* poses the main device's context applied / posed meshes it downloaded for a rebuild, since it was created */
  uint32_t last_meshes, last_launches;  /* its last update that skinned: meshes with a new pose, skinning kernels launched */
  uint64_t last_bytes_uploaded;         /* ... bytes that went up for them */
  double seconds, seconds_upload, seconds_skin; /* as LumMeshSkinStats (include/lum_core.h) */
  uint64_t host_materialisations;       /* times the host posed a mesh on the CPU because something read it, since the host was created */
} LuminaryMeshSkinStats;
LUMINARY_API LuminaryResult luminary_ext_get_mesh_skin_stats(LuminaryHost* host, LuminaryMeshSkinStats* out);
/* Morph targets / blend shapes: the host takes 4 bytes per target, the devices blend the vertices (include/lum_core.h lumc_mesh_morph_bind).
 *   luminary_ext_bind_mesh_morph    binds a mesh the host holds to target_count (1 ... 1024) sparse targets, target-major: offsets[target_count + 1] into
 *                                   corners[E] (a corner is 3 * triangle + 0 ... 2; strictly increasing within a target), delta_positions[3E] and delta_normals[3E]
 *                                   (NULL: zero). All weights start at 0. While a mesh is bound, luminary_ext_set_mesh_positions on it is refused.
 *   luminary_ext_set_mesh_weights   target_count (the binding's) finite floats; negative weights and weights above 1 are ordinary. Restarts the integration. Per corner
 *                                   the entries are added in ascending target order in binary32 (weight * delta, then the add; a weight of 0 skips the entry), and
 *                                   the normal of a corner something was added to is normalised. A mesh with an emissive triangle is also blended on the host at
 *                                   once and the light tree rebuilt; for any other mesh the host mesh is brought up to date - by the same function on the CPU,
 *                                   the same bytes, counted in host_materialisations - only when something reads it, as for a pose. Weights whose result is not
 *                                   finite fail the next render (LUMINARY_ERROR_CUDA).
 *   luminary_ext_unbind_mesh_morph  drops the targets.
 * A mesh has ONE rest shape, whether it is skinned, morphed or both: the first binding of either kind copies the host mesh as it is now; binding the other kind
 * while one is bound shares that copy; binding a kind again while the other is bound keeps it (for a mesh that holds one kind alone, binding that kind again makes
 * the current shape the rest, as before). A mesh that holds both is morphed first and the skin poses the result - its un-normalised position and normal - in one
 * kernel; until its first pose the morph alone shapes it. Unbinding one of two leaves what the other makes of the rest shape; unbinding the last makes the host mesh
 * the current shape, and plain again.
 * LUMINARY_ERROR_INVALID_API_ARGUMENT, and nothing changes: a mesh id the host does not have, another triangle count, NULL arrays, target_count 0 or above 1024,
 * offsets that do not start at 0 or decrease, a corner >= 3 * triangle_count, corners of a target that are not strictly increasing, a delta or a weight that is not
 * finite, weights or an unbind for a mesh without a morph, another target_count. */
LUMINARY_API LuminaryResult luminary_ext_bind_mesh_morph(LuminaryHost* host, uint32_t mesh_id, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets,
                                                         const uint32_t* corners, const float* delta_positions, const float* delta_normals);
LUMINARY_API LuminaryResult luminary_ext_unbind_mesh_morph(LuminaryHost* host, uint32_t mesh_id);
LUMINARY_API LuminaryResult luminary_ext_set_mesh_weights(LuminaryHost* host, uint32_t mesh_id, const float* weights, uint32_t target_count);
typedef struct LuminaryMeshMorphStats {
  uint64_t applied, rebuild_downloads;  /* weight sets the main device's context applied / morphed meshes it downloaded for a rebuild, since it was created */
  uint32_t last_meshes, last_launches;  /* its last update that morphed: meshes with new weights, morph kernels launched */
  uint64_t last_bytes_uploaded;         /* ... bytes that went up for them */
  double seconds, seconds_upload, seconds_morph; /* as LumMeshMorphStats (include/lum_core.h) */
  uint64_t host_materialisations;       /* the counter of LuminaryMeshSkinStats: times the host posed or blended a mesh on the CPU because something read it */
} LuminaryMeshMorphStats;
LUMINARY_API LuminaryResult luminary_ext_get_mesh_morph_stats(LuminaryHost* host, LuminaryMeshMorphStats* out);
/* Shutter: motion blur from two keys of the scene (csrc/host/mesh_shutter.h). The shutter interval is cut into slices; the scene is brought
 * to each slice's time on the devices and a share of the sample ids is rendered into the same accumulators.
 *   luminary_ext_shutter_open    the scene as it stands is the open key: every enabled device is brought up to date, as a render does before its first pass, the
 *                                camera's pos and rotation and every instance's position, rotation and scale are remembered, and from now on the host records
 *                                which meshes move. (Without a usable device the call still succeeds; luminary_ext_render_shutter then reports the device.)
 *   edits that define the close key, each behaving exactly as without a shutter: luminary_ext_set_mesh_positions, luminary_ext_set_mesh_pose,
 *                                luminary_ext_set_mesh_weights, luminary_ext_set_instance_transforms, a camera change of pos or rotation. A moved emitter needs
 *                                luminary_ext_set_light_refit(host, 1, ...) before the shutter opens.
 *   luminary_ext_render_shutter  slices 1 ... 1024, samples_per_slice >= 1. The moved meshes' open keys are taken on the devices, the ordinary update brings the
 *                                devices to the close key, the close keys are taken; then for slice k of S, t_k = (float) (2k + 1) / (float) (2S): the meshes
 *                                are written at t_k by a HIP kernel (a + t * (b - a) per coordinate in binary32), the camera's pos and rotation and the moved
 *                                instances' position, rotation and scale are set to a + t_k * (b - a) per component in binary32 - Euler angles, blended as they
 *                                are - and encoded into the device scene as the host's own encoders do, one lumc_scene_update applies them, and sample ids
 *                                [first + k n, first + (k + 1) n) are rendered without clearing, first the samples accumulated so far. Then time 1 and the
 *                                close key are applied once more: host and devices agree on the close key, bit for bit what an ordinary update leaves.
 *                                accumulated samples += S n; the outputs are produced as luminary_ext_render_samples produces them. Calling it again without an
 *                                edit in between keeps the keys and accumulates further; any edit afterwards drops the keys and restarts the integration.
 *   luminary_ext_shutter_cancel  forgets the open key (and the devices' keys); nothing else changes.
 * LUMINARY_ERROR_INVALID_API_ARGUMENT, with the reason in the log: luminary_ext_render_shutter without an open key, slices outside 1 ... 1024,
 * samples_per_slice == 0, settings.enable_adaptive_sampling - the host stays as it was -; any pending change other than the edits above (materials, textures, the
 * mesh or instance list, settings, sky, ocean, cloud, fog, particles, another camera field, the lens, the enabled devices, a pending rebuild of the light tree) -
 * the shutter is cancelled and nothing is rendered. Any other render call between open and luminary_ext_render_shutter cancels the shutter. A slice whose light
 * refit asks for a rebuild fails the call with LUMINARY_ERROR_API_EXCEPTION; the next render rebuilds the tree at the close key and the accumulation restarts.
 * Limits: the undersampling preview does not run inside a shutter render, and the denoiser's guides are those of the close key. */
typedef struct LuminaryShutterStats {
  uint64_t renders, slices;             /* shutter renders / slices rendered since the host was created */
  uint32_t last_moved_meshes, last_moved_instances, last_camera_moved, last_slices; /* of the last shutter render */
  double seconds_update, seconds_render; /* ... host wall clock spent in scene updates (keys included) / in rendering the slices */
} LuminaryShutterStats;
LUMINARY_API LuminaryResult luminary_ext_shutter_open(LuminaryHost* host);
LUMINARY_API LuminaryResult luminary_ext_shutter_cancel(LuminaryHost* host);
LUMINARY_API LuminaryResult luminary_ext_render_shutter(LuminaryHost* host, uint32_t slices, uint32_t samples_per_slice, uint32_t samples_per_pass);
LUMINARY_API LuminaryResult luminary_ext_get_shutter_stats(LuminaryHost* host, LuminaryShutterStats* out);
/* Converts the current scene to the device format (device_structs.c conversions + light tree build). The view and everything it points
 * to stay valid until the next call or host destruction. Needs no GPU. */
/* Whether replacing `old` by `input` restarts the integration (camera.c:80-147, settings.c:45-72) or only changes the outputs.
 * entity 0: LuminaryRendererSettings, 1: LuminaryCamera, 2: LuminaryCameraLens (any change restarts; luminary_ext_set_camera_lens applies it
 * while the camera is physical). luminary_host_set_camera / set_settings apply this rule. */
LUMINARY_API LuminaryResult luminary_ext_change_restarts_integration(int entity, const void* input, const void* old, bool* restarts);
/* The physical camera's lens (the camera "given through the API" that device_physical_camera.c:17-54 leaves as a TODO): interface i is a sphere
 * of `radius` (signed: centre at vertex - radius) whose vertex lies at `vertex` on the optical axis, cut off at `cylindrical_radius`; medium i
 * lies in front of interface i (num_interfaces + 1 media; cylindrical_radius FLT_MAX in air). Lengths in mm, the sensor side first. `abbe` is
 * kept for spectral rendering, which is out of scope. Default: the reference's 12-interface double-Gauss lens scaled to 50.53 mm focal length.
 * Rejected (LUMINARY_ERROR_INVALID_API_ARGUMENT): 0 or more than LUMINARY_CAMERA_LENS_MAX_INTERFACES interfaces, non-finite values, an index of
 * refraction <= 0. A new lens restarts the integration while use_physical_camera is set. */
#define LUMINARY_CAMERA_LENS_MAX_INTERFACES 24
typedef struct LuminaryCameraLensInterface { float radius, vertex, cylindrical_radius; } LuminaryCameraLensInterface;
typedef struct LuminaryCameraLensMedium { float design_ior, abbe, cylindrical_radius; } LuminaryCameraLensMedium;
typedef struct LuminaryCameraLens {
  uint32_t num_interfaces;
  LuminaryCameraLensInterface interfaces[LUMINARY_CAMERA_LENS_MAX_INTERFACES];
  LuminaryCameraLensMedium media[LUMINARY_CAMERA_LENS_MAX_INTERFACES + 1];
} LuminaryCameraLens;
LUMINARY_API LuminaryResult luminary_ext_set_camera_lens(LuminaryHost* host, const LuminaryCameraLens* lens);
LUMINARY_API LuminaryResult luminary_ext_get_camera_lens(LuminaryHost* host, LuminaryCameraLens* lens);
/* The path of a file named inside `base_file` (mesh files of a .lum, material libraries of an .obj, maps of an .mtl): path_extend +
 * path_apply of src/luminary/path.c */
LUMINARY_API LuminaryResult luminary_ext_path_extend(const char* base_file, const char* name, char* out, size_t out_size);
/* rotation_euler_angles_to_quaternion (src/luminary/host_math.c:6-21), x y z w */
LUMINARY_API LuminaryResult luminary_ext_euler_to_quaternion(const float rotation[3], float quaternion[4]);
LUMINARY_API LuminaryResult luminary_ext_build_device_scene(LuminaryHost* host, const struct LumDeviceSceneView** view);
/* Refit of the light tree on the devices (include/lum_core.h lumc_light_refit_bind). Off (the default): every edit that moves an emissive
 * triangle - luminary_ext_set_mesh_positions, luminary_ext_set_instance_transforms, luminary_ext_set_mesh_pose, luminary_ext_set_mesh_weights - builds the light
 * tree again on the host, and a posed or blended mesh that emits is brought up to date on the CPU at once. On: the tree of the last host build keeps its topology
 * and every device computes its statistics, the light BVH and the light table again from the vertices it holds; a posed or blended emitter stays lazy on the host.
 * Where a device cannot refit - a triangle collapsed or stopped being finite, or the root's cost grew beyond max_cost_growth (0: never rebuild for quality) - the
 * host builds the tree again, as with the switch off. The setting is remembered across uploads. The view of luminary_ext_build_device_scene holds the light
 * arrays as the devices hold them. */
LUMINARY_API LuminaryResult luminary_ext_set_light_refit(LuminaryHost* host, uint32_t on, float max_cost_growth);
typedef struct LuminaryLightRefitStats {
  uint64_t refits, fallbacks;           /* updates of the main device's context that refitted the lights / that asked for a rebuild, since it was created */
  uint32_t last_launches, last_flags;   /* its last such update: kernels launched; why it fell back (LUMC_LIGHT_REFIT_*) */
  uint64_t last_bytes_uploaded, last_bytes_downloaded;
  double seconds, seconds_fragments, seconds_stats, seconds_nodes, seconds_light_bvh, seconds_table, cost_growth; /* as LumLightRefitStats (include/lum_core.h) */
  uint64_t host_rebuilds;               /* times the host built the light tree again because a device asked for it, since the host was created */
} LuminaryLightRefitStats;
LUMINARY_API LuminaryResult luminary_ext_get_light_refit_stats(LuminaryHost* host, LuminaryLightRefitStats* out);
/* What the last build of the light tree left behind for its refit on a device (lum_core.h LumLightRefitPlan, lumc_light_refit_bind, lumc_light_refit_host): it
 * belongs to the light arrays of the view luminary_ext_build_device_scene returns. The pointers stay valid until the host builds the light tree again. */
LUMINARY_API LuminaryResult luminary_ext_get_light_refit_plan(LuminaryHost* host, struct LumLightRefitPlan* plan);
/* Synchronous batch rendering of sample ids [first_sample, first_sample + num_samples) of `pixels` (NULL = all) on this process' GPU. */
LUMINARY_API LuminaryResult luminary_ext_render_samples(
  LuminaryHost* host, const uint32_t* pixels, uint32_t num_pixels, uint32_t first_sample, uint32_t num_samples, uint32_t samples_per_pass);
/* The reference's render loop, synchronous: `num_samples` more sample allocations of the whole frame. With
 * settings.enable_adaptive_sampling an allocation is one execution of the adaptive sampler's current stage (rates per 4x4 block, stages
 * built after adaptive_sampling_update_interval << stage allocations); otherwise one sample id per pixel. Outputs (recurring and
 * requested) are produced through the result image: local error minimisation and adaptive_sampling_output_mode apply. */
LUMINARY_API LuminaryResult luminary_ext_render(LuminaryHost* host, uint32_t num_samples);
/* Asynchronous rendering is started by luminary_host_start_new_render, as in the reference (host.c:406-414): the host's "Device" worker
 * then renders until the host is destroyed, restarting the accumulation whenever an edit dirties the integration, and the frontend polls
 * luminary_host_try_await_output / luminary_host_acquire_output. Additive controls: stop that worker (returns once the running iteration
 * has ended; the accumulated frame stays and the luminary_ext_render* calls can drive the loop synchronously), and query it. */
LUMINARY_API LuminaryResult luminary_ext_stop_render(LuminaryHost* host);
LUMINARY_API LuminaryResult luminary_ext_is_rendering(LuminaryHost* host, bool* rendering, uint32_t* accumulated_samples);
/* Planar float accumulators of the pixels given to luminary_ext_render_samples: first moment [R|G|B] and luminance second moment. */
LUMINARY_API LuminaryResult luminary_ext_get_accumulators(LuminaryHost* host, float* first_moment, float* second_moment, uint32_t* num_pixels);
/* Radiance = first moment / sample_count for the full frame (rgb interleaved, width*height*3 floats). */
LUMINARY_API LuminaryResult luminary_ext_get_radiance(LuminaryHost* host, float* rgb, uint32_t* sample_count, uint32_t width, uint32_t height);
/* Denoiser (include/lum_core.h lumc_denoise): a variance-guided edge-avoiding a-trous filter on albedo-demodulated radiance, guided by first-hit albedo, normal and
 * depth. When enabled it runs between the result image and bloom, on beauty images of the whole frame in the default shading mode (where bloom runs); not on the
 * undersampling preview, the debug shading modes or the adaptive-sampling diagnostic images. The guides are rendered once per accumulation (guide_samples sample
 * ids, one closest-hit pass each, on the device that holds the frame). Off by default; setting it does not restart the integration.
 * The reference's `GENERAL DENOISER` key of .lum v4 files stays unread, as in the reference. */
typedef struct LuminaryDenoiserSettings {
  bool enabled;           /* false */
  uint32_t guide_samples; /* 4: 1 ... 1024 */
  uint32_t iterations;    /* 5: a-trous iterations, at most 6 */
  float sigma_luminance;  /* 4 */
  float sigma_normal;     /* 128 */
  float sigma_depth;      /* 1 */
} LuminaryDenoiserSettings;
LUMINARY_API LuminaryResult luminary_ext_set_denoiser(LuminaryHost* host, const LuminaryDenoiserSettings* settings);
LUMINARY_API LuminaryResult luminary_ext_get_denoiser(LuminaryHost* host, LuminaryDenoiserSettings* settings);
/* The denoised mean radiance of the full frame (rgb interleaved, width*height*3 floats), whether or not the denoiser is enabled for the outputs;
 * luminary_ext_get_radiance keeps returning the undenoised mean. */
LUMINARY_API LuminaryResult luminary_ext_get_denoised(LuminaryHost* host, float* rgb, uint32_t width, uint32_t height);
/* Firefly rejection (include/lum_core.h lumc_set_firefly_buckets / lumc_firefly_resolve; csrc/host/firefly.h): every sample id is also added to
 * one of `buckets` per-pixel sums (id mod buckets; 12 bytes per pixel and bucket on the device), and the result image takes, for a pixel whose bucket means disagree,
 * the mean of the buckets that are left after the Gini coefficient of their luminances has trimmed the darkest and the brightest; a bucket with a NaN or Inf is
 * left out. When enabled the resolve runs before the denoiser, on beauty images of the whole frame in the default shading mode (where the denoiser and bloom
 * run); never on the undersampling preview. An accumulation driven by adaptive sampling is not resolved (frames_skipped counts those images). Off by default.
 * A change of `enabled` or of `buckets` restarts the integration - unlike the denoiser: the buckets must see every id. The call is refused with
 * LUMINARY_ERROR_INVALID_API_ARGUMENT, with the reason in the log, for buckets outside 4 ... 16 and when the host renders on more than one device slot.
 * luminary_ext_get_radiance and luminary_ext_get_accumulators keep returning the plain sums; luminary_ext_get_denoised follows the outputs: with the switch on
 * it denoises the resolved image. The reference's `CAMERA FIREFLYC` key of .lum v4 files stays unread, as in the reference. */
typedef struct LuminaryFireflySettings {
  bool enabled;     /* false */
  uint32_t buckets; /* 8: 4 ... 16 */
} LuminaryFireflySettings;
typedef struct LuminaryFireflyStats {
  uint64_t frames_resolved, frames_skipped;                   /* result images resolved / left alone under adaptive sampling, since the host was created */
  uint32_t last_rewritten, last_trimmed, last_nonfinite;      /* of the last resolve: pixels written, buckets left out of a mean, pixels with a non-finite bucket */
  uint32_t buckets;                                           /* buckets the main device holds (0: none) */
  uint64_t bytes;                                             /* ... and their bytes */
} LuminaryFireflyStats;
LUMINARY_API LuminaryResult luminary_ext_set_firefly_rejection(LuminaryHost* host, const LuminaryFireflySettings* settings);
LUMINARY_API LuminaryResult luminary_ext_get_firefly_rejection(LuminaryHost* host, LuminaryFireflySettings* settings);
/* The mean radiance of the full frame after the resolve (rgb interleaved, width*height*3 floats), whatever the outputs do: no local error minimisation, no
 * denoiser. Needs the switch on and at least one sample. */
LUMINARY_API LuminaryResult luminary_ext_get_robust_radiance(LuminaryHost* host, float* rgb, uint32_t width, uint32_t height);
LUMINARY_API LuminaryResult luminary_ext_get_firefly_stats(LuminaryHost* host, LuminaryFireflyStats* out);
/* ID mattes (include/lum_core.h lumc_render_first_hits; csrc/host/matte.h): which instances and which materials a pixel's first hits saw, ranked
 * by the share of its samples - what a selection outline, a matte per object with anti-aliased edges (depth of field and the shutter included) or a grade per
 * object needs, and what luminary_host_get_pixel_info, one ray of one pixel, cannot tell. Rendered on demand on the main device over the whole frame, with one
 * closest-hit pass per sample id and no shading; the accumulation is not touched. Where the denoiser is on and its guides are due, the same rays make them.
 *   luminary_ext_render_mattes  samples 1 ... 1024 (0 = 4), layers LUMINARY_MATTE_LAYER_INSTANCE | LUMINARY_MATTE_LAYER_MATERIAL. 68 bytes per pixel and layer.
 *   luminary_ext_get_matte      one layer, ranks 1 ... 8: ids and coverage planar [ranks][width * height] (either may be NULL), rank 0 the id with most samples,
 *                               ties by ascending id, coverage = samples of the id / samples; ranks a pixel does not fill hold LUMINARY_MATTE_ID_EMPTY and 0.
 *                               LUMINARY_MATTE_ID_MISS / _OCEAN / _PARTICLE stand for first hits that are no triangle, in both layers. A pixel that saw more than
 *                               eight ids keeps the first eight it saw (LuminaryMatteStats::dropped_pixels counts such pixels).
 *   luminary_ext_get_matte_mask mask [width * height] = the share of a pixel's samples whose id is among ids[0 .. count), count <= 16.
 *   luminary_ext_get_first_hit_guides  the denoiser's first-hit guides of the frame, planar: albedo [3][width * height], normal [3][...], depth [width * height]
 *                               (-1: nothing hit); each may be NULL. Rendered with the denoiser's guide_samples where the host holds none.
 * A wrong layer, rank count, id count or frame size is LUMINARY_ERROR_INVALID_API_ARGUMENT; the getters before any luminary_ext_render_mattes, or after an edit of
 * the scene since, are LUMINARY_ERROR_API_EXCEPTION with a line in the log. */
#define LUMINARY_MATTE_LAYER_INSTANCE 1u
#define LUMINARY_MATTE_LAYER_MATERIAL 2u
#define LUMINARY_MATTE_ID_EMPTY 0xFFFFFFFFu
#define LUMINARY_MATTE_ID_MISS 0xFFFFFFFEu
#define LUMINARY_MATTE_ID_OCEAN 0xFFFFFFFDu
#define LUMINARY_MATTE_ID_PARTICLE 0xFFFFFFFCu
typedef struct LuminaryMatteStats {
  uint64_t renders;            /* luminary_ext_render_mattes calls that ran, since the host was created */
  uint64_t bytes;              /* held by the main device's matte planes */
  uint32_t valid;              /* 1: the getters would answer */
  uint32_t samples, layers;    /* of the last render */
  uint32_t dropped_pixels[2];  /* pixels that saw more than eight ids: instance layer, material layer */
  uint32_t reserved;
  double seconds;              /* the last render, first-hit rays included */
} LuminaryMatteStats;
LUMINARY_API LuminaryResult luminary_ext_render_mattes(LuminaryHost* host, uint32_t samples, uint32_t layers);
LUMINARY_API LuminaryResult luminary_ext_get_matte(LuminaryHost* host, uint32_t layer, uint32_t ranks, uint32_t* ids, float* coverage, uint32_t width, uint32_t height);
LUMINARY_API LuminaryResult luminary_ext_get_matte_mask(LuminaryHost* host, uint32_t layer, const uint32_t* ids, uint32_t count, float* mask, uint32_t width, uint32_t height);
LUMINARY_API LuminaryResult luminary_ext_get_matte_stats(LuminaryHost* host, LuminaryMatteStats* out);
LUMINARY_API LuminaryResult luminary_ext_get_first_hit_guides(LuminaryHost* host, float* albedo, float* normal, float* depth, uint32_t width, uint32_t height);
/* Image history (include/lum_core.h lumc_set_history / lumc_history_carry / lumc_history_blend; csrc/host/history.h): while it is on, a restart
 * of the integration whose only cause is a move of the thin-lens camera (luminary_host_set_camera with nothing changed but pos, rotation, thin_lens.fov,
 * thin_lens.aperture_size and object_distance - luminary_ext_camera_change_carries_history) keeps the image as it was last shown: the next output reprojects it
 * into the new camera through the first-hit guides and blends it with the new accumulation, shown = (W C + N cur) / (W + N). The stage runs in the output chain after
 * the denoiser and before bloom, for beauty images of the whole frame in the default shading mode, never for the undersampling preview's coarse images; the guides
 * are then rendered for every accumulation (the denoiser's guide_samples), with the denoiser on or off. Every other restart - any other entity, a material, a mesh, an
 * instance, the device partition, a frame-size change, a physical camera, a lens change, a shutter render, luminary_host_start_new_render - drops the history, with a
 * line in the log. Several moves without an output in between carry from the older frame. An accumulation driven by adaptive sampling is skipped and counted.
 * Off by default; setting it does not restart the integration; with it off no output changes a byte. luminary_ext_get_radiance, _get_accumulators, _get_denoised and the
 * mattes are never affected.
 *   luminary_ext_set_history        LUMINARY_ERROR_INVALID_API_ARGUMENT with a line in the log: max_history not > 0, depth_tolerance not >= 0, normal_threshold outside
 *                                   [-1, 1], clamp_sigma not >= 0, or a value that is not finite.
 *   luminary_ext_get_history_image  the image as last shown before bloom, interleaved rgb [height][width][3], and its weight plane (samples it stands for); each may
 *                                   be NULL. LUMINARY_ERROR_API_EXCEPTION while there is none (off, before the first output, after a drop). */
typedef struct LuminaryHistorySettings {
  bool enabled;            /* false */
  float max_history;       /* cap of the carried weight, in samples: 32 */
  float depth_tolerance;   /* a tap is refused when its depth differs from the reprojected distance by more than this fraction: 0.02 */
  float normal_threshold;  /* ... or when the dot product of the two normals is below this: 0.9 */
  float clamp_sigma;       /* > 0: the carried colour is clamped to mean +- clamp_sigma sigma of the new image's 3 x 3 neighbourhood; 0: off */
} LuminaryHistorySettings;
typedef struct LuminaryHistoryStats {
  uint64_t frames_carried, frames_dropped, frames_skipped;  /* accumulations that started from a reprojected frame / drops of a held frame / outputs skipped under adaptive sampling */
  uint32_t last_carried, last_rejected, last_off;            /* pixels of the last reprojection: carried; refused by the depth / normal / weight tests; behind or off the old frame */
  uint32_t valid;                                            /* 1: luminary_ext_get_history_image would answer */
  uint64_t bytes;                                            /* held by the main device's state and carried planes */
  double seconds;                                            /* device time of the history kernels while the core profiles (lumc_set_profiling), else 0 */
  char last_drop[96];                                        /* the last drop's cause, empty if none */
} LuminaryHistoryStats;
LUMINARY_API LuminaryResult luminary_ext_set_history(LuminaryHost* host, const LuminaryHistorySettings* settings);
LUMINARY_API LuminaryResult luminary_ext_get_history(LuminaryHost* host, LuminaryHistorySettings* settings);
LUMINARY_API LuminaryResult luminary_ext_get_history_image(LuminaryHost* host, float* rgb, float* weight, uint32_t width, uint32_t height);
LUMINARY_API LuminaryResult luminary_ext_get_history_stats(LuminaryHost* host, LuminaryHistoryStats* out);
/* Whether replacing camera `old` by `input` restarts the integration AND keeps the history (see above); false for a change that does not restart at all. */
LUMINARY_API LuminaryResult luminary_ext_camera_change_carries_history(const LuminaryCamera* input, const LuminaryCamera* old, bool* carries);
/* Image history, motion (include/lum_core.h lumc_set_history_motion; csrc/host/history.h "Motion"): an extension of the history, off by default.
 * While history and motion are on, a restart whose only cause is luminary_ext_set_instance_transforms keeps the shown image too - alone or together with camera moves
 * that carry -: every pixel is reprojected through the old and new transform of the instance its first hit saw (its owner), a pixel takes nothing from a tap another
 * moved instance or the background owned, and the weight carried on a moved instance is capped by motion_max_history, since its lighting has changed even where its
 * surface has not. A move of an instance with an emissive material drops the history ("a moved instance emits"), as every other cause does with the string it had.
 * Moved lights and shadows are not detected, only damped by the cap and the clamp; deforming meshes still drop. The guide render of an accumulation then makes the
 * owner plane as well (4 + 4 bytes per pixel, 32 + 128 bytes per instance). With the motion off nothing of this is allocated or launched and every output keeps its
 * bytes. Setting it does not restart the integration; switching it off drops the shown frame only while a carry granted for an instance move is still due
 * ("the history's motion was switched off"). Under the physical camera an instance move drops as it always did.
 *   luminary_ext_set_history_motion               LUMINARY_ERROR_INVALID_API_ARGUMENT with a line in the log: motion_max_history not > 0 or not finite.
 *   luminary_ext_instance_change_carries_history  whether luminary_ext_set_instance_transforms with these arguments would keep the history as the host stands
 *                                                 (false with history or motion off, for no instances, or where an instance that changes emits).
 *   luminary_ext_get_history_owner                the owner planes [height][width] of the shown frame and of the current guides (LUMINARY_MATTE_ID_* for first hits that
 *                                                 are no triangle); each may be NULL. LUMINARY_ERROR_API_EXCEPTION where the plane asked for is not held.
 *   luminary_ext_get_history_transforms           8 words per instance as the device holds them: the transforms the shown frame was shown with and the current ones;
 *                                                 each may be NULL; *shown_instances: how many the shown frame holds. */
typedef struct LuminaryHistoryMotionSettings {
  bool enabled;              /* false */
  float motion_max_history;  /* cap of the carried weight of pixels on a moved instance, in samples: 8 */
} LuminaryHistoryMotionSettings;
typedef struct LuminaryHistoryMotionStats {
  uint64_t frames_carried;   /* reprojections that went through the instance records */
  uint64_t bytes;            /* owner planes, transform snapshot, records on the main device */
  uint32_t instances_moved, instances_same, instances_void;  /* of the last such reprojection */
  uint32_t last_moved_pixels, last_moved_carried;            /* pixels whose owner moved; those of them that carried */
  uint32_t valid;            /* 1: the shown frame holds its owner plane and transforms: an instance move would carry */
  double owner_seconds, motion_seconds, reproject_seconds;   /* device time of the three launches while the core profiles, else 0 */
} LuminaryHistoryMotionStats;
LUMINARY_API LuminaryResult luminary_ext_set_history_motion(LuminaryHost* host, const LuminaryHistoryMotionSettings* settings);
LUMINARY_API LuminaryResult luminary_ext_get_history_motion(LuminaryHost* host, LuminaryHistoryMotionSettings* settings);
LUMINARY_API LuminaryResult luminary_ext_get_history_motion_stats(LuminaryHost* host, LuminaryHistoryMotionStats* out);
LUMINARY_API LuminaryResult luminary_ext_instance_change_carries_history(LuminaryHost* host, const LuminaryInstance* instances, uint32_t count, bool* carries);
LUMINARY_API LuminaryResult luminary_ext_get_history_owner(LuminaryHost* host, uint32_t* shown_owner, uint32_t* current_owner, uint32_t width, uint32_t height);
LUMINARY_API LuminaryResult luminary_ext_get_history_transforms(LuminaryHost* host, float* shown_transforms, float* current_transforms, uint32_t instances, uint32_t* shown_instances);
/* out[0] closest-hit rays, [1] shadow rays, [2] light-BVH queries, [3] shaded vertices, [4] BVH nodes visited, [5] triangles tested. */
LUMINARY_API LuminaryResult luminary_ext_get_ray_counters(LuminaryHost* host, uint64_t out[8]);
/* The lumc context of this host (include/lum_core.h), for callers that drive passes themselves. */
LUMINARY_API void* luminary_ext_get_core_context(LuminaryHost* host);

#ifdef __cplusplus
}
#endif

#endif
