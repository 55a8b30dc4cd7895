"""numpy mirrors of the contract structs in include/rt_shared.h.

Reference: shared/src/lib.rs:38-227 (#[repr(C)] Pod types).  These dtypes are
what the test/bench harness uses to build inputs for both the HIP library and
the oracle; sizes are asserted against the C header's static asserts.
"""
import numpy as np

f32 = np.float32
u32 = np.uint32

CAMERA = np.dtype([("position", f32, 3), ("direction", f32, 3), ("up", f32, 3), ("fov", f32)])
MATERIAL = np.dtype([
    ("albedo", f32, 3), ("metallic_roughness_f16", u32),
    ("emission", f32, 3), ("ior_transmission_f16", u32),
    ("specular_factor", f32), ("specular_color", f32, 3),
    ("attenuation_distance", f32), ("attenuation_color", f32, 3),
    ("thickness_factor", f32), ("diffuse_factor", f32, 3),
    ("glossiness_factor", f32), ("material_type", u32),
    ("texture_indices", u32, 8), ("_padding", f32, 2),
])
LIGHT = np.dtype([
    ("position", f32, 3), ("light_type", u32), ("color", f32, 3), ("intensity", f32),
    ("direction", f32, 3), ("range_packed", u32), ("cone_angles_packed", u32),
])
TEXTURE_INFO = np.dtype([("width", u32), ("height", u32), ("format", u32), ("mip_levels", u32),
                         ("offset", u32), ("size", u32), ("_padding", u32, 2)])
SPHERE = np.dtype([("center", f32, 3), ("radius", f32), ("material_id", u32)])
VERTEX = np.dtype([("position", f32, 3)])
TRIANGLE = np.dtype([("v0_index", u32), ("v1_index", u32), ("v2_index", u32), ("material_id", u32)])
AABB = np.dtype([("min", f32, 3), ("_padding0", f32), ("max", f32, 3), ("_padding1", f32)])
BVH_NODE = np.dtype([("bounds", AABB), ("left_child", u32), ("right_child", u32),
                     ("triangle_start", u32), ("triangle_count", u32)])
WAVEFRONT_RAY = np.dtype([
    ("origin", f32, 3), ("ray_type", u32), ("direction", f32, 3), ("bounce_depth", u32),
    ("throughput", f32, 3), ("medium_ior", f32), ("pixel_coord", u32, 2), ("inv_pdf", f32),
    ("t_min", f32), ("t_max", f32), ("wavelength_channel", u32), ("active", u32),
])
WAVEFRONT_COUNTERS = np.dtype([
    ("total_rays_generated", u32), ("rays_per_bounce", u32, 8), ("active_bounce_depths", u32),
    ("max_bounce_depth", u32), ("frame_seed", u32), ("_padding", u32, 3),
])
SCENE_METADATA_OFFSETS = np.dtype([
    ("spheres_offset", u32), ("spheres_count", u32), ("lights_offset", u32), ("lights_count", u32),
    ("bvh_nodes_offset", u32), ("bvh_nodes_count", u32),
    ("triangle_indices_offset", u32), ("triangle_indices_count", u32),
    ("vertices_offset", u32), ("vertices_count", u32),
])
PUSH_CONSTANTS = np.dtype([
    ("resolution", f32, 2), ("camera", CAMERA), ("triangle_count", u32), ("material_count", u32),
    ("tile_offset", u32, 2), ("tile_size_packed", u32), ("total_tiles", u32, 2),
    ("triangles_per_buffer", u32), ("metadata_offsets", SCENE_METADATA_OFFSETS),
    ("packed_flags", u32), ("frame_seed", u32),
])

# rt_hip.h
RENDER_PARAMS = np.dtype([
    ("camera", CAMERA), ("width", u32), ("height", u32), ("spp", u32), ("max_bounces", u32),
    ("mode", u32), ("frame_seed", u32), ("tile_size", u32), ("tile_rank", u32), ("tile_world", u32),
    ("flags", u32),
])
STATS = np.dtype([
    ("rays", np.uint64), ("primary_rays", np.uint64), ("continuation_rays", np.uint64), ("shadow_rays", np.uint64),
    ("pixels", np.uint64),
    ("node_visits", np.uint64), ("tri_tests", np.uint64),
    ("kernel_ms", np.float64), ("wall_ms", np.float64),
    ("node_bytes", np.uint64), ("tri_bytes", np.uint64), ("scene_bytes", np.uint64),
    ("bvh_nodes", u32), ("bvh_depth", u32), ("n_devices", u32), ("flags", u32),
    ("texture_bytes", np.uint64), ("n_textures", u32), ("tree_build", u32),
    ("grid_bytes", np.uint64), ("grid_build_ms", np.float64),
])
AOV = np.dtype([("albedo", f32, 3), ("depth", f32), ("normal", f32, 3), ("coverage", f32)])  # rt_aov
DENOISE_PARAMS = np.dtype([
    ("width", u32), ("height", u32), ("iterations", u32), ("flags", u32),
    ("sigma_color", f32), ("sigma_normal", f32), ("sigma_depth", f32), ("sigma_albedo", f32),
])
ADAPTIVE_PARAMS = np.dtype([("threshold", f32), ("min_samples", u32), ("flags", u32), ("_pad", u32)])  # rt_adaptive_params
ADAPTIVE_PIXEL = np.dtype([("sum", f32, 3), ("samples", f32), ("odd", f32, 3), ("error", f32)])  # rt_adaptive_pixel
SURFACE_POINT = np.dtype([("position", f32, 3), ("prim_id", u32), ("normal", f32, 3), ("material_id", u32)])  # rt_surface_point
AO_PARAMS = np.dtype([("samples", u32), ("seed", u32), ("max_distance", f32), ("bias", f32), ("flags", u32), ("_pad", u32, 3)])  # rt_ao_params
LIGHTING = np.dtype([("radiance", f32, 3), ("lit_mask", u32)])  # rt_lighting
DIRECT_LIGHT_PARAMS = np.dtype([("bias", f32), ("flags", u32), ("_pad", u32, 2)])  # rt_direct_light_params
PATH_PARAMS = np.dtype([("samples", u32), ("max_bounces", u32), ("seed", u32), ("first_sample", u32), ("flags", u32), ("_pad", u32, 3)])  # rt_path_params
PATH_RESULT = np.dtype([("radiance", f32, 3), ("segments", u32)])  # rt_path_result
PROBE = np.dtype([("position", f32, 3), ("_pad", u32)])  # rt_probe
SH9 = np.dtype([("sh", f32, (9, 3)), ("segments", u32)])  # rt_sh9
IRRADIANCE = np.dtype([("irradiance", f32, 3), ("segments", u32)])  # rt_irradiance_result
POINT_QUERY = np.dtype([("position", f32, 3), ("radius", f32)])  # rt_point_query
NEAREST = np.dtype([("position", f32, 3), ("distance", f32), ("u", f32), ("v", f32), ("prim_id", u32), ("material_id", u32)])  # rt_nearest
INSIDE_PARAMS = np.dtype([("rays", u32), ("flags", u32), ("_pad", u32, 2)])  # rt_inside_params
SWEEP = np.dtype([("origin", f32, 3), ("radius", f32), ("direction", f32, 3), ("tmax", f32)])  # rt_sweep
SWEEP_HIT = np.dtype([("position", f32, 3), ("t", f32), ("u", f32), ("v", f32), ("prim_id", u32), ("material_id", u32)])  # rt_sweep_hit
BOX = np.dtype([("center", f32, 3), ("_pad0", u32), ("half_extent", f32, 3), ("_pad1", u32)])  # rt_box
BOX_SWEEP = np.dtype([("center", f32, 3), ("_pad0", u32), ("half_extent", f32, 3), ("_pad1", u32), ("direction", f32, 3), ("tmax", f32)])  # rt_box_sweep
BOX_SWEEP_HIT = np.dtype([("normal", f32, 3), ("t", f32), ("axis", u32), ("_reserved", u32), ("prim_id", u32), ("material_id", u32)])  # rt_box_sweep_hit
OBB = np.dtype([("center", f32, 3), ("_pad0", u32), ("half_extent", f32, 3), ("_pad1", u32), ("rotation", f32, 4)])  # rt_obb
OBB_SWEEP = np.dtype([("center", f32, 3), ("_pad0", u32), ("half_extent", f32, 3), ("_pad1", u32), ("rotation", f32, 4), ("direction", f32, 3), ("tmax", f32)])  # rt_obb_sweep
TRIANGLE_QUERY = np.dtype([("v0", f32, 3), ("_pad0", u32), ("v1", f32, 3), ("_pad1", u32), ("v2", f32, 3), ("_pad2", u32)])  # rt_query_triangle
TRIANGLE_SWEEP = np.dtype([("v0", f32, 3), ("_pad0", u32), ("v1", f32, 3), ("_pad1", u32), ("v2", f32, 3), ("_pad2", u32), ("direction", f32, 3), ("tmax", f32)])  # rt_triangle_sweep
TRIANGLE_SWEEP_HIT = np.dtype([("normal", f32, 3), ("t", f32), ("axis", u32), ("_reserved", u32), ("prim_id", u32), ("material_id", u32)])  # rt_triangle_sweep_hit
TRIANGLE_CONTACT_QUERY = np.dtype([("v0", f32, 3), ("margin", f32), ("v1", f32, 3), ("_pad1", u32), ("v2", f32, 3), ("_pad2", u32)])  # rt_triangle_contact_query
TRIANGLE_CONTACT = np.dtype([("position", f32, 3), ("distance", f32), ("qu", f32), ("qv", f32), ("prim_id", u32), ("material_id", u32)])  # rt_triangle_contact
POSE = np.dtype([("position", f32, 3), ("_pad0", u32), ("rotation", f32, 4)])  # rt_pose
POSE_SWEEP = np.dtype([("position", f32, 3), ("_pad0", u32), ("rotation", f32, 4), ("direction", f32, 3), ("tmax", f32)])  # rt_pose_sweep
MESH_SWEEP_HIT = np.dtype([("normal", f32, 3), ("t", f32), ("axis", u32), ("triangle", u32), ("prim_id", u32), ("material_id", u32)])  # rt_mesh_sweep_hit
CAPSULE_SWEEP = np.dtype([("origin", f32, 3), ("radius", f32), ("axis", f32, 3), ("_pad", u32), ("direction", f32, 3), ("tmax", f32)])  # rt_capsule_sweep
CAPSULE_SWEEP_HIT = np.dtype([("position", f32, 3), ("t", f32), ("s", f32), ("_reserved", u32), ("prim_id", u32), ("material_id", u32)])  # rt_capsule_sweep_hit
CAPSULE = np.dtype([("origin", f32, 3), ("radius", f32), ("axis", f32, 3), ("_pad", u32)])  # rt_capsule
CONTACT = np.dtype([("position", f32, 3), ("distance", f32), ("s", f32), ("_reserved", u32), ("prim_id", u32), ("material_id", u32)])  # rt_contact
AOV_SAMPLES_PER_LAUNCH = 64  # RT_AOV_SAMPLES_PER_LAUNCH
DENOISE_DEMODULATE = 1  # RT_DENOISE_DEMODULATE
DENOISE_MAX_ITERATIONS = 10
DENOISE_DEFAULT_ITERATIONS = 2  # RT_DENOISE_DEFAULT_*: DESIGN.md section 4, the sweep they were chosen by
DENOISE_DEFAULT_SIGMA_COLOR = 4.0
DENOISE_DEFAULT_SIGMA_NORMAL = 1.0
DENOISE_DEFAULT_SIGMA_DEPTH = 0.1
DENOISE_DEFAULT_SIGMA_ALBEDO = 0.3
STAT_MEGAKERNEL_FALLBACK = 1
STAT_SINGLE_PASS = 2
PREPARE_SHADOW_GRIDS = 1
PREPARE_QUALITY_TREE = 2
MAX_BOUNCES = 255

EXPECTED_SIZES = {
    "CAMERA": 40, "MATERIAL": 128, "LIGHT": 52, "TEXTURE_INFO": 32, "SPHERE": 20, "VERTEX": 12,
    "TRIANGLE": 16, "AABB": 32, "BVH_NODE": 48, "WAVEFRONT_RAY": 76, "WAVEFRONT_COUNTERS": 60,
    "SCENE_METADATA_OFFSETS": 40, "PUSH_CONSTANTS": 128, "AOV": 32, "DENOISE_PARAMS": 32,
    "ADAPTIVE_PARAMS": 16, "ADAPTIVE_PIXEL": 32, "SURFACE_POINT": 32, "AO_PARAMS": 32, "LIGHTING": 16, "DIRECT_LIGHT_PARAMS": 16,
    "PATH_PARAMS": 32, "PATH_RESULT": 16, "PROBE": 16, "SH9": 112, "IRRADIANCE": 16, "POINT_QUERY": 16, "NEAREST": 32, "INSIDE_PARAMS": 16,
    "SWEEP": 32, "SWEEP_HIT": 32, "BOX": 32, "BOX_SWEEP": 48, "BOX_SWEEP_HIT": 32, "CAPSULE_SWEEP": 48, "CAPSULE_SWEEP_HIT": 32,
    "CAPSULE": 32, "CONTACT": 32, "OBB": 48, "OBB_SWEEP": 64, "TRIANGLE_QUERY": 48, "TRIANGLE_SWEEP": 64, "TRIANGLE_SWEEP_HIT": 32,
    "TRIANGLE_CONTACT_QUERY": 48, "TRIANGLE_CONTACT": 32, "POSE": 32, "POSE_SWEEP": 48, "MESH_SWEEP_HIT": 32,
}
for _name, _size in EXPECTED_SIZES.items():
    assert globals()[_name].itemsize == _size, (_name, globals()[_name].itemsize, _size)

TILE_SIZE = 128
MIN_RAY_DISTANCE = np.float32(0.00001)
INVALID_INDEX = 0xFFFFFFFF
REF_TRIANGLES_PER_BUFFER = 8388608  # src/buffers.rs:49-53
