"""ctypes bindings of the C ABI (include/functracer_hip.h, functracer_amd/host/host_api.h).

Plumbing only: structs, prototypes and a generic `SceneBuilder` that drives any library exporting
the builder half of the ABI under a symbol prefix (`ft_` for the HIP product; the test-only CPU
oracle exports the same shape under `fto_`, bound in oracle/ft_oracle_py.py).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

FT_OK = 0
STATUS_NAMES = {0: "FT_OK", -1: "FT_ERR_INVALID", -2: "FT_ERR_NO_DEVICE", -3: "FT_ERR_HIP", -4: "FT_ERR_UNSUPPORTED",
                -5: "FT_ERR_STATE", -6: "FT_ERR_OVERFLOW", -7: "FT_ERR_BUILD"}

# Scene.Primitive (Scene.fs:10-17) and Csg ops (Scene.fs:36-39)
CIRCLE, SQUARE, CUBE, SPHERE, PLANE, CONE, SOLID_CYLINDER, CYLINDER = range(8)
UNION, INTERSECT, SUBTRACT, EXCLUDE = range(4)
TRANSLATE, SCALE, ROTATE = range(3)

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)


class FtError(RuntimeError):
    def __init__(self, status, message=""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")


class ft_transform(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("v", C.c_double * 3), ("angle", C.c_double)]


class ft_material(C.Structure):
    _fields_ = [("colour", C.c_double * 3), ("roughness", C.c_double), ("reflectance", C.c_double),
                ("shineyness", C.c_double), ("apply_lighting", C.c_int32), ("_pad", C.c_int32)]


class ft_camera(C.Structure):
    _fields_ = [("o", C.c_double * 3), ("look_at", C.c_double * 3), ("up", C.c_double * 3), ("fov_y", C.c_double),
                ("aspect_ratio", C.c_double), ("has_focus", C.c_int32), ("_pad", C.c_int32),
                ("focal_length", C.c_double), ("aperture_angular_size", C.c_double)]


class ft_rect(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class ft_stats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_shadow", C.c_uint64), ("rays_reflect", C.c_uint64),
                ("rays_traced", C.c_uint64), ("rays_reference_equivalent", C.c_double), ("hits_primary", C.c_uint64),
                ("csg_overflow", C.c_uint64), ("kernel_ms", C.c_double), ("wall_ms", C.c_double),
                ("trace_kernel_ms", C.c_double), ("algorithmic_bytes", C.c_uint64), ("n_launches", C.c_int32),
                ("n_chunks", C.c_int32), ("hits_total", C.c_uint64), ("algorithmic_bytes_closest", C.c_uint64),
                ("algorithmic_bytes_shade", C.c_uint64), ("rays_tail", C.c_uint64), ("rays_primary_culled", C.c_uint64),
                ("algorithmic_bytes_primary", C.c_uint64), ("rays_shadow_primary", C.c_uint64), ("rays_reflect_primary", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ft_aov(C.Structure):
    _fields_ = [("t", c_double_p), ("p", c_double_p), ("n", c_double_p), ("colour", c_double_p), ("material", c_double_p),
                ("leaf", c_int32_p), ("node", c_int32_p), ("triangle", c_int32_p)]


class ft_denoise_params(C.Structure):
    """ft_denoise's parameters (include/functracer_hip.h): a-trous iterations 0 .. 6, the three edge-stopping sigmas (0 = term off),
    demodulation by the material colour and the variance-guided colour term."""
    _fields_ = [("iterations", C.c_int32), ("demodulate", C.c_int32), ("use_variance", C.c_int32), ("_pad", C.c_int32),
                ("sigma_colour", C.c_double), ("sigma_normal", C.c_double), ("sigma_position", C.c_double),
                ("albedo_floor", C.c_double), ("variance_floor", C.c_double)]


# Context.denoise's defaults (also the CLI's, functracer_amd/host/Program.cpp)
DENOISE_DEFAULTS = dict(iterations=5, sigma_colour=0.6, sigma_normal=0.3, sigma_position=0.0, demodulate=1, albedo_floor=1e-3,
                        use_variance=0, variance_floor=1e-4)

DENOISE_SIGNATURE = [C.c_void_p, C.POINTER(ft_camera), C.c_int32, C.c_int32, C.c_int32, c_double_p, C.c_int32, C.c_uint64, C.POINTER(ft_rect),
                     C.c_int32, C.POINTER(ft_denoise_params), C.c_int32, C.c_void_p, C.POINTER(ft_stats)]


class ft_temporal_params(C.Structure):
    """ft_temporal_accumulate's parameters (include/functracer_hip.h): the history length at which the running mean turns into an
    exponential average, whether the means replace the frame in HBM, and the two surface tests of a history tap."""
    _fields_ = [("max_history", C.c_int32), ("to_frame", C.c_int32), ("min_normal_dot", C.c_double), ("position_tolerance_px", C.c_double)]


# Context.temporal_accumulate's defaults
TEMPORAL_DEFAULTS = dict(max_history=32, to_frame=0, min_normal_dot=0.9, position_tolerance_px=4.0)

# ft_temporal_* (include/functracer_hip.h): frames along a camera path accumulated by reprojection.
TEMPORAL_SIGNATURES = [
    ("ft_temporal_begin", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ft_rect), C.c_int32]),
    ("ft_temporal_accumulate", C.c_int32, [C.c_void_p, C.POINTER(ft_camera), C.c_int32, c_double_p, C.c_int32, C.c_uint64,
                                           C.POINTER(ft_temporal_params), C.c_int32, C.c_void_p, C.POINTER(ft_stats)]),
    ("ft_temporal_fetch", C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("ft_temporal_status", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("ft_temporal_end", C.c_int32, [C.c_void_p]),
]


class ft_temporal_clamp_params(C.Structure):
    """ft_temporal_set_clamp's parameters (include/functracer_hip.h, clause 3a): the radius of the neighbourhood (1 .. 3), the history
    length a clamped pixel keeps at most, and the box mu +- (gamma * sd + floor)."""
    _fields_ = [("radius", C.c_int32), ("clamped_history", C.c_int32), ("gamma", C.c_double), ("floor", C.c_double)]


# Context.temporal_set_clamp's defaults
TEMPORAL_CLAMP_DEFAULTS = dict(radius=1, clamped_history=1, gamma=1.0, floor=1e-4)

TEMPORAL_SIGNATURES += [
    ("ft_temporal_set_clamp", C.c_int32, [C.c_void_p, C.POINTER(ft_temporal_clamp_params)]),
    ("ft_temporal_clamp_status", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
]


# Moving rigid objects under a temporal accumulation (include/functracer_hip.h): not part of the generic builder, which also drives the oracle.
MOTION_SIGNATURES = [
    ("ft_sg_set_transform", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(ft_transform), C.c_int32]),
    ("ft_scene_commit_moved", C.c_int32, [C.c_void_p]),
    ("ft_debug_leaf_matrices", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), c_double_p, c_double_p]),
]
# ft_debug_moved_commits (option "moved_in_place"): its four values, in order, and what `full_reason` says
MOVED_COMMITS_SIGNATURE = ("ft_debug_moved_commits", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)])
MOVED_COMMITS_FIELDS = ("in_place", "full", "full_reason", "pairs_refit")
MOVED_NOT_FULL, MOVED_OPTION_OFF, MOVED_PENDING, MOVED_DIFFERS = 0, 1, 2, 3
# ft_scene_commit_moved_enqueue / ft_scene_commit_lights_enqueue / ft_debug_pose_queue (include/functracer_hip.h, "queued pose and light
# commits"): the hook's eight values, in order, and the reasons a call took the blocking path
POSE_QUEUE_SIGNATURES = [
    ("ft_scene_commit_moved_enqueue", C.c_int32, [C.c_void_p]),
    ("ft_scene_commit_lights_enqueue", C.c_int32, [C.c_void_p]),
    ("ft_debug_pose_queue", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
]
POSE_QUEUE_FIELDS = ("moved_queued", "moved_blocking", "moved_reason", "lights_queued", "lights_blocking", "lights_reason", "sets", "pending")
POSE_QUEUED, POSE_HOST_ONLY, POSE_PENDING, POSE_DIFFERS, POSE_PAIR_CHANGED = 0, 1, 2, 3, 4
POSE_SETS_MAX = 9       # frame slots + FT_TEMPORAL_QUEUE_DEPTH + 1
# ft_scene_commit_deformed_enqueue / ft_debug_deform_queue (include/functracer_hip.h, "queued deform commits"): the hook's eight values,
# in order, and the reasons a call took the blocking path
DEFORM_QUEUE_SIGNATURES = [
    ("ft_scene_commit_deformed_enqueue", C.c_int32, [C.c_void_p]),
    ("ft_debug_deform_queue", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
]
DEFORM_QUEUE_FIELDS = ("queued", "blocking", "reason", "sets", "pending", "retired_for_set", "carried", "reserved")
(DEFORM_QUEUED, DEFORM_HOST_ONLY, DEFORM_MULTI_DEVICE, DEFORM_FIRST_REFIT, DEFORM_REBUILD, DEFORM_LIGHT_SPACE, DEFORM_TEMPORAL_FOLLOW) = range(7)
GEO_SETS_MAX = 9        # frame slots + FT_TEMPORAL_QUEUE_DEPTH + 1


# Deforming meshes (include/functracer_hip.h): new vertices for an existing bspMesh node, committed by a refit of its tree on the device.
DEFORM_SIGNATURES = [
    ("ft_sg_set_mesh_triangles", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int64]),
    ("ft_scene_commit_deformed", C.c_int32, [C.c_void_p]),
    ("ft_scene_tree_quality", C.c_int32, [C.c_void_p, C.c_int32, c_double_p]),
]

# Morph targets (include/functracer_hip.h): key shapes resident in device memory, weights per frame; ft_debug_morph's counts, in order
MAX_MORPH_TARGETS = 16
MORPH_SIGNATURES = [
    ("ft_sg_set_mesh_targets", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32, C.c_int64]),
    ("ft_sg_set_mesh_weights", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32]),
    ("ft_debug_morph", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), c_double_p]),
]
MORPH_FIELDS = ("device_commits", "device_meshes", "host_meshes", "resident_bytes")

# Skinning (include/functracer_hip.h): indices and weights per corner, a palette of 3x4 bone matrices per pose; ft_debug_skin's counts are MORPH_FIELDS
MAX_SKIN_BONES = 256
MAX_SKIN_INFLUENCES = 4
SKIN_SIGNATURES = [
    ("ft_sg_set_mesh_skin", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), c_double_p, C.c_int32, C.c_int64]),
    ("ft_sg_set_mesh_bones", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32]),
    ("ft_debug_skin", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
]
# Dual-quaternion palettes (include/functracer_hip.h, "dual-quaternion skinning"): 8 doubles per bone; ft_debug_skin_dq's counts are SKIN_DQ_FIELDS
SKIN_DQ_SIGNATURES = [
    ("ft_sg_set_mesh_bones_dq", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32]),
    ("ft_debug_skin_dq", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
]
SKIN_DQ_FIELDS = ("device_commits", "device_meshes", "host_meshes", "palette_kind")


# Moving lights (include/functracer_hip.h): new values for an existing light, committed without a flatten or a BVH build.
LIGHT_SIGNATURES = [
    ("ft_scene_set_directional", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, c_double_p]),
    ("ft_scene_set_soft_directional", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_double, c_double_p]),
    ("ft_scene_set_positional", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, c_double_p, c_double_p]),
    ("ft_scene_commit_lights", C.c_int32, [C.c_void_p]),
]


# ft_debug_mesh_trees (include/functracer_hip.h): the mesh trees as they lie in HBM, for the tests' structure checker.
MESH_TREES_SIGNATURE = [C.c_void_p, C.POINTER(C.c_int64)] + [C.c_void_p] * 9
BSP_NODE_DTYPE = np.dtype([("bmin", np.float64, 3), ("bmax", np.float64, 3), ("left", np.int32), ("right", np.int32), ("axis", np.uint32), ("pad", np.uint32)])
BVH_JOB_FIELDS = ["mesh", "first_global", "n", "node_base", "leaf_base", "tri_base", "wide_base", "coarse_first", "coarse_count"]


class ft_temporal_filter_params(C.Structure):
    """ft_temporal_filter's parameters (include/functracer_hip.h): a-trous iterations 0 .. 6, demodulation by the material colour, the
    history length below which the spatial variance estimate steps in, whether the result replaces the frame in HBM, the three
    edge-stopping sigmas (0 = term off) and the two floors."""
    _fields_ = [("iterations", C.c_int32), ("demodulate", C.c_int32), ("min_history", C.c_int32), ("to_frame", C.c_int32),
                ("sigma_colour", C.c_double), ("sigma_normal", C.c_double), ("sigma_position", C.c_double),
                ("albedo_floor", C.c_double), ("variance_floor", C.c_double)]


# Context.temporal_filter's defaults
TEMPORAL_FILTER_DEFAULTS = dict(iterations=4, demodulate=1, min_history=4, to_frame=0, sigma_colour=2.0, sigma_normal=0.3, sigma_position=0.0,
                                albedo_floor=1e-3, variance_floor=1e-6)

TEMPORAL_FILTER_SIGNATURE = [C.c_void_p, C.POINTER(ft_camera), C.c_int32, c_double_p, C.c_int32, C.c_uint64, C.POINTER(ft_temporal_filter_params),
                             C.c_int32, C.c_void_p, c_double_p, C.POINTER(ft_stats)]

# ft_temporal_enqueue / ft_temporal_wait (include/functracer_hip.h): the accumulate and its filter as one queued call.
TEMPORAL_QUEUE_DEPTH = 4
TEMPORAL_QUEUE_SIGNATURES = [
    ("ft_temporal_enqueue", C.c_int32, [C.c_void_p, C.POINTER(ft_camera), C.c_int32, c_double_p, C.c_int32, C.c_uint64, C.POINTER(ft_temporal_params),
                                        C.POINTER(ft_temporal_filter_params), C.c_int32, C.c_void_p]),
    ("ft_temporal_wait", C.c_int32, [C.c_void_p, C.POINTER(ft_stats)]),
]


# ft_render_aov channels: (name, dtype, components per pixel, value of a pixel whose ray misses everything)
AOV_CHANNELS = [("t", np.float64, 1, np.inf), ("p", np.float64, 3, 0.0), ("n", np.float64, 3, 0.0), ("colour", np.float64, 3, 0.0),
                ("material", np.float64, 3, 0.0), ("leaf", np.int32, 1, -1), ("node", np.int32, 1, -1), ("triangle", np.int32, 1, -1)]


# ft_debug_classify_reuse: its four counts, in order
CLASSIFY_REUSE_FIELDS = ("classified", "reused", "windows_launched", "windows_skipped")
# ft_debug_block_lists: an entry of a block's candidate list (ft_device.h, kListEntryWords) and the header of a block that has none
LIST_ENTRY_DTYPE = np.dtype([("tri", np.uint32), ("orig", np.uint32), ("x0", np.float32), ("x1", np.float32), ("y0", np.float32), ("y1", np.float32)])
LIST_NONE = 0xFFFFFFFF
# ft_debug_edge_records: a record is three lines (a, b, c) as floats (ft_device.h, kEdgeFloats)
EDGE_RECORD_SHAPE = (3, 3)
# ft_debug_ls_retree: the eight values of a pair's row, in order ("light_space_retree")
LS_RETREE_FIELDS = ("rec", "leaf", "light", "n_tris", "ls_first", "retreed", "block", "block_nodes")


class fth_options(C.Structure):
    _fields_ = [("camera", ft_camera), ("res_h", C.c_int32), ("res_v", C.c_int32), ("samples", C.c_int32), ("corner", C.c_int32)]


BUILDER_SIGNATURES = [
    ("sg_primitive", C.c_int32, [C.c_void_p, C.c_int32]),
    ("sg_triangle", C.c_int32, [C.c_void_p, c_double_p]),
    ("sg_bsp_mesh", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int64]),
    ("sg_transform", C.c_int32, [C.c_void_p, C.POINTER(ft_transform), C.c_int32, C.c_int32]),
    ("sg_material", C.c_int32, [C.c_void_p, C.POINTER(ft_material), C.c_int32]),
    ("sg_hue_shift", C.c_int32, [C.c_void_p, C.c_double, C.c_int32]),
    ("sg_ignore_light", C.c_int32, [C.c_void_p, C.c_int32]),
    ("sg_group", C.c_int32, [C.c_void_p, c_int32_p, C.c_int32]),
    ("sg_csg", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    ("sg_texture_grid", C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32]),
    ("sg_texture_image", C.c_int32, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, c_double_p, C.c_int32, C.c_int32]),
    ("scene_clear", C.c_int32, [C.c_void_p]),
    ("scene_set_objects", C.c_int32, [C.c_void_p, C.c_int32]),
    ("scene_add_directional", C.c_int32, [C.c_void_p, c_double_p, c_double_p]),
    ("scene_add_soft_directional", C.c_int32, [C.c_void_p, c_double_p, C.c_int32, C.c_double, c_double_p]),
    ("scene_add_positional", C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("scene_commit", C.c_int32, [C.c_void_p]),
]


# ft_progressive_* (include/functracer_hip.h): progressive accumulation over one fixed request.
PROGRESSIVE_SIGNATURES = [
    ("ft_progressive_begin", C.c_int32, [C.c_void_p, C.POINTER(ft_camera), C.c_int32, C.c_int32, C.c_int32, C.POINTER(ft_rect), C.c_int32,
                                         C.c_double, C.c_int32]),
    ("ft_progressive_pass", C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(ft_stats)]),
    ("ft_progressive_fetch", C.c_int32, [C.c_void_p, c_double_p, c_double_p, C.POINTER(C.c_uint32)]),
    ("ft_progressive_status", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("ft_progressive_end", C.c_int32, [C.c_void_p]),
]


class fth_builder(C.Structure):
    _fields_ = [(name, C.CFUNCTYPE(res, *args)) for name, res, args in BUILDER_SIGNATURES]


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def vec3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def load_library(path):
    if not os.path.exists(path):
        raise FtError(-2, f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (there is no Python/CPU fallback)")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def bind_builder(lib, prefix):
    """Set prototypes for the builder functions `prefix`sg_* / `prefix`scene_* and return an fth_builder table."""
    table = fth_builder()
    for name, res, args in BUILDER_SIGNATURES:
        fn = getattr(lib, prefix + name)
        fn.restype = res
        fn.argtypes = args
        setattr(table, name, C.cast(fn, C.CFUNCTYPE(res, *args)))
    return table


def transform_array(ops):
    """ft_transform[len(ops)] of ('translate', v) | ('scale', v) | ('rotate', axis, angle_rad) entries."""
    arr = (ft_transform * len(ops))()
    for i, op in enumerate(ops):
        kind = {"translate": TRANSLATE, "scale": SCALE, "rotate": ROTATE}[op[0]]
        arr[i].kind = kind
        v = op[1]
        if kind == SCALE and np.isscalar(v):
            v = (v, v, v)
        arr[i].v = (C.c_double * 3)(*[float(x) for x in v])
        arr[i].angle = float(op[2]) if kind == ROTATE else 0.0
    return arr


class SceneBuilder:
    """Mirror of the Scene.fs constructors over a C context (`lib`, `prefix`, `ctx` pointer)."""

    def __init__(self, lib, prefix, ctx):
        self._lib, self._prefix, self._ctx = lib, prefix, ctx
        self.table = bind_builder(lib, prefix)
        last = getattr(lib, prefix + "last_error")
        last.restype = C.c_char_p
        last.argtypes = [C.c_void_p]
        self._last_error = last

    def _f(self, name):
        return getattr(self._lib, self._prefix + name)

    def last_error(self):
        return (self._last_error(self._ctx) or b"").decode()

    def _check(self, rc):
        if rc < 0:
            raise FtError(rc, self.last_error())
        return rc

    # Scene.Primitive ------------------------------------------------------------------
    def primitive(self, kind):
        return self._check(self._f("sg_primitive")(self._ctx, kind))

    def triangle(self, a, b, c):
        v = as_f64([a, b, c], (9,))
        return self._check(self._f("sg_triangle")(self._ctx, dptr(v)))

    def bsp_mesh(self, depth, triangles):
        t = as_f64(triangles).reshape(-1, 9)
        return self._check(self._f("sg_bsp_mesh")(self._ctx, int(depth), dptr(t), t.shape[0]))

    # Scene.SceneFunction --------------------------------------------------------------
    def transform(self, ops, child):
        """ops: list of ('translate', v) | ('scale', v) | ('rotate', axis, angle_rad); >1 entries = Composed."""
        return self._check(self._f("sg_transform")(self._ctx, transform_array(ops), len(ops), child))

    def translate(self, v, child):
        return self.transform([("translate", v)], child)

    def scale(self, v, child):
        return self.transform([("scale", v)], child)

    def rotate(self, axis, angle_rad, child):
        return self.transform([("rotate", axis, angle_rad)], child)

    def material(self, child, colour=(1, 1, 1), roughness=0.0, reflectance=0.0, shineyness=0.0, apply_lighting=True):
        m = ft_material()
        m.colour = (C.c_double * 3)(*[float(x) for x in colour])
        m.roughness, m.reflectance, m.shineyness = float(roughness), float(reflectance), float(shineyness)
        m.apply_lighting = 1 if apply_lighting else 0
        return self._check(self._f("sg_material")(self._ctx, C.byref(m), child))

    def hue_shift(self, angle, child):
        return self._check(self._f("sg_hue_shift")(self._ctx, float(angle), child))

    def ignore_light(self, child):
        return self._check(self._f("sg_ignore_light")(self._ctx, child))

    def group(self, children):
        arr = (C.c_int32 * len(children))(*children)
        return self._check(self._f("sg_group")(self._ctx, arr, len(children)))

    def csg(self, op, a, b):
        return self._check(self._f("sg_csg")(self._ctx, op, a, b))

    def union(self, a, b):
        return self.csg(UNION, a, b)

    def intersect(self, a, b):
        return self.csg(INTERSECT, a, b)

    def subtract(self, a, b):
        return self.csg(SUBTRACT, a, b)

    def exclude(self, a, b):
        return self.csg(EXCLUDE, a, b)

    def texture_grid(self, colour_a, colour_b, uv_ops, child):
        ops = as_f64(uv_ops).reshape(-1, 3) if len(uv_ops) else np.zeros((0, 3))
        return self._check(self._f("sg_texture_grid")(self._ctx, vec3(colour_a), vec3(colour_b), dptr(ops), ops.shape[0], child))

    def texture_image(self, pixels, uv_ops, child):
        """pixels: (height, width, 3) uint8, row 0 = top (image.SavePixelData() of an Rgb24 image)."""
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        assert px.ndim == 3 and px.shape[2] == 3
        ops = as_f64(uv_ops).reshape(-1, 3) if len(uv_ops) else np.zeros((0, 3))
        return self._check(self._f("sg_texture_image")(self._ctx, px.ctypes.data_as(C.POINTER(C.c_uint8)), px.shape[1], px.shape[0],
                                                       dptr(ops), ops.shape[0], child))

    # Scene.Scene / Light --------------------------------------------------------------
    def clear(self):
        self._check(self._f("scene_clear")(self._ctx))

    def set_objects(self, root):
        self._check(self._f("scene_set_objects")(self._ctx, root))

    def add_directional(self, direction, colour):
        self._check(self._f("scene_add_directional")(self._ctx, vec3(direction), vec3(colour)))

    def add_soft_directional(self, direction, samples, scatter_rad, colour):
        self._check(self._f("scene_add_soft_directional")(self._ctx, vec3(direction), int(samples), float(scatter_rad), vec3(colour)))

    def add_positional(self, position, falloff, colour):
        self._check(self._f("scene_add_positional")(self._ctx, vec3(position), vec3(falloff), vec3(colour)))

    def commit(self):
        self._check(self._f("scene_commit")(self._ctx))


def make_camera(o, look_at, up, fov_y_rad, aspect_ratio=1.0):
    cam = ft_camera()
    cam.o = (C.c_double * 3)(*[float(x) for x in o])
    cam.look_at = (C.c_double * 3)(*[float(x) for x in look_at])
    cam.up = (C.c_double * 3)(*[float(x) for x in up])
    cam.fov_y, cam.aspect_ratio = float(fov_y_rad), float(aspect_ratio)
    return cam


def make_rects(tiles):
    if tiles is None:
        return None, 0
    arr = (ft_rect * len(tiles))()
    for i, (x0, y0, w, h) in enumerate(tiles):
        arr[i].x0, arr[i].y0, arr[i].w, arr[i].h = int(x0), int(y0), int(w), int(h)
    return arr, len(tiles)
