"""functracer_amd — Python face of the MI355X-native FuncTracer render loop.

The product is `lib/libfunctracer_hip.so` (hand-written gfx950 kernels behind the C ABI of
include/functracer_hip.h) plus `lib/libfunctracer_host.so` (the host side that is F# in the
reference: SceneParser / PlyParser / Program).  This package only binds them; nothing here
computes pixels, and nothing here touches the CPU oracle under oracle/.  If the HIP library or a
GPU is missing, `Context()` raises — there is no fallback path.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import (CIRCLE, CONE, CUBE, CYLINDER, EXCLUDE, INTERSECT, PLANE, SOLID_CYLINDER, SPHERE, SQUARE, SUBTRACT, UNION,
                    FtError, SceneBuilder, make_camera)

__all__ = ["Context", "ls_topology", "PinnedArray", "ParsedScene", "parse_scene", "parse_scene_file", "jitter_pattern", "morph_blend", "skin_blend", "skin_blend_dq", "dual_quaternions", "quantise_rgba8", "write_png",
           "parse_colour", "parse_ply", "FtError", "make_camera", "HIP_LIB", "HOST_LIB", "DEFAULT_SEED"]

HIP_LIB = os.environ.get("FT_HIP_LIB") or os.path.join(_capi.LIB_DIR, "libfunctracer_hip.so")   # FT_HIP_LIB: experimental builds
HOST_LIB = os.environ.get("FT_HOST_LIB") or os.path.join(_capi.LIB_DIR, "libfunctracer_host.so")
DEFAULT_SEED = 20260104          # jitter pattern seed of the BASELINE configs
MAX_DEPTH = 8                    # Shading.fs:142

_hip = None
_host = None


def hip_lib():
    global _hip
    if _hip is None:
        lib = _capi.load_library(HIP_LIB)
        lib.ft_create.argtypes = [_capi.c_int32_p, C.c_int32, C.POINTER(C.c_void_p)]
        lib.ft_create_host_only.argtypes = [C.POINTER(C.c_void_p)]
        lib.ft_destroy.argtypes = [C.c_void_p]
        lib.ft_destroy.restype = None
        lib.ft_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        lib.ft_render.argtypes = [C.c_void_p, C.POINTER(_capi.ft_camera), C.c_int32, C.c_int32, C.c_int32, _capi.c_double_p, C.c_int32,
                                  C.c_uint64, C.POINTER(_capi.ft_rect), C.c_int32, _capi.c_double_p, C.POINTER(_capi.ft_stats)]
        lib.ft_fetch_frame.argtypes = [C.c_void_p, _capi.c_double_p]
        lib.ft_render_rgba8.argtypes = [C.c_void_p, C.POINTER(_capi.ft_camera), C.c_int32, C.c_int32, C.c_int32, _capi.c_double_p, C.c_int32,
                                        C.c_uint64, C.POINTER(_capi.ft_rect), C.c_int32, C.POINTER(C.c_uint8), C.POINTER(_capi.ft_stats)]
        lib.ft_fetch_frame_rgba8.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
        lib.ft_render_enqueue_rgba8.argtypes = [C.c_void_p, C.POINTER(_capi.ft_camera), C.c_int32, C.c_int32, C.c_int32, _capi.c_double_p, C.c_int32, C.c_uint64, C.POINTER(_capi.ft_rect), C.c_int32]
        lib.ft_host_alloc.restype = C.c_void_p
        lib.ft_host_alloc.argtypes = [C.c_size_t]
        lib.ft_host_free.restype = None
        lib.ft_host_free.argtypes = [C.c_void_p]
        lib.ft_debug_closest.argtypes = [C.c_void_p, _capi.c_double_p, _capi.c_double_p, C.c_int64, _capi.c_int32_p,
                                         _capi.c_double_p, _capi.c_double_p, _capi.c_double_p, _capi.c_double_p]
        lib.ft_debug_blocked.argtypes = [C.c_void_p, _capi.c_double_p, _capi.c_double_p, _capi.c_double_p, C.c_int64, _capi.c_int32_p]
        lib.ft_debug_colour.argtypes = [C.c_void_p, _capi.c_double_p, _capi.c_double_p, C.c_int64, C.c_int32, _capi.c_double_p]
        lib.ft_get_commit_times.argtypes = [C.c_void_p, _capi.c_double_p]
        lib.ft_debug_scene_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.ft_debug_devices.argtypes = [C.c_void_p, _capi.c_int32_p, C.c_int32]
        lib.ft_debug_classify_reuse.restype, lib.ft_debug_classify_reuse.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]
        if hasattr(lib, "ft_debug_primary_kernels"):              # (FT_HIP_LIB may name an older build: A/B runs against the parent commit's library)
            lib.ft_debug_primary_kernels.restype, lib.ft_debug_primary_kernels.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]
        lib.ft_debug_mesh_trees.restype, lib.ft_debug_mesh_trees.argtypes = C.c_int32, _capi.MESH_TREES_SIGNATURE
        lib.ft_debug_slice.argtypes = [_capi.c_double_p] * 4 + [_capi.c_int32_p, _capi.c_double_p, _capi.c_int32_p]
        lib.ft_render_enqueue.argtypes = [C.c_void_p, C.POINTER(_capi.ft_camera), C.c_int32, C.c_int32, C.c_int32, _capi.c_double_p, C.c_int32, C.c_uint64, C.POINTER(_capi.ft_rect), C.c_int32]
        lib.ft_render_wait.argtypes = [C.c_void_p, C.POINTER(_capi.ft_stats)]
        lib.ft_render_enqueue_into.argtypes = [C.c_void_p, C.POINTER(_capi.ft_camera), C.c_int32, C.c_int32, C.c_int32, _capi.c_double_p, C.c_int32, C.c_uint64, C.POINTER(_capi.ft_rect), C.c_int32, C.c_int32, C.c_void_p]
        lib.ft_get_kernel_times.argtypes = [C.c_void_p, _capi.c_double_p, _capi.c_int32_p]
        lib.ft_render_aov.argtypes = [C.c_void_p, C.POINTER(_capi.ft_camera), C.c_int32, C.c_int32, C.c_int32, _capi.c_double_p, C.c_int32,
                                      C.c_uint64, C.POINTER(_capi.ft_rect), C.c_int32, C.POINTER(_capi.ft_aov), C.POINTER(_capi.ft_stats)]
        lib.ft_denoise.argtypes = _capi.DENOISE_SIGNATURE
        lib.ft_temporal_filter.restype, lib.ft_temporal_filter.argtypes = C.c_int32, _capi.TEMPORAL_FILTER_SIGNATURE
        lib.ft_quantise_rgba8.argtypes = [_capi.c_double_p, C.c_int64, C.POINTER(C.c_uint8)]
        for name, res, args in _capi.PROGRESSIVE_SIGNATURES + _capi.TEMPORAL_SIGNATURES + _capi.TEMPORAL_QUEUE_SIGNATURES + _capi.MOTION_SIGNATURES + _capi.DEFORM_SIGNATURES + _capi.LIGHT_SIGNATURES:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if hasattr(lib, _capi.MOVED_COMMITS_SIGNATURE[0]):          # (FT_HIP_LIB may name an older build, as above)
            fn = getattr(lib, _capi.MOVED_COMMITS_SIGNATURE[0])
            fn.restype, fn.argtypes = _capi.MOVED_COMMITS_SIGNATURE[1:]
        for name, res, args in _capi.POSE_QUEUE_SIGNATURES + _capi.DEFORM_QUEUE_SIGNATURES + _capi.MORPH_SIGNATURES + _capi.SKIN_SIGNATURES + _capi.SKIN_DQ_SIGNATURES:
            if hasattr(lib, name):                                  # (FT_HIP_LIB may name an older build, as above)
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        _hip = lib
    return _hip


def host_lib():
    global _host
    if _host is None:
        lib = _capi.load_library(HOST_LIB)
        lib.fth_parse_scene.restype = C.c_void_p
        lib.fth_parse_scene.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32]
        lib.fth_parse_scene_file.restype = C.c_void_p
        lib.fth_parse_scene_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int32]
        lib.fth_scene_free.argtypes = [C.c_void_p]
        lib.fth_scene_free.restype = None
        lib.fth_scene_options.argtypes = [C.c_void_p, C.POINTER(_capi.fth_options)]
        lib.fth_scene_counts.argtypes = [C.c_void_p, _capi.c_int32_p, _capi.c_int32_p]
        lib.fth_scene_lower.argtypes = [C.c_void_p, C.POINTER(_capi.fth_builder), C.c_void_p]
        lib.fth_parse_colour.argtypes = [C.c_char_p, _capi.c_double_p]
        lib.fth_parse_ply.restype = C.c_int64
        lib.fth_parse_ply.argtypes = [C.c_char_p, _capi.c_double_p, C.c_int64, C.c_char_p, C.c_int32]
        lib.fth_jitter_pattern.argtypes = [C.c_uint64, C.c_int32, _capi.c_double_p]
        lib.fth_write_png.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]
        lib.fth_load_image.restype = C.c_int64
        lib.fth_load_image.argtypes = [C.c_char_p, _capi.c_int32_p, _capi.c_int32_p, C.POINTER(C.c_uint8), C.c_int64, C.c_char_p, C.c_int32]
        _host = lib
    return _host


class ParsedScene:
    """Result of SceneParser.parse (SceneParser.fs:360-366): (SceneOptions, Scene)."""

    def __init__(self, handle):
        self._h = handle
        opt = _capi.fth_options()
        host_lib().fth_scene_options(handle, C.byref(opt))
        self.camera = opt.camera
        self.resolution = (opt.res_h, opt.res_v)
        self.samples = opt.samples
        self.corner = bool(opt.corner)
        n_obj, n_l = C.c_int32(), C.c_int32()
        host_lib().fth_scene_counts(handle, C.byref(n_obj), C.byref(n_l))
        self.n_objects, self.n_lights = n_obj.value, n_l.value

    def lower(self, builder):
        """Hand the scene to anything with a SceneBuilder (`Context`, or the oracle in tests)."""
        rc = host_lib().fth_scene_lower(self._h, C.byref(builder.table), builder._ctx)
        if rc < 0:
            raise FtError(rc, builder.last_error())

    def __del__(self):
        if getattr(self, "_h", None) and _host is not None:
            _host.fth_scene_free(self._h)
            self._h = None


def parse_scene(text, base_dir=""):
    err = C.create_string_buffer(2048)
    h = host_lib().fth_parse_scene(text.encode(), base_dir.encode(), err, len(err))
    if not h:
        raise ValueError(err.value.decode())
    return ParsedScene(h)


def parse_scene_file(path):
    err = C.create_string_buffer(2048)
    h = host_lib().fth_parse_scene_file(os.fspath(path).encode(), err, len(err))
    if not h:
        raise ValueError(err.value.decode())
    return ParsedScene(h)


def parse_colour(text):
    rgb = np.zeros(3)
    if host_lib().fth_parse_colour(text.encode(), _capi.dptr(rgb)) != 0:
        raise ValueError("Parsing failed")
    return tuple(rgb)


def parse_ply(text):
    err = C.create_string_buffer(1024)
    n = host_lib().fth_parse_ply(text.encode(), None, 0, err, len(err))
    if n < 0:
        raise ValueError(err.value.decode())
    out = np.zeros((n, 9))
    host_lib().fth_parse_ply(text.encode(), _capi.dptr(out), n, err, len(err))
    return out


def morph_blend(base, targets, w):
    """The vertices ft_sg_set_mesh_weights declares (include/functracer_hip.h, "morph targets"), evaluated in numpy with one elementwise
    IEEE double operation per step: D_k = T_k - B, then acc = B; p = w_k * D_k; acc = acc + p for k = 0 .. K-1 in order, every term
    evaluated.  base [n, 9], targets [K, n, 9] (absolute positions), w [K]; returns [n, 9].  What the library promises bit for bit."""
    base = np.ascontiguousarray(base, dtype=np.float64).reshape(-1, 9)
    targets = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, base.shape[0], 9)
    w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if w.shape[0] != targets.shape[0]:
        raise ValueError("morph_blend: one weight per target")
    acc = base.copy()
    for k in range(targets.shape[0]):
        d = targets[k] - base
        p = w[k] * d
        acc = acc + p
    return acc


def skin_blend(shape, index, weight, bones):
    """The vertices ft_sg_set_mesh_bones declares (include/functracer_hip.h, "skinning"), evaluated in numpy with one elementwise IEEE
    double operation per step: per corner and influence j in order t_i = ((M[i][0] * x + M[i][1] * y) + M[i][2] * z) + M[i][3],
    q_i = w_j * t_i, acc_i = q_i (j = 0) or acc_i + q_i, every influence evaluated.  shape [n, 9] (or [n, 3, 3]), index and weight
    [n, 3, J] (or [3n, J]), bones [n_bones, 12] (or [n_bones, 3, 4]); returns [n, 9].  What the library promises bit for bit."""
    shape = np.ascontiguousarray(shape, dtype=np.float64).reshape(-1, 3)
    index = np.asarray(index, dtype=np.int64).reshape(shape.shape[0], -1)
    weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(shape.shape[0], -1)
    bones = np.ascontiguousarray(bones, dtype=np.float64).reshape(-1, 3, 4)
    if index.shape != weight.shape or index.shape[1] < 1:
        raise ValueError("skin_blend: one weight per index, at least one influence per corner")
    x, y, z = shape[:, 0:1], shape[:, 1:2], shape[:, 2:3]
    acc = None
    for j in range(index.shape[1]):
        m = bones[index[:, j]]                                      # [corners, 3, 4]
        px = m[:, :, 0] * x
        py = m[:, :, 1] * y
        pz = m[:, :, 2] * z
        t = px + py
        t = t + pz
        t = t + m[:, :, 3]
        q = weight[:, j:j + 1] * t
        acc = q if j == 0 else acc + q
    return np.ascontiguousarray(acc).reshape(-1, 9)


def _cross(a, b):
    """cross(a, b) of [n, 3] arrays: per component two products and one difference, one elementwise operation per step."""
    out = []
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        left = a[:, i1] * b[:, i2]
        right = a[:, i2] * b[:, i1]
        out.append(left - right)
    return np.stack(out, axis=1)


def skin_blend_dq(shape, index, weight, dq):
    """The vertices ft_sg_set_mesh_bones_dq declares (include/functracer_hip.h, "dual-quaternion skinning"), evaluated in numpy with one
    elementwise IEEE double operation per step: per corner the weighted sum of the bones' dual quaternions in slot order, a bone whose
    real part lies opposite slot 0's entering with its weight negated, normalised by the length of the real part, applied to the shape
    position.  shape [n, 9] (or [n, 3, 3]), index and weight [n, 3, J] (or [3n, J]), dq [n_bones, 8] (real w, x, y, z, then dual); returns
    [n, 9].  What the library promises bit for bit."""
    p = np.ascontiguousarray(shape, dtype=np.float64).reshape(-1, 3)
    index = np.asarray(index, dtype=np.int64).reshape(p.shape[0], -1)
    weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(p.shape[0], -1)
    dq = np.ascontiguousarray(dq, dtype=np.float64).reshape(-1, 8)
    if index.shape != weight.shape or index.shape[1] < 1:
        raise ValueError("skin_blend_dq: one weight per index, at least one influence per corner")
    with np.errstate(all="ignore"):
        r0 = dq[index[:, 0], :4]
        acc = None
        for j in range(index.shape[1]):
            d = dq[index[:, j]]                                     # [corners, 8]
            ws = weight[:, j]
            if j > 0:
                g0 = d[:, 0] * r0[:, 0]
                g1 = d[:, 1] * r0[:, 1]
                g2 = d[:, 2] * r0[:, 2]
                g3 = d[:, 3] * r0[:, 3]
                g = g0 + g1
                g = g + g2
                g = g + g3
                ws = np.where(g < 0.0, -ws, ws)                     # (a NaN g does not negate)
            q = ws[:, None] * d
            acc = q if j == 0 else acc + q
        sq = acc[:, :4] * acc[:, :4]
        n2 = sq[:, 0] + sq[:, 1]
        n2 = n2 + sq[:, 2]
        n2 = n2 + sq[:, 3]
        n = np.sqrt(n2)
        s = 1.0 / n
        u = acc * s[:, None]
        w, v, e, f = u[:, 0:1], u[:, 1:4], u[:, 4:5], u[:, 5:8]
        wp = w * p
        c = _cross(v, p) + wp
        h = _cross(v, c)
        wf = w * f
        ev = e * v
        m = wf - ev
        m = m + _cross(v, f)
        h2 = 2.0 * h
        m2 = 2.0 * m
        out = p + h2
        out = out + m2
    return np.ascontiguousarray(out).reshape(-1, 9)


def dual_quaternions(rotations, translations):
    """Palettes [n, 8] for ft_sg_set_mesh_bones_dq from unit quaternions [n, 4] (w, x, y, z) and translations [n, 3]: "rotate by r, then
    translate by t" has real part r and dual part 0.5 * (0, t) (x) r.  A convenience, not part of the bit promise."""
    r = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(translations, dtype=np.float64).reshape(-1, 3)
    if r.shape[0] != t.shape[0]:
        raise ValueError("dual_quaternions: one translation per rotation")
    rw, rv = r[:, 0:1], r[:, 1:4]
    dw = -0.5 * np.sum(t * rv, axis=1, keepdims=True)
    dv = 0.5 * (rw * t + np.cross(t, rv))
    return np.ascontiguousarray(np.concatenate([r, dw, dv], axis=1))


def jitter_pattern(n, seed=DEFAULT_SEED):
    """Jitter.pattern random Jitter.circle n on the documented seeded stream (host_api.h)."""
    out = np.zeros((n, 2))
    host_lib().fth_jitter_pattern(int(seed), int(n), _capi.dptr(out))
    return out


def quantise_rgba8(rgb):
    """Image.write's toByte (Image.fs:36)."""
    rgb = _capi.as_f64(rgb)
    n = rgb.size // 3
    out = np.zeros((n, 4), dtype=np.uint8)
    rc = hip_lib().ft_quantise_rgba8(_capi.dptr(rgb), n, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc < 0:
        raise FtError(rc)
    return out.reshape(rgb.shape[:-1] + (4,))


def write_png(path, rgba):
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = rgba.shape[:2]
    rc = host_lib().fth_write_png(os.fspath(path).encode(), rgba.ctypes.data_as(C.POINTER(C.c_uint8)), w, h)
    if rc < 0:
        raise FtError(rc, "write_png")


def load_image(path):
    """Image.Load<Rgb24> for local PNG / PPM files (Textures/Image.fs:21-26): (height, width, 3) uint8, row 0 = top."""
    lib = host_lib()
    w, h = C.c_int32(), C.c_int32()
    err = C.create_string_buffer(512)
    n = lib.fth_load_image(os.fspath(path).encode(), C.byref(w), C.byref(h), None, 0, err, 512)
    if n < 0:
        raise FtError(int(n), err.value.decode())
    out = np.empty(n, dtype=np.uint8)
    lib.fth_load_image(os.fspath(path).encode(), C.byref(w), C.byref(h), out.ctypes.data_as(C.POINTER(C.c_uint8)), n, err, 512)
    return out.reshape(h.value, w.value, 3)


class PinnedArray:
    """A numpy array over page-locked host memory from ft_host_alloc: frames copied into it arrive by one DMA at link rate
    (`with ft.PinnedArray((h, w, 3)) as frame: ctx.render(..., out=frame)`)."""

    def __init__(self, shape, dtype=np.float64):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = hip_lib().ft_host_alloc(self.nbytes)
        if not self._p:
            raise MemoryError(f"ft_host_alloc({self.nbytes}) failed")
        self.array = np.frombuffer((C.c_char * self.nbytes).from_address(self._p), dtype=dtype).reshape(shape)

    def __enter__(self):
        return self.array

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._p:
            self.array = None
            hip_lib().ft_host_free(self._p)
            self._p = None


class Context(SceneBuilder):
    """One ft_context on one MI355X.  `host_only=True` gives the test hook that can build and flatten
    scenes but never renders."""

    def __init__(self, device=0, host_only=False):
        lib = hip_lib()
        h = C.c_void_p()
        if host_only:
            rc = lib.ft_create_host_only(C.byref(h))
        else:
            ids = [int(d) for d in device] if isinstance(device, (list, tuple)) else [int(device)]
            dev = (C.c_int32 * len(ids))(*ids)                # several ids: one context that tiles every frame over those GPUs
            rc = lib.ft_create(dev, len(ids), C.byref(h))
        if rc < 0:
            raise FtError(rc, "ft_create: no usable HIP device (the HIP path has no CPU fallback)" if rc == -2 else "ft_create")
        self.device = device
        super().__init__(lib, "ft_", h)

    def close(self):
        if self._ctx:
            self._lib.ft_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        """ft_set_option: an integer tunable by name (include/functracer_hip.h lists them).  Among them "temporal_follow_deformed" (0 / 1,
        no new commit needed): commit_deformed keeps the records of the meshes it refits as the open temporal accumulation last saw them and
        the next temporal_accumulate follows their triangles."""
        self._check(self._lib.ft_set_option(self._ctx, key.encode(), int(value)))

    def render(self, camera, res_h, res_v, spp, jitter, max_depth=MAX_DEPTH, seed=DEFAULT_SEED, tiles=None, out=None, fetch=True):
        """Program.fs:54-64 on the GPU.  Returns (rgb[res_v, res_h, 3] float64, stats dict).  With
        fetch=False the frame stays in HBM (returns (None, stats)); `fetch_frame` copies it out later."""
        jitter = np.zeros((1, 2)) if spp == 0 else _capi.as_f64(jitter, (spp, 2))   # spp == 0: `samples corner` (Image.fs:125-150)
        if fetch and out is None:
            out = np.zeros((res_v, res_h, 3))
        rects, n_rects = _capi.make_rects(tiles)
        st = _capi.ft_stats()
        rc = self._lib.ft_render(self._ctx, C.byref(camera), res_h, res_v, spp, _capi.dptr(jitter), max_depth, int(seed), rects, n_rects,
                                 _capi.dptr(out) if fetch else None, C.byref(st))
        self._check(rc)
        return (out if fetch else None), st.as_dict()

    def fetch_frame(self, out):
        self._check(self._lib.ft_fetch_frame(self._ctx, _capi.dptr(out)))
        return out

    def render_rgba8(self, camera, res_h, res_v, spp, jitter, max_depth=MAX_DEPTH, seed=DEFAULT_SEED, tiles=None, out=None, fetch=True):
        """ft_render_rgba8: the frame as Image.write consumes it (Image.fs:35-44), quantised on the device.  Returns
        (rgba[res_v, res_h, 4] uint8, stats dict); with fetch=False the bytes stay in HBM until `fetch_frame_rgba8`."""
        jitter = np.zeros((1, 2)) if spp == 0 else _capi.as_f64(jitter, (spp, 2))
        if fetch and out is None:
            out = np.zeros((res_v, res_h, 4), dtype=np.uint8)
        rects, n_rects = _capi.make_rects(tiles)
        st = _capi.ft_stats()
        rc = self._lib.ft_render_rgba8(self._ctx, C.byref(camera), res_h, res_v, spp, _capi.dptr(jitter), max_depth, int(seed), rects, n_rects,
                                       out.ctypes.data_as(C.POINTER(C.c_uint8)) if fetch else None, C.byref(st))
        self._check(rc)
        return (out if fetch else None), st.as_dict()

    def fetch_frame_rgba8(self, out):
        self._check(self._lib.ft_fetch_frame_rgba8(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def render_enqueue(self, camera, res_h, res_v, spp, jitter, max_depth=MAX_DEPTH, seed=DEFAULT_SEED, tiles=None, rgba8=False, out=None):
        """ft_render_enqueue[_rgba8]: queue a frame and return; `wait()` retires what is queued.  With `out` (a PinnedArray's array, or any
        C-contiguous array of the frame's shape that outlives the frame) the copy to the host is queued behind the frame: ft_render_enqueue_into."""
        jitter = np.zeros((1, 2)) if spp == 0 else _capi.as_f64(jitter, (spp, 2))
        rects, n_rects = _capi.make_rects(tiles)
        if out is not None:
            assert out.flags["C_CONTIGUOUS"] and out.nbytes == res_h * res_v * (4 if rgba8 else 24)
            self._check(self._lib.ft_render_enqueue_into(self._ctx, C.byref(camera), res_h, res_v, spp, _capi.dptr(jitter), max_depth, int(seed), rects, n_rects,
                                                         1 if rgba8 else 0, out.ctypes.data_as(C.c_void_p)))
            return
        fn = self._lib.ft_render_enqueue_rgba8 if rgba8 else self._lib.ft_render_enqueue
        self._check(fn(self._ctx, C.byref(camera), res_h, res_v, spp, _capi.dptr(jitter), max_depth, int(seed), rects, n_rects))

    def wait(self):
        """ft_render_wait: statistics of the last queued frame; kernel_times() then holds the sums over all frames since the previous wait."""
        st = _capi.ft_stats()
        self._check(self._lib.ft_render_wait(self._ctx, C.byref(st)))
        return st.as_dict()

    def kernel_times(self):
        ms = np.zeros(5)
        n = np.zeros(5, dtype=np.int32)
        self._check(self._lib.ft_get_kernel_times(self._ctx, _capi.dptr(ms), n.ctypes.data_as(_capi.c_int32_p)))
        names = ["other", "closest", "shade", "resolve", "primary"]   # "other": the fill, k_classify (and k_resolve unless "timing" = 2); "shade": k_bounce, all levels; "closest": unused
        return {k: {"ms": float(ms[i]), "launches": int(n[i])} for i, k in enumerate(names)}

    # progressive accumulation (ft_progressive_*, include/functracer_hip.h) ---------------------------
    def progressive_begin(self, camera, res_h, res_v, max_depth=MAX_DEPTH, tiles=None, tolerance=0.0, min_samples=2):
        """Start accumulating one fixed request pass by pass (replaces any earlier accumulation).  tolerance > 0: adaptive - an 8x8 block
        stops receiving samples once it has min_samples and the standard error of every pixel's mean is within tolerance."""
        rects, n_rects = _capi.make_rects(tiles)
        self._check(self._lib.ft_progressive_begin(self._ctx, C.byref(camera), res_h, res_v, max_depth, rects, n_rects, float(tolerance), int(min_samples)))
        self._progressive = (res_h, res_v, tolerance > 0)

    def progressive_pass(self, spp, jitter, seed=DEFAULT_SEED, rgba8=False, out=None, fetch=True):
        """spp new samples (jitter: spp x 2) for every block not yet retired.  Returns (running mean frame - rgb[res_v, res_h, 3] float64, or
        rgba[res_v, res_h, 4] uint8 with rgba8 - and this pass's stats dict); with fetch=False the frame stays in HBM (returns (None, stats))."""
        res_h, res_v, _ = self._progressive_shape()
        jitter = _capi.as_f64(jitter, (int(spp), 2)) if spp > 0 else np.zeros((1, 2))
        if fetch and out is None:
            out = np.zeros((res_v, res_h, 4), dtype=np.uint8) if rgba8 else np.zeros((res_v, res_h, 3))
        st = _capi.ft_stats()
        self._check(self._lib.ft_progressive_pass(self._ctx, int(spp), _capi.dptr(jitter), int(seed), 1 if rgba8 else 0,
                                                  out.ctypes.data_as(C.c_void_p) if fetch else None, C.byref(st)))
        return (out if fetch else None), st.as_dict()

    def progressive_fetch(self):
        """(mean[res_v, res_h, 3], stderr[res_v, res_h, 3] or None for a plain accumulation, samples[res_v, res_h] uint32) of the tile
        pixels; other pixels stay 0."""
        res_h, res_v, adaptive = self._progressive_shape()
        mean, samples = np.zeros((res_v, res_h, 3)), np.zeros((res_v, res_h), dtype=np.uint32)
        se = np.zeros((res_v, res_h, 3)) if adaptive else None
        self._check(self._lib.ft_progressive_fetch(self._ctx, _capi.dptr(mean), _capi.dptr(se) if adaptive else None,
                                                   samples.ctypes.data_as(C.POINTER(C.c_uint32))))
        return mean, se, samples

    def progressive_status(self):
        out = (C.c_int64 * 6)()
        self._check(self._lib.ft_progressive_status(self._ctx, out))
        keys = ["passes", "min_samples", "max_samples", "blocks", "blocks_retired", "samples_traced"]
        return dict(zip(keys, list(out)))

    def progressive_end(self):
        self._check(self._lib.ft_progressive_end(self._ctx))
        self._progressive = None

    def progressive(self, camera, res_h, res_v, pieces, seeds, tolerance=0.0, min_samples=2, max_depth=MAX_DEPTH, tiles=None, rgba8=False):
        """Begin, then one pass per piece of a jitter pattern (pieces: arrays of n x 2 offsets; seeds: one per pass), yielding
        (frame, stats) after each; the accumulation stays open afterwards for progressive_fetch / progressive_status."""
        self.progressive_begin(camera, res_h, res_v, max_depth=max_depth, tiles=tiles, tolerance=tolerance, min_samples=min_samples)
        for piece, seed in zip(pieces, seeds):
            piece = _capi.as_f64(piece).reshape(-1, 2)
            yield self.progressive_pass(piece.shape[0], piece, seed=seed, rgba8=rgba8)

    def _progressive_shape(self):
        shape = getattr(self, "_progressive", None)
        if shape is None:                                           # the frame's size is unknown: nothing to size the output by
            raise FtError(-5, "no progressive accumulation (progressive_begin)")
        return shape

    def render_aov(self, camera, res_h, res_v, spp, jitter, sample=0, seed=DEFAULT_SEED, tiles=None, channels=None, out=None):
        """Per-pixel surface buffers (ft_render_aov): the hit of sample `sample`'s geometry ray of the frame
        render(camera, res_h, res_v, spp, jitter, seed=seed, tiles=tiles) would trace, per tile pixel.  Returns a dict of the requested
        planes ('t', 'p', 'n', 'colour', 'material', 'leaf', 'node', 'triangle'; None = all), each [res_v, res_h] or [res_v, res_h, 3],
        plus 'stats'.  Planes are created holding the miss values; `out` may hand over planes of its own (pixels outside the tiles keep
        what they hold)."""
        want = [c[0] for c in _capi.AOV_CHANNELS] if channels is None else list(channels)
        unknown = set(want) - {c[0] for c in _capi.AOV_CHANNELS}
        if unknown:
            raise ValueError(f"unknown AOV channels {sorted(unknown)}")
        jitter = np.zeros((1, 2)) if spp == 0 else _capi.as_f64(jitter, (spp, 2))
        planes, aov = {}, _capi.ft_aov()
        for name, dtype, width, miss in _capi.AOV_CHANNELS:
            if name not in want:
                continue
            shape = (res_v, res_h) if width == 1 else (res_v, res_h, width)
            a = out[name] if out is not None and name in out else np.full(shape, miss, dtype=dtype)
            if a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError(f"AOV plane {name}: need a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
            planes[name] = a
            setattr(aov, name, a.ctypes.data_as(_capi.c_double_p if dtype == np.float64 else _capi.c_int32_p))
        rects, n_rects = _capi.make_rects(tiles)
        st = _capi.ft_stats()
        self._check(self._lib.ft_render_aov(self._ctx, C.byref(camera), res_h, res_v, spp, _capi.dptr(jitter), int(sample), int(seed),
                                            rects, n_rects, C.byref(aov), C.byref(st)))
        planes["stats"] = st.as_dict()
        return planes

    def denoise(self, camera, res_h, res_v, spp, jitter, sample=0, seed=DEFAULT_SEED, tiles=None, rgba8=False, out=None, **params):
        """ft_denoise: the FP64 frame in HBM (the last render / progressive_pass of res_h x res_v) filtered on the device by an
        edge-avoiding a-trous filter guided by render_aov's n, p and colour of the same (camera, spp, jitter, sample, seed, tiles).
        params: iterations, sigma_colour, sigma_normal, sigma_position, demodulate, albedo_floor, use_variance, variance_floor
        (_capi.DENOISE_DEFAULTS).  Returns (rgb[res_v, res_h, 3] float64 or rgba[res_v, res_h, 4] uint8, stats dict); pixels outside
        the tiles keep what `out` held (0 in a fresh array).  The frame in HBM stays as it was."""
        unknown = set(params) - set(_capi.DENOISE_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown denoise parameters {sorted(unknown)}")
        p = _capi.ft_denoise_params()
        for k, v in {**_capi.DENOISE_DEFAULTS, **params}.items():
            setattr(p, k, int(v) if k in ("iterations", "demodulate", "use_variance") else float(v))
        jitter = np.zeros((1, 2)) if spp == 0 else _capi.as_f64(jitter, (spp, 2))
        shape, dtype = ((res_v, res_h, 4), np.uint8) if rgba8 else ((res_v, res_h, 3), np.float64)
        if out is None:
            out = np.zeros(shape, dtype=dtype)
        if out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError(f"denoise: need a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        rects, n_rects = _capi.make_rects(tiles)
        st = _capi.ft_stats()
        self._check(self._lib.ft_denoise(self._ctx, C.byref(camera), res_h, res_v, spp, _capi.dptr(jitter), int(sample), int(seed), rects, n_rects,
                                         C.byref(p), 1 if rgba8 else 0, out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, st.as_dict()

    # reprojected frame accumulation for a moving camera (ft_temporal_*, include/functracer_hip.h) -----
    def temporal_begin(self, res_h, res_v, tiles=None):
        """Start accumulating the frames of a camera path (replaces any earlier accumulation); fixes the frame size and the tiles."""
        rects, n_rects = _capi.make_rects(tiles)
        self._check(self._lib.ft_temporal_begin(self._ctx, int(res_h), int(res_v), rects, n_rects))
        self._temporal = (int(res_h), int(res_v))

    def temporal_accumulate(self, camera, spp, jitter, sample=0, seed=DEFAULT_SEED, rgba8=False, out=None, fetch=True, **params):
        """ft_temporal_accumulate: the FP64 frame in HBM (the last render of the begin's size, from `camera`) blended with the history
        of the surfaces render_aov reports for (camera, spp, jitter, sample, seed), looked up where they lay in the previous call's
        image.  params: max_history, to_frame, min_normal_dot, position_tolerance_px (_capi.TEMPORAL_DEFAULTS).  Returns (the
        accumulated rgb[res_v, res_h, 3] float64 or rgba[res_v, res_h, 4] uint8, stats dict); pixels outside the tiles keep what
        `out` held (0 in a fresh array); with fetch=False nothing is copied out (returns (None, stats)).  After a commit_moved the history
        follows the moved leaves; after a commit_deformed under set_option("temporal_follow_deformed", 1) it follows the triangles."""
        unknown = set(params) - set(_capi.TEMPORAL_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown temporal parameters {sorted(unknown)}")
        res_h, res_v = self._temporal_shape()
        p = _capi.ft_temporal_params()
        for k, v in {**_capi.TEMPORAL_DEFAULTS, **params}.items():
            setattr(p, k, int(v) if k in ("max_history", "to_frame") else float(v))
        jitter = np.zeros((1, 2)) if spp <= 0 else _capi.as_f64(jitter, (spp, 2))
        shape, dtype = ((res_v, res_h, 4), np.uint8) if rgba8 else ((res_v, res_h, 3), np.float64)
        if fetch and out is None:
            out = np.zeros(shape, dtype=dtype)
        if fetch and (out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous):
            raise ValueError(f"temporal_accumulate: need a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        st = _capi.ft_stats()
        self._check(self._lib.ft_temporal_accumulate(self._ctx, C.byref(camera), int(spp), _capi.dptr(jitter), int(sample), int(seed), C.byref(p),
                                                     1 if rgba8 else 0, out.ctypes.data_as(C.c_void_p) if fetch else None, C.byref(st)))
        return (out if fetch else None), st.as_dict()

    def temporal_filter(self, camera=None, spp=1, jitter=None, sample=0, seed=DEFAULT_SEED, rgba8=False, out=None, variance=False, **params):
        """ft_temporal_filter: the history the last temporal_accumulate wrote, filtered on the device by an edge-avoiding a-trous filter
        whose colour term is scaled by a per-pixel variance (the history's standard error; a 7x7 spatial estimate where the history is
        shorter than min_history) that is filtered from iteration to iteration.  With demodulate, (camera, spp, jitter, sample, seed) are
        those of that temporal_accumulate; without, they are not read.  params: iterations, demodulate, min_history, to_frame,
        sigma_colour, sigma_normal, sigma_position, albedo_floor, variance_floor (_capi.TEMPORAL_FILTER_DEFAULTS).  variance: False, True
        (a fresh plane) or a float64 array [res_v, res_h] to fill; out=False copies no colour out.  Returns (rgb[res_v, res_h, 3] float64
        or rgba[res_v, res_h, 4] uint8 or None, variance[res_v, res_h] or None, stats dict); pixels outside the tiles keep what the
        arrays held (0 in fresh ones)."""
        unknown = set(params) - set(_capi.TEMPORAL_FILTER_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown temporal filter parameters {sorted(unknown)}")
        res_h, res_v = self._temporal_shape()
        p = _capi.ft_temporal_filter_params()
        for k, v in {**_capi.TEMPORAL_FILTER_DEFAULTS, **params}.items():
            setattr(p, k, int(v) if k in ("iterations", "demodulate", "min_history", "to_frame") else float(v))
        if jitter is not None:
            jitter = np.zeros((1, 2)) if spp <= 0 else _capi.as_f64(jitter, (spp, 2))
        shape, dtype = ((res_v, res_h, 4), np.uint8) if rgba8 else ((res_v, res_h, 3), np.float64)
        if out is None:
            out = np.zeros(shape, dtype=dtype)
        elif out is False:
            out = None
        if out is not None and (out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous):
            raise ValueError(f"temporal_filter: need a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        var = np.zeros((res_v, res_h)) if variance is True else None if variance is False or variance is None else variance
        if var is not None and (var.shape != (res_v, res_h) or var.dtype != np.float64 or not var.flags.c_contiguous):
            raise ValueError(f"temporal_filter: the variance needs a C-contiguous float64 array of shape {(res_v, res_h)}")
        st = _capi.ft_stats()
        self._check(self._lib.ft_temporal_filter(self._ctx, C.byref(camera) if camera is not None else None, int(spp),
                                                 _capi.dptr(jitter) if jitter is not None else None, int(sample), int(seed), C.byref(p), 1 if rgba8 else 0,
                                                 out.ctypes.data_as(C.c_void_p) if out is not None else None, _capi.dptr(var) if var is not None else None, C.byref(st)))
        return out, var, st.as_dict()

    def temporal_enqueue(self, camera, spp, jitter, sample=0, seed=DEFAULT_SEED, rgba8=False, out=None, filter=None, **params):
        """ft_temporal_enqueue: temporal_accumulate and, with `filter` (a dict of temporal_filter's parameters; {} for the defaults), the
        temporal_filter of its result, queued behind the last frame queued or rendered; returns at once.  out: a C-contiguous array of
        the result's shape (rgb[res_v, res_h, 3] float64 or rgba[res_v, res_h, 4] uint8) that outlives the call, best a PinnedArray's,
        one per call in flight; it is the host's again after temporal_wait(), or once _capi.TEMPORAL_QUEUE_DEPTH more calls were queued.
        None (without a filter only): nothing leaves the device.  params: temporal_accumulate's; to_frame is refused, here and in `filter`."""
        unknown = set(params) - set(_capi.TEMPORAL_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown temporal parameters {sorted(unknown)}")
        res_h, res_v = self._temporal_shape()
        p = _capi.ft_temporal_params()
        for k, v in {**_capi.TEMPORAL_DEFAULTS, **params}.items():
            setattr(p, k, int(v) if k in ("max_history", "to_frame") else float(v))
        fp = None
        if filter is not None:
            unknown = set(filter) - set(_capi.TEMPORAL_FILTER_DEFAULTS)
            if unknown:
                raise ValueError(f"unknown temporal filter parameters {sorted(unknown)}")
            fp = _capi.ft_temporal_filter_params()
            for k, v in {**_capi.TEMPORAL_FILTER_DEFAULTS, **filter}.items():
                setattr(fp, k, int(v) if k in ("iterations", "demodulate", "min_history", "to_frame") else float(v))
        jitter = np.zeros((1, 2)) if spp <= 0 else _capi.as_f64(jitter, (spp, 2))
        shape, dtype = ((res_v, res_h, 4), np.uint8) if rgba8 else ((res_v, res_h, 3), np.float64)
        if out is not None and (out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous):
            raise ValueError(f"temporal_enqueue: need a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        self._check(self._lib.ft_temporal_enqueue(self._ctx, C.byref(camera), int(spp), _capi.dptr(jitter), int(sample), int(seed), C.byref(p),
                                                  C.byref(fp) if fp is not None else None, 1 if rgba8 else 0,
                                                  out.ctypes.data_as(C.c_void_p) if out is not None else None))

    def temporal_wait(self):
        """ft_temporal_wait: blocks until every queued temporal call has finished, raises the first error among them and returns the
        stats dict of the last one (all zero with nothing queued)."""
        st = _capi.ft_stats()
        self._check(self._lib.ft_temporal_wait(self._ctx, C.byref(st)))
        return st.as_dict()

    def temporal_fetch(self):
        """(mean[res_v, res_h, 3], stderr[res_v, res_h, 3], history length[res_v, res_h] float64) of the tile pixels; other pixels stay 0."""
        res_h, res_v = self._temporal_shape()
        mean, se, length = np.zeros((res_v, res_h, 3)), np.zeros((res_v, res_h, 3)), np.zeros((res_v, res_h))
        self._check(self._lib.ft_temporal_fetch(self._ctx, _capi.dptr(mean), _capi.dptr(se), _capi.dptr(length)))
        return mean, se, length

    def temporal_status(self):
        out = (C.c_int64 * 4)()
        self._check(self._lib.ft_temporal_status(self._ctx, out))
        return dict(zip(["calls", "pixels", "with_history", "at_max_history"], list(out)))

    def temporal_set_clamp(self, params=(), off=False, **kw):
        """ft_temporal_set_clamp: the neighbourhood clamp of the history for every later temporal_accumulate of the open accumulation -
        the fetched mean is moved into mu +- (gamma * sd + floor) of the current frame's (2 radius + 1)^2 neighbourhood and a pixel it
        moved keeps at most clamped_history of its length.  Keywords: radius, clamped_history, gamma, floor
        (_capi.TEMPORAL_CLAMP_DEFAULTS).  temporal_set_clamp(None) or off=True switches it off, as temporal_begin does."""
        if params is None or off:
            if kw:
                raise ValueError("temporal_set_clamp: parameters given together with off")
            self._check(self._lib.ft_temporal_set_clamp(self._ctx, None))
            return
        kw = {**dict(params), **kw}
        unknown = set(kw) - set(_capi.TEMPORAL_CLAMP_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown temporal clamp parameters {sorted(unknown)}")
        p = _capi.ft_temporal_clamp_params()
        for k, v in {**_capi.TEMPORAL_CLAMP_DEFAULTS, **kw}.items():
            setattr(p, k, int(v) if k in ("radius", "clamped_history") else float(v))
        self._check(self._lib.ft_temporal_set_clamp(self._ctx, C.byref(p)))

    def temporal_clamp_status(self):
        """ft_temporal_clamp_status: {"radius": the radius in force (0 = off), "clamped": pixels the clamp moved in the last accumulate}."""
        out = (C.c_int64 * 2)()
        self._check(self._lib.ft_temporal_clamp_status(self._ctx, out))
        return dict(zip(["radius", "clamped"], list(out)))

    def temporal_end(self):
        self._check(self._lib.ft_temporal_end(self._ctx))
        self._temporal = None

    def _temporal_shape(self):
        shape = getattr(self, "_temporal", None)
        if shape is None:                                           # the frame's size is unknown: nothing to size the output by
            raise FtError(-5, "no temporal accumulation (temporal_begin)")
        return shape

    # moving rigid objects under a temporal accumulation (include/functracer_hip.h) ---------------------
    def set_transform(self, node, ops):
        """ft_sg_set_transform: replace the transform list of the node `transform(ops, child)` returned (ops as there); the child stays."""
        self._check(self._lib.ft_sg_set_transform(self._ctx, int(node), _capi.transform_array(ops) if len(ops) else None, len(ops)))

    def commit_moved(self):
        """ft_scene_commit_moved: commit a graph whose transforms alone changed since the last commit.  A temporal accumulation stays open
        and its history follows the moved leaves; a progressive accumulation ends.  Under set_option("moved_in_place", 1) a device context
        uploads the new poses over the old ones and refits the light-space shadow structures of the leaves that turned, instead of
        committing the whole scene again, whenever nothing but poses changed; every later call gives the same bits either way
        (moved_commits tells which way a call went)."""
        self._check(self._lib.ft_scene_commit_moved(self._ctx))
        self._progressive = None

    def moved_commits(self):
        """ft_debug_moved_commits: a dict of `in_place` and `full` (commit_moved calls done in place / by the full commit since the context
        was created), `full_reason` (of the last call: 0 it was done in place, 1 option "moved_in_place" off or a host-only context, 2 a
        light setter, new mesh vertices or a commit-time option pending, 3 the re-flatten differs in more than poses) and `pairs_refit`
        (light-space pairs the last in-place call refit or retreed)."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.ft_debug_moved_commits(self._ctx, out))
        return dict(zip(_capi.MOVED_COMMITS_FIELDS, (int(v) for v in out)))

    # deforming meshes: a refit instead of a rebuild (include/functracer_hip.h) ------------------------
    def set_mesh_triangles(self, node, tris):
        """ft_sg_set_mesh_triangles: replace the vertices of the node `bsp_mesh(depth, tris)` returned (tris as there, the same count)."""
        t = _capi.as_f64(tris).reshape(-1, 9)
        self._check(self._lib.ft_sg_set_mesh_triangles(self._ctx, int(node), _capi.dptr(t), t.shape[0]))

    def commit_deformed(self):
        """ft_scene_commit_deformed: commit a graph whose mesh vertices alone changed since the last commit by refitting the trees on the
        device.  A temporal accumulation stays open; a progressive accumulation ends.  Under set_option("temporal_follow_deformed", 1) the
        edited meshes' records are kept as the accumulation last saw them (72 bytes per triangle, until the next temporal_accumulate)."""
        self._check(self._lib.ft_scene_commit_deformed(self._ctx))
        self._progressive = None

    # morph targets: vertices blended on the device before the refit (include/functracer_hip.h) --------
    def set_mesh_targets(self, node, targets):
        """ft_sg_set_mesh_targets: the key shapes of the `bsp_mesh` node, [K, n, 9] absolute positions (K = 0 .. 16; an empty array removes
        them).  The node's vertices as they stand become the base; the library keeps the targets as deltas from it."""
        t = _capi.as_f64(targets)
        if t.ndim == 4:                                             # [K, n, 3, 3]
            t = t.reshape(t.shape[0], t.shape[1], -1)
        if t.ndim != 3 or t.shape[2] != 9:
            raise ValueError("set_mesh_targets: targets are [K, n, 9]")
        self._check(self._lib.ft_sg_set_mesh_targets(self._ctx, int(node), _capi.dptr(t) if t.shape[0] else None, t.shape[0], t.shape[1]))

    def set_mesh_weights(self, node, w):
        """ft_sg_set_mesh_weights: the node's vertices are morph_blend(base, targets, w) from the next commit on; commit_deformed makes
        them on the device (option "morph_on_device", default 1)."""
        w = _capi.as_f64(w).reshape(-1)
        self._check(self._lib.ft_sg_set_mesh_weights(self._ctx, int(node), _capi.dptr(w) if w.size else None, w.shape[0]))

    def morph(self, node):
        """ft_debug_morph: a dict of `device_commits` (commit_deformed calls since the context was created that blended a mesh on the
        device), `device_meshes` / `host_meshes` (meshes the last commit_deformed blended on the device / on the host), `resident_bytes`
        (base and deltas of `node` per device), `scan` (8 doubles: the bounds lo, hi and the extent that call used for `node`) and
        `from_device` (whether they were reduced on the device)."""
        counts = (C.c_int64 * 4)()
        scan = np.zeros(8)
        self._check(self._lib.ft_debug_morph(self._ctx, int(node), counts, _capi.dptr(scan)))
        out = dict(zip(_capi.MORPH_FIELDS, (int(v) for v in counts)))
        out["scan"], out["from_device"] = scan, bool(scan[7] == 1.0)
        return out

    # skinning: vertices posed from a bone palette on the device before the refit (include/functracer_hip.h) --------
    def set_mesh_skin(self, node, index, weight):
        """ft_sg_set_mesh_skin: bone indices and weights of the `bsp_mesh` node's corners, [n, 3, J] each (J = 1 .. 4), corner-major.  It
        removes any palette; J = 0 (arrays of shape [n, 3, 0]) removes the skin as well."""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        w = _capi.as_f64(weight)
        if idx.ndim != 3 or idx.shape[1] != 3 or w.shape != idx.shape:
            raise ValueError("set_mesh_skin: index and weight are [n, 3, J]")
        j = idx.shape[2]
        self._check(self._lib.ft_sg_set_mesh_skin(self._ctx, int(node), idx.ctypes.data_as(C.POINTER(C.c_int32)) if j else None, _capi.dptr(w) if j else None, j, idx.shape[0]))

    def set_mesh_bones(self, node, matrices):
        """ft_sg_set_mesh_bones: the node's vertices are skin_blend(shape, index, weight, matrices) from the next commit on, matrices
        [n_bones, 12] or [n_bones, 3, 4] (an empty array removes the palette); commit_deformed makes them on the device (option
        "skin_on_device", default 1)."""
        m = _capi.as_f64(matrices).reshape(-1, 12)
        self._check(self._lib.ft_sg_set_mesh_bones(self._ctx, int(node), _capi.dptr(m) if m.shape[0] else None, m.shape[0]))

    def skin(self, node):
        """ft_debug_skin: a dict of `device_commits` (commit_deformed calls since the context was created that skinned a mesh on the device),
        `device_meshes` / `host_meshes` (meshes the last commit_deformed skinned on the device / on the host) and `resident_bytes` (rest
        shape, indices, weights and palette of `node` per device)."""
        counts = (C.c_int64 * 4)()
        self._check(self._lib.ft_debug_skin(self._ctx, int(node), counts))
        return dict(zip(_capi.MORPH_FIELDS, (int(v) for v in counts)))

    def set_mesh_bones_dq(self, node, dq):
        """ft_sg_set_mesh_bones_dq: the node's vertices are skin_blend_dq(shape, index, weight, dq) from the next commit on, dq [n_bones, 8]
        (real part w, x, y, z, then the dual part; an empty array removes whichever palette is in force); it replaces a matrix palette,
        and commit_deformed makes the vertices on the device as for set_mesh_bones (option "skin_on_device", default 1)."""
        d = _capi.as_f64(dq).reshape(-1, 8)
        self._check(self._lib.ft_sg_set_mesh_bones_dq(self._ctx, int(node), _capi.dptr(d) if d.shape[0] else None, d.shape[0]))

    def skin_dq(self, node):
        """ft_debug_skin_dq: a dict of `device_commits` (commit_deformed calls since the context was created that posed a mesh with k_skin_dq
        on the device), `device_meshes` / `host_meshes` (meshes whose dual-quaternion skin the last commit_deformed made on the device / on
        the host) and `palette_kind` (0 none, 1 matrices, 2 dual quaternions in force for `node`)."""
        counts = (C.c_int64 * 4)()
        self._check(self._lib.ft_debug_skin_dq(self._ctx, int(node), counts))
        return dict(zip(_capi.SKIN_DQ_FIELDS, (int(v) for v in counts)))

    # moving lights (include/functracer_hip.h) ---------------------------------------------------------
    def set_directional(self, light, direction, colour):
        """ft_scene_set_directional: new direction and colour for light `light` (the index in add_* order), a directional light."""
        self._check(self._lib.ft_scene_set_directional(self._ctx, int(light), _capi.vec3(direction), _capi.vec3(colour)))

    def set_soft_directional(self, light, direction, scatter_rad, colour):
        """ft_scene_set_soft_directional: new direction, scatter angle and colour for a soft directional light; its sample count stays."""
        self._check(self._lib.ft_scene_set_soft_directional(self._ctx, int(light), _capi.vec3(direction), float(scatter_rad), _capi.vec3(colour)))

    def set_positional(self, light, position, falloff, colour):
        """ft_scene_set_positional: new position, falloff and colour for a point light."""
        self._check(self._lib.ft_scene_set_positional(self._ctx, int(light), _capi.vec3(position), _capi.vec3(falloff), _capi.vec3(colour)))

    def commit_lights(self):
        """ft_scene_commit_lights: commit a graph whose light values alone changed since the last commit: the lights are uploaded again and
        the light-space shadow trees of the directions that changed are refit on the device.  A temporal accumulation stays open; a
        progressive accumulation ends."""
        self._check(self._lib.ft_scene_commit_lights(self._ctx))
        self._progressive = None

    # queued pose and light commits (include/functracer_hip.h) ------------------------------------------
    def commit_moved_enqueue(self):
        """ft_scene_commit_moved_enqueue: commit_moved as under "moved_in_place" 1, but nothing queued is retired and no stream is drained:
        frames and temporal calls queued before the call show the old poses, everything queued or run after it the new ones.  Takes the
        blocking path, with its bits, when it cannot queue (pose_queue tells why)."""
        self._check(self._lib.ft_scene_commit_moved_enqueue(self._ctx))
        self._progressive = None

    def commit_lights_enqueue(self):
        """ft_scene_commit_lights_enqueue: commit_lights without retiring what is queued, unless a directional light over a mesh with
        light-space shadow structures turns (pose_queue tells)."""
        self._check(self._lib.ft_scene_commit_lights_enqueue(self._ctx))
        self._progressive = None

    def pose_queue(self):
        """ft_debug_pose_queue: a dict of `moved_queued`, `moved_blocking`, `moved_reason` (of the last commit_moved_enqueue: 0 queued, 1 host-only
        context, 2 a light setter, new vertices or a commit-time option pending, 3 the re-flatten differs in more than poses, 4 a
        light-space pair's frame changed), the same three for commit_lights_enqueue, `sets` (pose sets on the first device) and `pending`
        (frames + temporal calls the host still had pending on the first device when the last of the two calls returned)."""
        out = (C.c_int64 * 8)()
        self._check(self._lib.ft_debug_pose_queue(self._ctx, out))
        return dict(zip(_capi.POSE_QUEUE_FIELDS, (int(v) for v in out)))

    # queued deform commits (include/functracer_hip.h) --------------------------------------------------
    def commit_deformed_enqueue(self):
        """ft_scene_commit_deformed_enqueue: commit_deformed, but nothing queued is retired and no stream a frame runs on is waited for: the
        refit goes into a copy of the mesh trees that no frame in flight reads.  Frames and temporal calls queued before the call show the
        old vertices, everything queued or run after it the new ones, bit for bit a fresh context's.  Every kind of edit can be queued -
        set_mesh_triangles, weights, matrix or dual-quaternion palettes, their host twins.  Takes the blocking path, with its bits and
        its draining, when it cannot queue (deform_queue tells why)."""
        self._check(self._lib.ft_scene_commit_deformed_enqueue(self._ctx))
        self._progressive = None

    def deform_queue(self):
        """ft_debug_deform_queue: a dict of `queued`, `blocking`, `reason` (of the last commit_deformed_enqueue: 0 queued, 1 host-only
        context, 2 several devices, 3 the first refit since a full commit, 4 "refit_rebuild_percent" above 0, 5 "deform_light_space" gives
        an edited mesh a light-space job, 6 "temporal_follow_deformed" with an accumulation that has accumulated), `sets` (geometry sets on
        the first device), `pending` (frames + temporal calls the host still had pending there when the last call returned),
        `retired_for_set` (frames or temporal calls retired because every set was held) and `carried` (mesh ranges copied between sets
        by the last call)."""
        out = (C.c_int64 * 8)()
        self._check(self._lib.ft_debug_deform_queue(self._ctx, out))
        return dict(zip(_capi.DEFORM_QUEUE_FIELDS, (int(v) for v in out)))

    def tree_quality(self, node):
        """ft_scene_tree_quality: the measured surface-area cost of the tree of the `bsp_mesh(0, tris)` node as it lies in device memory.
        A dict of `cost` (now), `cost_built` (when the tree was last built), `ratio` (cost / cost_built; 1.0 when cost_built is 0),
        `rebuildable` (the tree was built on the device: "refit_rebuild_percent" can rebuild it in place) and `rebuilds` (in place, since the
        last full commit)."""
        out = np.zeros(4)
        self._check(self._lib.ft_scene_tree_quality(self._ctx, int(node), _capi.dptr(out)))
        cost, built = float(out[0]), float(out[1])
        return {"cost": cost, "cost_built": built, "ratio": cost / built if built > 0.0 else 1.0, "rebuildable": int(out[2]), "rebuilds": int(out[3])}

    def leaf_matrices(self):
        """ft_debug_leaf_matrices: (m2w[leaves, 3, 4], w2m[leaves, 3, 4]) of the scene the context holds."""
        n = C.c_int64()
        self._check(self._lib.ft_debug_leaf_matrices(self._ctx, C.byref(n), None, None))
        m2w, w2m = np.zeros((n.value, 3, 4)), np.zeros((n.value, 3, 4))
        self._check(self._lib.ft_debug_leaf_matrices(self._ctx, C.byref(n), _capi.dptr(m2w), _capi.dptr(w2m)))
        return m2w, w2m

    def pick(self, camera, res_h, res_v, x, y, spp=1, jitter=None, sample=0, seed=DEFAULT_SEED):
        """What is at pixel (x, y) (row 0 = top): the record of render_aov for that one pixel (a 1x1 tile) as a dict of plain
        values, or None when the ray misses everything.  The device counterpart of printIntersectionAt (Program.fs:33-49)."""
        jitter = np.zeros((1, 2)) if jitter is None else jitter
        out = {name: np.full((res_v, res_h) if w == 1 else (res_v, res_h, w), miss, dtype=dt) for name, dt, w, miss in _capi.AOV_CHANNELS}
        self.render_aov(camera, res_h, res_v, spp, jitter, sample=sample, seed=seed, tiles=[(x, y, 1, 1)], out=out)
        if out["leaf"][y, x] < 0:
            return None
        rec = {}
        for name, dt, w, _ in _capi.AOV_CHANNELS:
            v = out[name][y, x]
            rec[name] = tuple(float(c) for c in v) if w == 3 else (float(v) if dt == np.float64 else int(v))
        return rec

    def closest(self, origins, dirs):
        """Scene.intersectScene (Scene.fs:118) for explicit rays, through the device path."""
        o = _capi.as_f64(origins).reshape(-1, 3)
        d = _capi.as_f64(dirs).reshape(-1, 3)
        n = o.shape[0]
        hit = np.zeros(n, dtype=np.int32)
        t, p, nr, col = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        self._check(self._lib.ft_debug_closest(self._ctx, _capi.dptr(o), _capi.dptr(d), n, hit.ctypes.data_as(_capi.c_int32_p),
                                               _capi.dptr(t), _capi.dptr(p), _capi.dptr(nr), _capi.dptr(col)))
        return hit, t, p, nr, col

    def blocked(self, origins, dirs, max_dist):
        """Scene.lightIsBocked (Scene.fs:119-121) for explicit rays, through the device path."""
        o = _capi.as_f64(origins).reshape(-1, 3)
        d = _capi.as_f64(dirs).reshape(-1, 3)
        m = _capi.as_f64(max_dist).reshape(-1)
        out = np.zeros(o.shape[0], dtype=np.int32)
        self._check(self._lib.ft_debug_blocked(self._ctx, _capi.dptr(o), _capi.dptr(d), _capi.dptr(m), o.shape[0], out.ctypes.data_as(_capi.c_int32_p)))
        return out

    def colour_for_ray(self, origins, dirs, max_depth=MAX_DEPTH):
        """Shading.getColourForRay (Shading.fs:131-139) for explicit rays, through the device path."""
        o = _capi.as_f64(origins).reshape(-1, 3)
        d = _capi.as_f64(dirs).reshape(-1, 3)
        rgb = np.zeros((o.shape[0], 3))
        self._check(self._lib.ft_debug_colour(self._ctx, _capi.dptr(o), _capi.dptr(d), o.shape[0], max_depth, _capi.dptr(rgb)))
        return rgb

    def devices(self):
        """The device ordinals behind this context (several for a multi-device context)."""
        out = (C.c_int32 * 64)()
        n = self._check(self._lib.ft_debug_devices(self._ctx, out, 64))
        return list(out[:n])

    def commit_times(self):
        """ft_get_commit_times of the last commit: host flatten, device BVH builds, uploads (ms) and the tallest device-built tree."""
        ms = np.zeros(4)
        self._check(self._lib.ft_get_commit_times(self._ctx, _capi.dptr(ms)))
        return {"flatten_ms": float(ms[0]), "device_bvh_ms": float(ms[1]), "upload_ms": float(ms[2]), "device_bvh_height": int(ms[3])}

    def mesh_trees(self):
        """ft_debug_mesh_trees: the mesh trees of the committed scene as the kernels walk them, read back from device memory (from the
        flattened scene in a host-only context).  A dict of `nodes` (records of _capi.BSP_NODE_DTYPE), `bsp_leaves` [n, 2] (first_tri,
        n_tris), `tris` [n, 9], `tri_orig`, `tri_src`, `wide` [n, 28] float64, `coarse_boxes` [n, 6] float32, `meshes` [n, 6] int32 (root,
        bvh_root, n_source_tris, wide root, first coarse box, coarse box count), `jobs` (a list of dicts, _capi.BVH_JOB_FIELDS),
        `stack_capacity` and `from_device`."""
        sizes = (C.c_int64 * 12)()
        self._check(self._lib.ft_debug_mesh_trees(self._ctx, sizes, *([None] * 9)))
        n = list(sizes)
        out = {"nodes": np.zeros(n[0], dtype=_capi.BSP_NODE_DTYPE), "bsp_leaves": np.zeros((n[1], 2), dtype=np.uint32), "tris": np.zeros((n[2], 9)),
               "tri_orig": np.zeros(n[3], dtype=np.uint32), "tri_src": np.zeros(n[4], dtype=np.uint32), "wide": np.zeros((n[5], 28)),
               "coarse_boxes": np.zeros((n[6], 6), dtype=np.float32), "meshes": np.zeros((n[7], 6), dtype=np.int32)}
        jobs = np.zeros((n[8], 9), dtype=np.uint32)
        order = ["nodes", "bsp_leaves", "tris", "tri_orig", "tri_src", "wide", "coarse_boxes", "meshes"]
        self._check(self._lib.ft_debug_mesh_trees(self._ctx, sizes, *[out[k].ctypes.data for k in order], jobs.ctypes.data))
        out["jobs"] = [dict(zip(_capi.BVH_JOB_FIELDS, (int(v) for v in row))) for row in jobs]
        out["stack_capacity"], out["from_device"] = int(sizes[9]), bool(sizes[10])
        return out

    def block_lists(self):
        """ft_debug_block_lists: the per-block triangle candidate lists of the last frame queued (option "primary_block_lists"), read
        back from device memory.  A dict of `leaf` (the mesh leaf the lists are for; -1: that frame was not classified or carried none, the arrays are then
        empty), `heads` (one word per active block: _capi.LIST_NONE = the block walks the tree, else first entry << 7 | count),
        `pos_block` (the block of the frame's pixel list behind each active block), `entries` (records of _capi.LIST_ENTRY_DTYPE: the
        triangle's record and list index and its rectangle on the image plane, in the (jx, jy) of the primary rays), `plane` (tlx, tly,
        pw, ph: pixel (x, y) under jitter offset (ox, oy) looks through jx = tlx + (x + ox) pw, jy = tly - (y - oy) ph) and `capacity`."""
        sizes = (C.c_int64 * 4)()
        plane = np.zeros(4)
        fn = self._lib.ft_debug_block_lists
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(fn(self._ctx, sizes, None, None, None, None))
        heads, pos_block = np.zeros(sizes[0], dtype=np.uint32), np.zeros(sizes[0], dtype=np.uint32)
        entries = np.zeros(sizes[1], dtype=_capi.LIST_ENTRY_DTYPE)
        self._check(fn(self._ctx, sizes, plane.ctypes.data, heads.ctypes.data, pos_block.ctypes.data, entries.ctypes.data))
        return {"leaf": int(sizes[2]), "heads": heads, "pos_block": pos_block, "entries": entries, "plane": plane, "capacity": int(sizes[3])}

    def edge_records(self):
        """ft_debug_edge_records: the edge records of option "edge_cull" as they lie in device memory - a dict of `grid` (n x 3 x 3 floats,
        one record per triangle record ft_debug_light_space hands out, under the same index; empty where the scene carries none) and `lists`
        (one per entry of block_lists()["entries"]).  A record is three lines (a, b, c), a x + b y + c <= 0 inside; zeros: no edges."""
        sizes = (C.c_int64 * 2)()
        fn = self._lib.ft_debug_edge_records
        fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
        self._check(fn(self._ctx, sizes, None, None))
        grid = np.zeros((sizes[0],) + _capi.EDGE_RECORD_SHAPE, dtype=np.float32)
        lists = np.zeros((sizes[1],) + _capi.EDGE_RECORD_SHAPE, dtype=np.float32)
        self._check(fn(self._ctx, sizes, grid.ctypes.data, lists.ctypes.data))
        return {"grid": grid[:sizes[0]], "lists": lists[:sizes[1]]}

    def ls_retree(self):
        """ft_debug_ls_retree: the pairs ft_scene_commit_lights / ft_scene_commit_deformed keep track of since the last full commit (option
        "light_space_retree") - a list of dicts, one per pair: `rec` (its pair record), `leaf`, `light`, `n_tris`, `ls_first` (the first of
        its tree's leaf records, -1: none), `R`, `retreed`, `block` (the first node of its block, -1: none) and `block_nodes` (N)."""
        fn = self._lib.ft_debug_ls_retree
        fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
        n = C.c_int64()
        self._check(fn(self._ctx, C.byref(n), None, None))
        rows, R = np.zeros((n.value, 8), dtype=np.int64), np.zeros(n.value)
        self._check(fn(self._ctx, C.byref(n), rows.ctypes.data, R.ctypes.data))
        out = []
        for row, r in zip(rows[:n.value], R):
            d = dict(zip(_capi.LS_RETREE_FIELDS, (int(v) for v in row)))
            d["retreed"], d["R"] = bool(d["retreed"]), float(r)
            out.append(d)
        return out

    def classify_reuse(self):
        """ft_debug_classify_reuse: what the frames queued since the context was created did with their classifications (option
        "classify_reuse"), summed over its devices - a dict of `classified` (k_classify launched), `reused` (a slot's kept classification
        read as it was), `windows_launched` and `windows_skipped` (windows past the end of a kept active list)."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.ft_debug_classify_reuse(self._ctx, out))
        return dict(zip(_capi.CLASSIFY_REUSE_FIELDS, (int(v) for v in out)))

    def primary_kernels(self):
        """ft_debug_primary_kernels: the bounce-0 launches since the context was created, summed over its devices - a dict of `k_primary`
        and `k_primary_mesh` (option "primary_mesh_kernel")."""
        out = (C.c_int64 * 2)()
        self._check(self._lib.ft_debug_primary_kernels(self._ctx, out))
        return {"k_primary": int(out[0]), "k_primary_mesh": int(out[1])}

    def scene_info(self):
        out = (C.c_int64 * 12)()
        self._check(self._lib.ft_debug_scene_info(self._ctx, out))
        keys = ["leaves", "program_words", "meshes", "bsp_nodes", "bsp_leaves", "triangles", "csg_capacity", "stack_capacity", "items", "bounded_items",
                "unbounded", "face_directions"]
        return dict(zip(keys, list(out)))


def rays_handled_by(kernel, st):
    """Rays one frame's launches of `kernel` trace, from the frame's ft_stats (bench.py's roofline line)."""
    generated = st["rays_primary"] - st["rays_primary_culled"]
    if kernel == "primary":                                         # fused bounce 0: every generated primary ray + the shadow rays of its hits
        return generated + st["rays_shadow_primary"]
    # k_bounce ("shade"): the reflection rays of every level >= 1 and the shadow rays of their hits
    return st["rays_reflect"] + st["rays_shadow"] - st["rays_shadow_primary"]


def ls_topology(n, ls_first, first_node):
    """ft_debug_ls_topology: the tree option "light_space_retree" gives n sorted leaf records from ls_first on in a block of nodes from
    first_node on, as the host generates it - (child words N x 4 int32, order N uint32, levels k x 2 uint32: offset into order and count,
    deepest level first)."""
    fn = hip_lib().ft_debug_ls_topology
    fn.restype, fn.argtypes = C.c_int32, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p]
    sizes = (C.c_int64 * 2)()
    rc = fn(n, ls_first, first_node, sizes, None, None, None)
    if rc < 0:
        raise FtError(rc, "ls_topology")
    child, order, levels = np.zeros((sizes[0], 4), dtype=np.int32), np.zeros(sizes[0], dtype=np.uint32), np.zeros((sizes[1], 2), dtype=np.uint32)
    rc = fn(n, ls_first, first_node, sizes, child.ctypes.data, order.ctypes.data, levels.ctypes.data)
    if rc < 0:
        raise FtError(rc, "ls_topology")
    return child, order, levels


def debug_slice(p0, n, tri):
    """Triangle.slice as implemented by the product's BSP builder."""
    above, below = np.zeros(18), np.zeros(18)
    na, nb = C.c_int32(), C.c_int32()
    tri = _capi.as_f64(tri, (9,))
    rc = hip_lib().ft_debug_slice(_capi.dptr(_capi.as_f64(p0)), _capi.dptr(_capi.as_f64(n)), _capi.dptr(tri), _capi.dptr(above), C.byref(na),
                                  _capi.dptr(below), C.byref(nb))
    if rc < 0:
        raise FtError(rc, "slice")
    return above[:9 * na.value].reshape(-1, 3, 3), below[:9 * nb.value].reshape(-1, 3, 3)
