"""Python mirror of the reference's host interface for the hot path, over the pt_api.h /
pt_scene.h C ABI (ctypes; build/libptrace.so).

Names follow the reference so that its call sequence reads the same:
  load_vertex_data(obj, mtl)  geometry_loader.h:15-142   -> (tris[N,16], mats[M,16])
  buildSAHTree(tris)          bvh.h:255-268              -> nodes[K,12]
  setupBuffers(obj, mtl)      ogl_path_trace.h:367-530   -> SceneBuffers (5 std140 buffers)
  ComputeShader / PathTracer  shader_c.h + glDispatchCompute(ogl_path_trace.h:174-186)
    .dispatch(frame, accumulate)        one reference dispatch (uniforms frame/accumulate)
    .render(frame_first, n, acc_first)  n dispatches fused in one launch (bit-identical)
Errors raise PTError carrying the library's code and message (the reference prints and
continues; the drop-in fails loudly instead -- DESIGN.md §1).

There is no CPU fallback: if the HIP library is missing or no device is present, the
calls raise.  The CPU oracle lives in oracle/ and is only used by tests and the bench's
cpu_baseline leg.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# PT_LIB selects another in-tree build of the same library (tools/ab.py A/B timing only).
LIB_PATH = os.environ.get("PT_LIB") or os.path.join(PKG_DIR, "build", "libptrace.so")
INCLUDE_DIR = os.path.join(os.path.dirname(PKG_DIR), "include")

PT_FLAG_NO_AA, PT_FLAG_NO_SKY, PT_FLAG_NO_SPHERES, PT_FLAG_NO_TRIANGLES, PT_FLAG_REF_DISPATCH = 1, 2, 4, 8, 16
PT_FLAG_MOLLER_TRUMBORE = 32   # opt-in fast triangle test (not the reference image; see pt_api.h)
DEFAULT_CAMERA = np.array([0, -6, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)  # ogl_path_trace.h:53-54

_ERR = {-1: "PT_E_ARG", -2: "PT_E_IO", -3: "PT_E_PARSE", -4: "PT_E_SCENE", -5: "PT_E_HIP", -6: "PT_E_STATE",
        -7: "PT_E_RCCL"}


class PTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (_ERR.get(code, "PT_E?"), code, msg))
        self.code = code


class _Config(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "height", "max_bounce", "display_mode", "flags",
                                       "rays_per_pixel", "device", "rank", "world")]


class ViewerFrame(C.Structure):
    """pt_viewer_frame_info (include/pt_viewer.h)."""
    _fields_ = [("camera", C.c_float * 12), ("frame", C.c_int), ("accumulate", C.c_int),
                ("display_mode", C.c_int), ("should_close", C.c_int)]


class NoiseStats(C.Structure):
    """pt_noise_stats (include/pt_api.h): the integer noise summary of a context's pixels."""
    _fields_ = [("pixels", C.c_ulonglong), ("sum_q", C.c_ulonglong), ("above", C.c_ulonglong),
                ("max_q", C.c_uint), ("frames", C.c_int)]

    def as_dict(self):
        """The fields, plus the mean / largest relative error and the fraction above the target."""
        n = max(int(self.pixels), 1)
        return dict(pixels=int(self.pixels), sum_q=int(self.sum_q), above=int(self.above), max_q=int(self.max_q),
                    frames=int(self.frames), mean=int(self.sum_q) / n / 65536.0, max=int(self.max_q) / 65536.0,
                    above_frac=int(self.above) / n)


class AdaptiveStats(C.Structure):
    """pt_adaptive_stats (include/pt_api.h): the summary of a pt_render_adaptive call."""
    _fields_ = [("noise", NoiseStats), ("tiles", C.c_ulonglong), ("tiles_active", C.c_ulonglong),
                ("pixel_frames", C.c_ulonglong)]

    def as_dict(self):
        """NoiseStats.as_dict of the noise summary, plus tiles, tiles_active and pixel_frames."""
        return dict(self.noise.as_dict(), tiles=int(self.tiles), tiles_active=int(self.tiles_active),
                    pixel_frames=int(self.pixel_frames))


class DenoiseParams(C.Structure):
    """pt_denoise_params (include/pt_api.h)."""
    _fields_ = [("iterations", C.c_int), ("guide_frames", C.c_int), ("sigma_lum", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float)]


class DenoiseInfo(C.Structure):
    """pt_denoise_info (include/pt_api.h)."""
    _fields_ = [(n, C.c_int) for n in ("guided", "guides_rendered", "iterations", "frames")]


PT_CAM_PINHOLE, PT_CAM_THIN_LENS, PT_CAM_ORTHO, PT_CAM_EQUIRECT = 0, 1, 2, 3
PT_CAM_NO_AA = 1
CAMERA_MODELS = {"pinhole": PT_CAM_PINHOLE, "thinlens": PT_CAM_THIN_LENS, "ortho": PT_CAM_ORTHO,
                 "equirect": PT_CAM_EQUIRECT}


class Camera(C.Structure):
    """pt_camera (include/pt_api.h): Camera("thinlens", W, H, cam, aperture=0.05, focus=6.0),
    Camera("ortho", W, H, cam, ortho_width=4.0), Camera("equirect", W, H, cam, aa=False), ...  model: a name of
    CAMERA_MODELS or a PT_CAM_* value; cam: the 12 floats of pt_set_camera (None: the reference's default)."""
    _fields_ = [("model", C.c_int), ("width", C.c_int), ("height", C.c_int), ("flags", C.c_int),
                ("cam", C.c_float * 12), ("aperture", C.c_float), ("focus", C.c_float), ("ortho_width", C.c_float),
                ("pad", C.c_float)]

    def __init__(self, model="pinhole", width=1, height=1, cam=None, aperture=0.0, focus=1.0, ortho_width=1.0,
                 aa=True, flags=None):
        super().__init__()
        self.model = CAMERA_MODELS[model] if isinstance(model, str) else int(model)
        self.width, self.height = int(width), int(height)
        self.flags = int(flags) if flags is not None else (0 if aa else PT_CAM_NO_AA)
        self.cam[:] = [float(v) for v in np.asarray(DEFAULT_CAMERA if cam is None else cam, np.float32).reshape(12)]
        self.aperture, self.focus, self.ortho_width = float(aperture), float(focus), float(ortho_width)

    @property
    def pixels(self):
        return self.width * self.height


def denoise_params(**params):
    """pt_denoise_defaults, with the given fields replaced."""
    p = DenoiseParams()
    lib().pt_denoise_defaults(C.byref(p))
    names = [n for n, _ in DenoiseParams._fields_]
    for key, value in params.items():
        if key not in names:
            raise TypeError("unknown denoise parameter %r (one of %s)" % (key, ", ".join(names)))
        setattr(p, key, value)
    return p


_lib = None
_F = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_I = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


def build(force=False):
    """Compile build/libptrace.so (hipcc, gfx950) in-tree."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, "all"])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PTError(-5, "native library %s is missing; run `make -C %s`" % (LIB_PATH, PKG_DIR))
        L = C.CDLL(LIB_PATH)
        vp, ip, fp = C.c_void_p, C.c_int, C.c_float
        sig = {
            "pt_scene_load_obj": (ip, [C.c_char_p, C.c_char_p, C.POINTER(vp)]),
            "pt_scene_load_obj_ex": (ip, [C.c_char_p, C.c_char_p, ip, C.POINTER(vp)]),
            "pt_scene_from_arrays": (ip, [_F, ip, _F, ip, C.POINTER(vp)]),
            "pt_scene_add_builtins": (ip, [vp]),
            "pt_scene_build_bvh": (ip, [vp]),
            "pt_scene_counts": (ip, [vp, np.ctypeslib.ndpointer(np.int32)]),
            "pt_scene_get_tris": (ip, [vp, _F, ip]),
            "pt_scene_get_mats": (ip, [vp, _F, ip]),
            "pt_scene_get_spheres": (ip, [vp, _F, ip]),
            "pt_scene_get_nodes": (ip, [vp, _F, ip]),
            "pt_scene_last_error": (C.c_char_p, [vp]),
            "pt_scene_free": (None, [vp]),
            "pt_bvh_build": (ip, [_F, ip, _F, ip, C.POINTER(ip)]),
            "pt_bvh_build_gpu": (ip, [_F, ip, _F, ip, C.POINTER(ip), ip]),
            "pt_scene_build_bvh_gpu": (ip, [vp, ip]),
            "pt_bvh_last_error": (C.c_char_p, []),
            "pt_bvh_culling_ok": (ip, [_F, ip]),
            "pt_aces_rgba8_host": (None, [_F, C.c_longlong, np.ctypeslib.ndpointer(np.uint8)]),
            "pt_create": (ip, [C.POINTER(_Config), C.POINTER(vp)]),
            "pt_destroy": (None, [vp]),
            "pt_last_error": (C.c_char_p, [vp]),
            "pt_upload_scene": (ip, [vp, _F, ip, _F, ip, _F, ip, _F, ip]),
            "pt_set_camera": (ip, [vp, _F]),
            "pt_render": (ip, [vp, ip, ip, ip]),
            "pt_render_async": (ip, [vp, ip, ip, ip]),
            "pt_sync": (ip, [vp]),
            "pt_rows": (ip, [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]),
            "pt_read_rgba32f": (ip, [vp, vp, C.c_size_t]),
            "pt_read_rgba8_aces": (ip, [vp, vp, C.c_size_t]),
            "pt_write_rgba32f": (ip, [vp, vp, C.c_size_t]),
            "pt_present_begin": (ip, [vp, ip]),
            "pt_present_end": (ip, [vp, ip, C.POINTER(C.POINTER(C.c_ubyte))]),
            "pt_accum_device": (ip, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
            "pt_stream": (ip, [vp, C.POINTER(vp)]),
            "pt_set_counting": (ip, [vp, ip]),
            "pt_stats": (ip, [vp, C.POINTER(C.c_double), np.ctypeslib.ndpointer(np.uint64)]),
            "pt_set_kernel": (ip, [vp, ip]),
            "pt_copy_rows_device": (ip, [vp, vp, C.c_size_t]),
            "pt_timing": (ip, [vp, C.POINTER(C.c_double), C.POINTER(ip), ip]),
            "pt_stats_ex": (ip, [vp, np.ctypeslib.ndpointer(np.uint64)]),
            "pt_debug_launches": (ip, [vp, np.ctypeslib.ndpointer(np.uint64)]),
            "pt_debug_window_cull": (ip, [vp, C.POINTER(ip), C.POINTER(fp)]),
            "pt_debug_sweep": (ip, [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]),
            "pt_debug_pool": (ip, [vp, C.POINTER(ip)]),
            "pt_debug_tile_order": (ip, [vp, C.POINTER(C.c_ulonglong), vp, ip, C.POINTER(ip), C.POINTER(ip)]),
            "pt_set_tuning": (ip, [vp, ip, ip]),
            "pt_progressive_setup": (ip, [vp, ip, ip]),
            "pt_progressive_reset": (ip, [vp, ip]),
            "pt_progressive_run": (ip, [vp, ip]),
            "pt_set_display_mode": (ip, [vp, ip]),
            "pt_get_config": (ip, [vp, C.POINTER(_Config)]),
            "pt_set_moments": (ip, [vp, ip]),
            "pt_read_moments": (ip, [vp, vp, C.c_size_t, C.POINTER(ip)]),
            "pt_noise": (ip, [vp, fp, C.POINTER(NoiseStats)]),
            "pt_noise_host": (ip, [_F, vp, C.c_size_t, ip, fp, C.POINTER(NoiseStats)]),
            "pt_render_until": (ip, [vp, ip, ip, ip, ip, fp, C.POINTER(ip), C.POINTER(NoiseStats)]),
            "pt_group_noise": (ip, [vp, fp, C.POINTER(NoiseStats)]),
            "pt_render_adaptive": (ip, [vp, ip, ip, ip, ip, fp, C.POINTER(ip), C.POINTER(AdaptiveStats)]),
            "pt_read_tile_frames": (ip, [vp, vp, ip, C.POINTER(ip), C.POINTER(ip)]),
            "pt_tile_retires_host": (ip, [_F, vp, C.c_size_t, ip, fp, C.POINTER(ip)]),
            "pt_denoise_defaults": (None, [C.POINTER(DenoiseParams)]),
            "pt_denoise": (ip, [vp, C.POINTER(DenoiseParams), C.POINTER(DenoiseInfo)]),
            "pt_denoise_async": (ip, [vp, C.POINTER(DenoiseParams), C.POINTER(DenoiseInfo)]),
            "pt_read_denoised_rgba32f": (ip, [vp, vp, C.c_size_t]),
            "pt_read_denoised_rgba8_aces": (ip, [vp, vp, C.c_size_t]),
            "pt_read_guides": (ip, [vp, vp, C.c_size_t]),
            "pt_denoise_host": (ip, [_F, vp, _F, vp, ip, ip, C.POINTER(DenoiseParams), _F]),
            "pt_intersect": (ip, [vp, vp, C.c_longlong, vp, ip]),
            "pt_intersect_device": (ip, [vp, vp, C.c_longlong, vp, ip]),
            "pt_pixel_rays": (ip, [ip, ip, _F, vp, C.c_longlong, vp]),
            "pt_pick": (ip, [vp, vp, C.c_longlong, vp]),
            "pt_intersect_host": (ip, [_F, ip, _F, ip, _F, ip, _F, ip, ip, vp, C.c_longlong, vp, ip]),
            "pt_trace": (ip, [vp, vp, vp, C.c_longlong, ip, ip, ip, vp]),
            "pt_trace_device": (ip, [vp, vp, vp, C.c_longlong, ip, ip, ip, vp]),
            "pt_pixel_seeds": (ip, [vp, C.c_longlong, vp]),
            "pt_trace_host": (ip, [_F, ip, _F, ip, _F, ip, _F, ip, ip, ip, ip, vp, vp, C.c_longlong, ip, ip, ip, vp]),
            "pt_trace_camera": (ip, [vp, C.POINTER(Camera), ip, ip, ip, vp]),
            "pt_trace_camera_device": (ip, [vp, C.POINTER(Camera), ip, ip, ip, vp]),
            "pt_trace_camera_host": (ip, [_F, ip, _F, ip, _F, ip, _F, ip, ip, ip, ip, C.POINTER(Camera), ip, ip, ip, vp]),
            "pt_camera_rays_host": (ip, [C.POINTER(Camera), vp, C.c_longlong, ip, vp, vp]),
            "pt_camera_rays_device": (ip, [vp, C.POINTER(Camera), ip, vp, vp]),
            "pt_film_create": (ip, [vp, C.POINTER(Camera), ip, C.POINTER(vp)]),
            "pt_film_destroy": (None, [vp]),
            "pt_film_set_camera": (ip, [vp, C.POINTER(Camera)]),
            "pt_film_expose": (ip, [vp, ip, ip, ip]),
            "pt_film_noise": (ip, [vp, fp, C.POINTER(NoiseStats)]),
            "pt_film_expose_until": (ip, [vp, ip, ip, ip, ip, fp, C.POINTER(ip), C.POINTER(NoiseStats)]),
            "pt_film_denoise": (ip, [vp, C.POINTER(DenoiseParams), C.POINTER(DenoiseInfo)]),
            "pt_film_info": (ip, [vp, C.POINTER(ip), C.POINTER(ip)]),
            "pt_film_read": (ip, [vp, ip, vp, C.c_size_t]),
            "pt_film_device": (ip, [vp, ip, C.POINTER(vp), C.POINTER(C.c_size_t)]),
            "pt_film_expose_host": (ip, [_F, ip, _F, ip, _F, ip, _F, ip, ip, ip, ip, C.POINTER(Camera), ip, ip, ip, ip, ip,
                                         ip, _F, _F, _F, C.POINTER(ip)]),
            "pt_group_create": (ip, [C.POINTER(vp), ip, C.POINTER(vp)]),
            "pt_group_destroy": (None, [vp]),
            "pt_group_last_error": (C.c_char_p, [vp]),
            "pt_group_upload_scene": (ip, [vp, _F, ip, _F, ip, _F, ip, _F, ip]),
            "pt_group_gather_rgba32f": (ip, [vp, vp, C.c_size_t, ip]),
            "pt_group_stats": (ip, [vp, C.POINTER(C.c_double), C.POINTER(C.c_size_t)]),
            "pt_group_gather_rgba8_aces": (ip, [vp, vp, C.c_size_t, ip]),
            "pt_group_present_begin": (ip, [vp, ip]),
            "pt_group_present_end": (ip, [vp, ip, C.POINTER(C.POINTER(C.c_ubyte))]),
            "pt_gather_rgba32f": (ip, [C.POINTER(vp), ip, vp, C.c_size_t, ip]),
            "pt_group_plan": (ip, [_I, _I, ip, _I, C.POINTER(ip), _I, _I, C.POINTER(ip), _I]),
            "pt_group_interleave_host": (ip, [_F, C.c_size_t, _I, ip, ip, ip, _F]),
            "pt_viewer_create": (ip, [vp, ip, C.POINTER(vp)]),
            "pt_viewer_destroy": (None, [vp]),
            "pt_viewer_set_params": (ip, [vp, fp, fp, ip]),
            "pt_viewer_key": (ip, [vp, ip, ip]),
            "pt_viewer_cursor": (ip, [vp, C.c_double, C.c_double]),
            "pt_viewer_should_close": (ip, [vp]),
            "pt_viewer_next": (ip, [vp, C.c_double, C.POINTER(ViewerFrame)]),
            "pt_viewer_frame": (ip, [vp, vp, C.c_double, C.POINTER(ViewerFrame)]),
        }
        for name, (res, args) in sig.items():
            # tools/ab_inproc.py loads older builds beside this one: PT_LIB_PARTIAL=1 lets a
            # build without the newer entry points load (the product always binds all of them)
            if os.environ.get("PT_LIB_PARTIAL") == "1" and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def header_symbols():
    """Function names declared in include/*.h (for the ABI export test)."""
    import re
    names = []
    for h in ("pt_api.h", "pt_scene.h", "pt_viewer.h", "pt_group.h"):
        txt = open(os.path.join(INCLUDE_DIR, h)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        names += re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(names))


# ----------------------------------------------------------------------------- scene ingest
def _f32(a, cols):
    a = np.ascontiguousarray(a, np.float32)
    return a.reshape(-1, cols) if a.size else np.zeros((0, cols), np.float32)


class _Scene:
    def __init__(self, handle):
        self.h = handle

    def __del__(self):
        if getattr(self, "h", None):
            lib().pt_scene_free(self.h)
            self.h = None

    def check(self, rc):
        if rc:
            raise PTError(rc, lib().pt_scene_last_error(self.h).decode())

    def counts(self):
        c = np.zeros(5, np.int32)
        self.check(lib().pt_scene_counts(self.h, c))
        return dict(n_tris=int(c[0]), n_mats=int(c[1]), n_spheres=int(c[2]), n_nodes=int(c[3]), n_loaded_mats=int(c[4]))

    def arrays(self):
        c = self.counts()
        out = {}
        for key, n, cols, fn in (("tris", c["n_tris"], 16, lib().pt_scene_get_tris),
                                 ("mats", c["n_mats"], 16, lib().pt_scene_get_mats),
                                 ("spheres", c["n_spheres"], 8, lib().pt_scene_get_spheres),
                                 ("nodes", c["n_nodes"], 12, lib().pt_scene_get_nodes)):
            a = np.zeros((max(n, 1), cols), np.float32)
            self.check(fn(self.h, a, max(n, 1)))
            out[key] = a[:n].copy()
        out["n_loaded_mats"] = c["n_loaded_mats"]
        return out


def load_vertex_data(obj_path, mtl_path):
    """geometry_loader.h:15 -> (tris[N,16], mats[M,16]) float32 std140 records."""
    h = C.c_void_p()
    rc = lib().pt_scene_load_obj(str(obj_path).encode(), str(mtl_path).encode(), C.byref(h))
    s = _Scene(h)
    s.check(rc)
    a = s.arrays()
    return a["tris"], a["mats"]


def load_obj_robust(obj_path, mtl_path=None):
    """General Wavefront ingest (pt_scene_load_obj_ex, PT_LOAD_ROBUST) -> (tris, mats);
    mtl_path None = the OBJ's `mtllib`."""
    h = C.c_void_p()
    rc = lib().pt_scene_load_obj_ex(str(obj_path).encode(), None if mtl_path is None else str(mtl_path).encode(),
                                    1, C.byref(h))
    if not h.value:
        raise PTError(rc, "pt_scene_load_obj_ex failed")
    s = _Scene(h)
    s.check(rc)
    a = s.arrays()
    return a["tris"], a["mats"]


def buildSAHTree(tris, device=None):
    """bvh.h:255 -> nodes[K,12] {min, max, {tri0, tri1, hit, miss}} (preorder-pair layout).
    device: None = the host builder (pt_bvh_build), else the GPU builder on that device
    (pt_bvh_build_gpu; the same output)."""
    tris = _f32(tris, 16)
    n = len(tris)
    out = np.zeros((max(2 * n, 1), 12), np.float32)
    nn = C.c_int()
    src = tris.reshape(-1) if n else np.zeros(16, np.float32)
    if device is None:
        rc = lib().pt_bvh_build(src, n, out.reshape(-1), len(out), C.byref(nn))
    else:
        rc = lib().pt_bvh_build_gpu(src, n, out.reshape(-1), len(out), C.byref(nn), int(device))
    if rc:
        raise PTError(rc, lib().pt_bvh_last_error().decode())
    return out[: nn.value].copy()


class SceneBuffers(dict):
    """The five SSBO contents of setupBuffers(): tris, nodes, mats, spheres, cam."""


def setupBuffers(obj_path, mtl_path, camera=None, device=None, robust=False):
    """ogl_path_trace.h:367-530: load, build the BVH, append built-ins + metal sphere.
    device: None = the host builder, else pt_scene_build_bvh_gpu on that device (the same nodes).
    robust: read the OBJ with the general Wavefront reader (pt_scene_load_obj_ex, PT_LOAD_ROBUST)."""
    h = C.c_void_p()
    if robust:
        rc = lib().pt_scene_load_obj_ex(str(obj_path).encode(), None if mtl_path is None else str(mtl_path).encode(),
                                        1, C.byref(h))
        if not h.value:
            raise PTError(rc, "pt_scene_load_obj_ex failed")
    else:
        rc = lib().pt_scene_load_obj(str(obj_path).encode(), str(mtl_path).encode(), C.byref(h))
    s = _Scene(h)
    s.check(rc)
    s.check(lib().pt_scene_add_builtins(s.h))
    s.check(lib().pt_scene_build_bvh(s.h) if device is None else lib().pt_scene_build_bvh_gpu(s.h, int(device)))
    a = s.arrays()
    a["cam"] = DEFAULT_CAMERA.copy() if camera is None else np.asarray(camera, np.float32).reshape(12)
    return SceneBuffers(a)


def scene_from_arrays(tris, mats, builtins=True, camera=None):
    tris, mats = _f32(tris, 16), _f32(mats, 16)
    h = C.c_void_p()
    rc = lib().pt_scene_from_arrays(tris.reshape(-1) if len(tris) else np.zeros(16, np.float32), len(tris),
                                    mats.reshape(-1) if len(mats) else np.zeros(16, np.float32), len(mats), C.byref(h))
    s = _Scene(h)
    s.check(rc)
    if builtins:
        s.check(lib().pt_scene_add_builtins(s.h))
    if len(tris):
        s.check(lib().pt_scene_build_bvh(s.h))
    a = s.arrays()
    a["cam"] = DEFAULT_CAMERA.copy() if camera is None else np.asarray(camera, np.float32).reshape(12)
    return SceneBuffers(a)


def bvh_culling_ok(nodes):
    """pt_bvh_culling_ok: does the threaded tree qualify for the culling walk?"""
    n = _f32(nodes, 12)
    return bool(lib().pt_bvh_culling_ok(n.reshape(-1) if len(n) else np.zeros(12, np.float32), len(n)))


def aces_rgba8_host(img):
    img = np.ascontiguousarray(img, np.float32)
    out = np.zeros(img.shape[:-1] + (4,), np.uint8)
    lib().pt_aces_rgba8_host(img.reshape(-1), img.size // 4, out.reshape(-1))
    return out


# ----------------------------------------------------------------------------- renderer
class PathTracer:
    """The compute program + its image: pt_create / pt_upload_scene / pt_render."""

    def __init__(self, width, height, max_bounce=5, display_mode=1, flags=0, rays_per_pixel=1,
                 device=0, rank=0, world=1):
        cfg = _Config(width, height, max_bounce, display_mode, flags, rays_per_pixel, device, rank, world)
        h = C.c_void_p()
        rc = lib().pt_create(C.byref(cfg), C.byref(h))
        self.h = h
        self.width, self.height = width, height
        self._check(rc)
        rl, r0, rs = C.c_int(), C.c_int(), C.c_int()
        self._check(lib().pt_rows(self.h, C.byref(rl), C.byref(r0), C.byref(rs)))
        self.rows_local, self.row0, self.row_stride = rl.value, r0.value, rs.value

    def _check(self, rc):
        if rc:
            raise PTError(rc, lib().pt_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            lib().pt_destroy(self.h)
            self.h = None

    __del__ = close

    def upload(self, sb):
        t, n, m, s = _f32(sb["tris"], 16), _f32(sb["nodes"], 12), _f32(sb["mats"], 16), _f32(sb["spheres"], 8)
        z = lambda a, c: a.reshape(-1) if a.size else np.zeros(c, np.float32)
        self._check(lib().pt_upload_scene(self.h, z(t, 16), len(t), z(n, 12), len(n), z(m, 16), len(m), z(s, 8), len(s)))
        if "cam" in sb:
            self.set_camera(sb["cam"])

    def set_camera(self, cam):
        self._check(lib().pt_set_camera(self.h, np.ascontiguousarray(cam, np.float32).reshape(12)))

    def set_display_mode(self, mode):
        """Uniform displayMode (ogl_path_trace.h:182)."""
        self._check(lib().pt_set_display_mode(self.h, int(mode)))

    def set_counting(self, on=True):
        self._check(lib().pt_set_counting(self.h, int(bool(on))))

    def set_kernel(self, variant):
        self._check(lib().pt_set_kernel(self.h, int(variant)))

    def set_tuning(self, leaf_thresh=None, shade_thresh=None, adaptive=None, waves_per_simd=None, group=None,
                   trav_floor=None, compact_max=None, scratch_mib=None):
        if leaf_thresh is not None:
            self._check(lib().pt_set_tuning(self.h, 0, int(leaf_thresh)))
        if shade_thresh is not None:
            self._check(lib().pt_set_tuning(self.h, 1, int(shade_thresh)))
        if adaptive is not None:
            self._check(lib().pt_set_tuning(self.h, 2, int(bool(adaptive))))
        if waves_per_simd is not None:
            self._check(lib().pt_set_tuning(self.h, 3, int(waves_per_simd)))
        if group is not None:
            self._check(lib().pt_set_tuning(self.h, 5, int(group)))
        if trav_floor is not None:
            self._check(lib().pt_set_tuning(self.h, 6, int(trav_floor)))
        if compact_max is not None:
            self._check(lib().pt_set_tuning(self.h, 7, int(compact_max)))
        if scratch_mib is not None:
            self._check(lib().pt_set_tuning(self.h, 8, int(scratch_mib)))

    def set_culling(self, enable):
        """Tuning key 15: the LDS walk's conservative culling (on by default where the tree
        qualifies).  Never changes the image."""
        self._check(lib().pt_set_tuning(self.h, 15, 0 if enable else 1))

    def set_common(self, enable):
        """Tuning key 21: the specialised default-path kernel (on by default where the launch
        qualifies).  Never changes the image."""
        self._check(lib().pt_set_tuning(self.h, 21, 0 if enable else 1))

    def set_window_cull(self, enable):
        """Tuning key 22: the window clause of the LDS culling walk (on by default; DESIGN.md
        §5.6).  Never changes the image."""
        self._check(lib().pt_set_tuning(self.h, 22, 0 if enable else 1))

    def window_cull(self):
        """pt_debug_window_cull -> (the clause is active, the scene's window slack)."""
        a, s = C.c_int(), C.c_float()
        self._check(lib().pt_debug_window_cull(self.h, C.byref(a), C.byref(s)))
        return bool(a.value), float(s.value)

    def set_sweep(self, enable):
        """Tuning key 23: the leaf sweep of scenes with a few leaves (on by default where the scene
        qualifies; DESIGN.md §5.6, "The leaf sweep").  Never changes the image."""
        self._check(lib().pt_set_tuning(self.h, 23, 0 if enable else 1))

    def leaf_sweep(self):
        """pt_debug_sweep -> dict(swept: the last launch ran the sweep, qualifies: the scene has a
        sweep table, n_leaves: its leaf pairs)."""
        a, q, n = C.c_int(), C.c_int(), C.c_int()
        fn = getattr(lib(), "pt_debug_sweep", None)     # (an older build loaded with PT_LIB_PARTIAL has none)
        if fn is not None:
            self._check(fn(self.h, C.byref(a), C.byref(q), C.byref(n)))
        return dict(swept=bool(a.value), qualifies=bool(q.value), n_leaves=int(n.value))

    def set_pool(self, enable):
        """Tuning key 24: the per-wave path pool of the specialised swept line.  Never
        changes the image."""
        self._check(lib().pt_set_tuning(self.h, 24, 0 if enable else 1))

    def pooled(self):
        """pt_debug_pool -> the last render launch ran the path-pool kernel."""
        a = C.c_int()
        fn = getattr(lib(), "pt_debug_pool", None)      # (an older build loaded with PT_LIB_PARTIAL has none)
        if fn is not None:
            self._check(fn(self.h, C.byref(a)))
        return bool(a.value)

    def tile_order(self):
        """pt_debug_tile_order -> dict(sorts: tile-order sorts since the scene upload, n_tiles, tiles_x:
        the tile grid, perm: the order the next launch reads as (n_tiles, 2) int (ty, tx)).  Waits
        for the context's work."""
        n, tx, sorts = C.c_int(), C.c_int(), C.c_ulonglong()
        self._check(lib().pt_debug_tile_order(self.h, None, None, 0, C.byref(n), None))
        perm = np.zeros(max(n.value, 1), np.uint32)
        self._check(lib().pt_debug_tile_order(self.h, C.byref(sorts), perm.ctypes.data, len(perm), C.byref(n),
                                              C.byref(tx)))
        perm = perm[: n.value]
        return dict(sorts=int(sorts.value), n_tiles=n.value, tiles_x=tx.value,
                    perm=np.stack([perm >> 16, perm & 0xffff], 1).astype(np.int64))

    def launches(self):
        """pt_debug_launches -> (launches on a generic line, on the specialised line)."""
        v = np.zeros(2, np.uint64)
        self._check(lib().pt_debug_launches(self.h, v))
        return int(v[0]), int(v[1])

    def set_key(self, key, value):
        """Raw pt_set_tuning(key, value) (experiments)."""
        self._check(lib().pt_set_tuning(self.h, int(key), int(value)))

    def dispatch(self, frame, accumulate):
        """One glDispatchCompute with uniforms frame/accumulate (ogl_path_trace.h:176-183)."""
        self._check(lib().pt_render(self.h, frame, 1, accumulate))

    def render(self, frame_first, n_frames, accumulate_first):
        self._check(lib().pt_render(self.h, frame_first, n_frames, accumulate_first))

    def render_async(self, frame_first, n_frames, accumulate_first):
        self._check(lib().pt_render_async(self.h, frame_first, n_frames, accumulate_first))

    def sync(self):
        self._check(lib().pt_sync(self.h))

    def read_rgba32f(self):
        out = np.zeros((self.rows_local, self.width, 4), np.float32)
        self._check(lib().pt_read_rgba32f(self.h, out.ctypes.data, out.nbytes))
        return out

    def write_rgba32f(self, img):
        img = np.ascontiguousarray(img, np.float32)
        self._check(lib().pt_write_rgba32f(self.h, img.ctypes.data, img.nbytes))

    def read_rgba8(self):
        out = np.zeros((self.rows_local, self.width, 4), np.uint8)
        self._check(lib().pt_read_rgba8_aces(self.h, out.ctypes.data, out.nbytes))
        return out

    def present_begin(self, buf):
        """Enqueue the ACES RGBA8 image of the renders issued so far into pinned buffer buf
        (0..3) without waiting (pt_present_begin)."""
        self._check(lib().pt_present_begin(self.h, int(buf)))

    def present_end(self, buf, copy=True):
        """Wait for buffer buf and return its (rows_local, W, 4) uint8 pixels: a copy, or with
        copy=False a view of the pinned buffer, valid until the next present_begin(buf)."""
        ptr = C.POINTER(C.c_ubyte)()
        self._check(lib().pt_present_end(self.h, int(buf), C.byref(ptr)))
        view = np.ctypeslib.as_array(ptr, shape=(self.rows_local, self.width, 4))
        return view.copy() if copy else view

    def accum_device(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(lib().pt_accum_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def progressive_setup(self, frames_per_launch, launches_per_replay):
        """Capture the progressive sample loop as a hipGraph (see pt_api.h)."""
        self._check(lib().pt_progressive_setup(self.h, int(frames_per_launch), int(launches_per_replay)))

    def progressive_reset(self, next_frame=1):
        self._check(lib().pt_progressive_reset(self.h, int(next_frame)))

    def progressive_run(self, replays=1, sync=True):
        self._check(lib().pt_progressive_run(self.h, int(replays)))
        if sync:
            self.sync()

    def set_moments(self, enable=True):
        """Keep per-pixel luminance moments beside the image (pt_set_moments): the noise estimate
        of noise() / render_until().  Never changes the image."""
        self._check(lib().pt_set_moments(self.h, int(bool(enable))))

    def read_moments(self):
        """-> ((rows_local, W, 2) float32 of (S1, S2), frames folded in)."""
        out = np.zeros((self.rows_local, self.width, 2), np.float32)
        n = C.c_int()
        self._check(lib().pt_read_moments(self.h, out.ctypes.data, out.nbytes, C.byref(n)))
        return out, n.value

    def noise(self, target):
        """pt_noise: the integer noise summary of the local rows as a dict (NoiseStats.as_dict)."""
        s = NoiseStats()
        self._check(lib().pt_noise(self.h, float(target), C.byref(s)))
        return s.as_dict()

    def render_until(self, target, batch=16, max_frames=1024, frame_first=1, accumulate_first=0):
        """pt_render_until: frames in batches until the mean relative error is at most `target`
        (or max_frames) -> (frames_done, summary dict)."""
        done, s = C.c_int(), NoiseStats()
        self._check(lib().pt_render_until(self.h, int(frame_first), int(accumulate_first), int(batch), int(max_frames),
                                          float(target), C.byref(done), C.byref(s)))
        return done.value, s.as_dict()

    def render_adaptive(self, target, batch=16, max_frames=1024, frame_first=1, accumulate_first=0):
        """pt_render_adaptive: frames in batches, each work-queue tile until its own mean relative
        error is at most `target` (or max_frames) -> (frames_done, summary dict of
        AdaptiveStats.as_dict)."""
        done, s = C.c_int(), AdaptiveStats()
        self._check(lib().pt_render_adaptive(self.h, int(frame_first), int(accumulate_first), int(batch),
                                             int(max_frames), float(target), C.byref(done), C.byref(s)))
        return done.value, s.as_dict()

    def tile_frames(self):
        """pt_read_tile_frames -> (tiles_y, tiles_x) uint32: the frames each tile of the work queue
        received in the last render_adaptive (row 0 = the tiles of local row 0)."""
        n, tx = C.c_int(), C.c_int()
        self._check(lib().pt_read_tile_frames(self.h, None, 0, C.byref(n), C.byref(tx)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self._check(lib().pt_read_tile_frames(self.h, out.ctypes.data, len(out), C.byref(n), C.byref(tx)))
        return out[: n.value].reshape(-1, max(tx.value, 1))

    def denoise(self, sync=True, **params):
        """pt_denoise (sync=False: pt_denoise_async): the variance-guided a-trous filter of the image as
        of the renders issued so far.  params: fields of pt_denoise_params over its
        defaults.  -> dict(guided, guides_rendered, iterations, frames).  Never changes the image."""
        p, info = denoise_params(**params), DenoiseInfo()
        fn = lib().pt_denoise if sync else lib().pt_denoise_async
        self._check(fn(self.h, C.byref(p), C.byref(info)))
        return dict(guided=bool(info.guided), guides_rendered=bool(info.guides_rendered),
                    iterations=int(info.iterations), frames=int(info.frames))

    def read_denoised(self):
        """The last denoise's (rows_local, W, 4) float32 result: rgb filtered, alpha the image's."""
        out = np.zeros((self.rows_local, self.width, 4), np.float32)
        self._check(lib().pt_read_denoised_rgba32f(self.h, out.ctypes.data, out.nbytes))
        return out

    def read_denoised_rgba8(self):
        """... through the ACES view, (rows_local, W, 4) uint8."""
        out = np.zeros((self.rows_local, self.width, 4), np.uint8)
        self._check(lib().pt_read_denoised_rgba8_aces(self.h, out.ctypes.data, out.nbytes))
        return out

    def read_guides(self):
        """The guides of the last denoise, (rows_local, W, 8) float32: N.rgb, Z, A.rgb, 0."""
        out = np.zeros((self.rows_local, self.width, 8), np.float32)
        self._check(lib().pt_read_guides(self.h, out.ctypes.data, out.nbytes))
        return out

    def intersect(self, rays, any_hit=False):
        """pt_intersect: what each ray hits (RAY_DTYPE or (n, 8) float32 rays -> HIT_DTYPE), synchronous."""
        rays = _rays_in(rays)
        hits = np.zeros(len(rays), HIT_DTYPE)
        self._check(lib().pt_intersect(self.h, rays.ctypes.data, len(rays), hits.ctypes.data,
                                       PT_QUERY_ANY_HIT if any_hit else 0))
        return hits

    def intersect_device(self, rays_ptr, n, hits_ptr, any_hit=False):
        """pt_intersect_device: n rays at device pointer rays_ptr (32 B each) -> hits at hits_ptr (48 B each), e.g.
        the data_ptr() of torch tensors of shapes (n, 8) / (n, 12) float32; enqueued on the context's stream
        (stream()), not synchronised."""
        self._check(lib().pt_intersect_device(self.h, C.c_void_p(int(rays_ptr)), int(n), C.c_void_p(int(hits_ptr)),
                                              PT_QUERY_ANY_HIT if any_hit else 0))

    def pick(self, xy):
        """pt_pick: the closest hit under each of the (n, 2) pixels xy (row 0 = bottom) -> HIT_DTYPE."""
        xy = _xy_in(xy)
        hits = np.zeros(len(xy), HIT_DTYPE)
        self._check(lib().pt_pick(self.h, xy.ctypes.data, len(xy), hits.ctypes.data))
        return hits

    def trace(self, rays, seeds=None, frame_first=1, n_frames=1, prior=None):
        """pt_trace: the radiance along each ray (RAY_DTYPE or (n, 8) float32), frames frame_first ..
        frame_first + n_frames - 1 folded in frame order -> (n, 4) float32, synchronous.  seeds: (n,) uint32 (None:
        those of pixels (i, 0)).  prior: (n, 4) float32 the first frame averages over (None: it overwrites)."""
        rays = _rays_in(rays)
        seeds = _seeds_in(seeds, len(rays))
        out = _prior_in(prior, len(rays))
        self._check(lib().pt_trace(self.h, rays.ctypes.data, None if seeds is None else seeds.ctypes.data, len(rays),
                                   int(frame_first), int(n_frames), int(prior is not None), out.ctypes.data))
        return out

    def trace_device(self, rays_ptr, seeds_ptr, n, rgba_ptr, frame_first=1, n_frames=1, accumulate_first=0):
        """pt_trace_device: n rays at device pointer rays_ptr (32 B each), seeds at seeds_ptr (4 B each, or None) ->
        running means at rgba_ptr (16 B each, in/out); enqueued on the context's stream (stream()), not
        synchronised."""
        self._check(lib().pt_trace_device(self.h, C.c_void_p(int(rays_ptr)),
                                          C.c_void_p(int(seeds_ptr)) if seeds_ptr else None, int(n), int(frame_first),
                                          int(n_frames), int(accumulate_first), C.c_void_p(int(rgba_ptr))))

    def trace_camera(self, camera, frame_first=1, n_frames=1, prior=None):
        """pt_trace_camera: frames frame_first .. frame_first + n_frames - 1 of every pixel of the Camera, folded in
        frame order -> (height, width, 4) float32 (row 0 = bottom), synchronous.  prior: the image the first frame
        averages over (None: it overwrites)."""
        out = _prior_in(prior, camera.pixels)
        self._check(lib().pt_trace_camera(self.h, C.byref(camera), int(frame_first), int(n_frames),
                                          int(prior is not None), out.ctypes.data))
        return out.reshape(camera.height, camera.width, 4)

    def trace_camera_device(self, camera, rgba_ptr, frame_first=1, n_frames=1, accumulate_first=0):
        """pt_trace_camera_device: the same into the running means at device pointer rgba_ptr (16 B per pixel,
        in/out); enqueued on the context's stream (stream()), not synchronised."""
        self._check(lib().pt_trace_camera_device(self.h, C.byref(camera), int(frame_first), int(n_frames),
                                                 int(accumulate_first), C.c_void_p(int(rgba_ptr))))

    def camera_rays_device(self, camera, frame, rays_ptr, states_ptr=None):
        """pt_camera_rays_device: the Camera's ray of every pixel in frame `frame` at device pointer rays_ptr (32 B
        each, pixel order) and, where given, the random state after the camera's draws at states_ptr (4 B each);
        enqueued on the context's stream, not synchronised."""
        self._check(lib().pt_camera_rays_device(self.h, C.byref(camera), int(frame), C.c_void_p(int(rays_ptr)),
                                                C.c_void_p(int(states_ptr)) if states_ptr else None))

    def diag(self):
        """Lane utilisation per kernel phase from the last counting render."""
        v = np.zeros(16, np.uint64)
        self._check(lib().pt_stats_ex(self.h, v))
        util = lambda w, l: float(v[l]) / max(1.0, 64.0 * float(v[w]))
        return dict(trav_iters=int(v[5]), trav_util=util(5, 6), leaf_iters=int(v[7]), leaf_util=util(7, 8),
                    seg_iters=int(v[9]), seg_util=util(9, 10), slow_segments=int(v[11]), nan_segments=int(v[12]),
                    lds_bytes=int(v[13]), lds_bytes_sinks=int(v[14]), culling_walk=bool(v[15]),
                    swept=self.leaf_sweep()["swept"])

    def copy_rows_device(self, dst_ptr, nbytes):
        self._check(lib().pt_copy_rows_device(self.h, C.c_void_p(dst_ptr), nbytes))

    def timing(self, reset=False):
        ms, n = C.c_double(), C.c_int()
        self._check(lib().pt_timing(self.h, C.byref(ms), C.byref(n), int(bool(reset))))
        return ms.value, n.value

    def stream(self):
        s = C.c_void_p()
        self._check(lib().pt_stream(self.h, C.byref(s)))
        return s.value

    def stats(self):
        ms = C.c_double()
        cnt = np.zeros(5, np.uint64)
        self._check(lib().pt_stats(self.h, C.byref(ms), cnt))
        return ms.value, dict(segments=int(cnt[0]), node_visits=int(cnt[1]), tri_tests=int(cnt[2]),
                              sphere_tests=int(cnt[3]), hits=int(cnt[4]))


# ----------------------------------------------------------------------------- interactive loop
# GLFW key codes / actions the reference's key callback tests (ogl_path_trace.h:258-299)
KEY_SPACE, KEY_1, KEY_2, KEY_3, KEY_4 = 32, 49, 50, 51, 52
KEY_A, KEY_D, KEY_S, KEY_W, KEY_ESCAPE, KEY_LEFT_SHIFT = 65, 68, 83, 87, 256, 340
RELEASE, PRESS, REPEAT = 0, 1, 2


class Viewer:
    """The reference's render loop without its window (include/pt_viewer.h): GLFW
    callbacks handleMovementInput / cursorPosCallback, then one frame per frame() call."""

    def __init__(self, camera=None, display_mode=1, move_speed=10.0, rot_speed=0.1, accumulate=1):
        h = C.c_void_p()
        cam = None if camera is None else np.ascontiguousarray(camera, np.float32).reshape(12)
        rc = lib().pt_viewer_create(None if cam is None else cam.ctypes.data, int(display_mode), C.byref(h))
        if rc:
            raise PTError(rc, "pt_viewer_create")
        self.h = h
        self._cam = cam
        self._check(lib().pt_viewer_set_params(self.h, move_speed, rot_speed, int(accumulate)))

    def _check(self, rc):
        if rc:
            raise PTError(rc, "pt_viewer")

    def close(self):
        if getattr(self, "h", None):
            lib().pt_viewer_destroy(self.h)
            self.h = None

    __del__ = close

    def key(self, key, action):
        self._check(lib().pt_viewer_key(self.h, int(key), int(action)))

    def cursor(self, x, y):
        self._check(lib().pt_viewer_cursor(self.h, float(x), float(y)))

    @property
    def should_close(self):
        return bool(lib().pt_viewer_should_close(self.h))

    @staticmethod
    def _info(fi):
        return dict(camera=np.array(fi.camera[:], np.float32), frame=fi.frame, accumulate=fi.accumulate,
                    display_mode=fi.display_mode, should_close=bool(fi.should_close))

    def next(self, now):
        """Host side of one loop iteration -> its dispatch parameters."""
        fi = ViewerFrame()
        self._check(lib().pt_viewer_next(self.h, float(now), C.byref(fi)))
        return self._info(fi)

    def frame(self, pt, now):
        """One loop iteration rendered on PathTracer pt."""
        fi = ViewerFrame()
        rc = lib().pt_viewer_frame(self.h, pt.h, float(now), C.byref(fi))
        if rc:
            raise PTError(rc, lib().pt_last_error(pt.h).decode())
        return self._info(fi)


class Group:
    """pt_group.h: one process, several row-split contexts of one image -- the scene
    validated once and broadcast over RCCL, the frame gathered over RCCL and interleaved on the
    first context's device."""

    def __init__(self, tracers):
        self.tracers = list(tracers)
        arr = (C.c_void_p * len(self.tracers))(*[t.h for t in self.tracers])
        h = C.c_void_p()
        rc = lib().pt_group_create(arr, len(self.tracers), C.byref(h))
        self.h = h
        if rc:
            msg = lib().pt_group_last_error(h).decode() if h.value else ""
            self.close()
            raise PTError(rc, msg)
        t0 = self.tracers[0]
        self.W, self.H = t0.width, t0.height

    def _check(self, rc):
        if rc:
            raise PTError(rc, lib().pt_group_last_error(self.h).decode())

    def upload(self, sb):
        t, n, m, s = (_f32(sb["tris"], 16), _f32(sb["nodes"], 12), _f32(sb["mats"], 16), _f32(sb["spheres"], 8))
        flat = lambda a, c: a.reshape(-1) if len(a) else np.zeros(c, np.float32)
        self._check(lib().pt_group_upload_scene(self.h, flat(t, 16), len(t), flat(n, 12), len(n), flat(m, 16), len(m),
                                                flat(s, 8), len(s)))
        if "cam" in sb:
            for tr in self.tracers:
                tr.set_camera(sb["cam"])

    def gather(self, device_ptr=None):
        """The full (H, W, 4) frame: to host (numpy), or into device memory at device_ptr on the
        first context's device (returns None)."""
        nbytes = self.W * self.H * 16
        if device_ptr is not None:
            self._check(lib().pt_group_gather_rgba32f(self.h, C.c_void_p(device_ptr), nbytes, 1))
            return None
        out = np.zeros((self.H, self.W, 4), np.float32)
        self._check(lib().pt_group_gather_rgba32f(self.h, out.ctypes.data, nbytes, 0))
        return out

    def gather_rgba8(self, device_ptr=None):
        """The gathered frame through the ACES view (H, W, 4) uint8: to host, or into root-device
        memory at device_ptr (returns None)."""
        nbytes = self.W * self.H * 4
        if device_ptr is not None:
            self._check(lib().pt_group_gather_rgba8_aces(self.h, C.c_void_p(device_ptr), nbytes, 1))
            return None
        out = np.zeros((self.H, self.W, 4), np.uint8)
        self._check(lib().pt_group_gather_rgba8_aces(self.h, out.ctypes.data, nbytes, 0))
        return out

    def present_begin(self, buf):
        self._check(lib().pt_group_present_begin(self.h, int(buf)))

    def present_end(self, buf, copy=True):
        p = C.POINTER(C.c_ubyte)()
        self._check(lib().pt_group_present_end(self.h, int(buf), C.byref(p)))
        arr = np.ctypeslib.as_array(p, shape=(self.H, self.W, 4))
        return arr.copy() if copy else arr

    def noise(self, target):
        """pt_group_noise: the contexts' noise summaries added (PathTracer.noise's dict)."""
        s = NoiseStats()
        self._check(lib().pt_group_noise(self.h, float(target), C.byref(s)))
        return s.as_dict()

    def stats(self):
        ms, b = C.c_double(), C.c_size_t()
        self._check(lib().pt_group_stats(self.h, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().pt_group_destroy(self.h)
        self.h = C.c_void_p()


# ----------------------------------------------------------------------------- ray queries
PT_HIT_NONE, PT_HIT_SPHERE, PT_HIT_TRIANGLE = 0, 1, 2
PT_QUERY_ANY_HIT = 1
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("t_max", np.float32), ("d", np.float32, 3), ("pad", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("kind", np.int32), ("prim", np.int32), ("mat", np.int32),
                      ("n", np.float32, 4), ("p", np.float32, 4)])


def make_rays(o, d, t_max=np.inf):
    """n rays as a RAY_DTYPE array from (n, 3) origins and directions and a t_max (scalar or (n,))."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    r = np.zeros(len(o), RAY_DTYPE)
    r["o"], r["d"], r["t_max"] = o, np.asarray(d, np.float32).reshape(-1, 3), t_max
    return r


def _rays_in(rays):
    """Rays as a contiguous RAY_DTYPE array: structured already, or (n, 8) float32."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("rays must be a RAY_DTYPE array or (n, 8) float32")
    return a.view(RAY_DTYPE).reshape(-1)


def _xy_in(xy):
    a = np.ascontiguousarray(xy, np.int32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("xy must be (n, 2) pixel coordinates")
    return a


def hits_words(hits):
    """The (n, 12) uint32 words of a HIT_DTYPE array (for bit-for-bit comparisons)."""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 12)


def pixel_rays(width, height, cam, xy):
    """pt_pixel_rays: the PT_FLAG_NO_AA camera rays of the (n, 2) pixels xy (row 0 = bottom), on the host."""
    xy = _xy_in(xy)
    rays = np.zeros(len(xy), RAY_DTYPE)
    rc = lib().pt_pixel_rays(int(width), int(height), np.ascontiguousarray(cam, np.float32).reshape(12),
                             xy.ctypes.data, len(xy), rays.ctypes.data)
    if rc:
        raise PTError(rc, "pt_pixel_rays: bad size or arrays")
    return rays


def intersect_host(sb, rays, any_hit=False, flags=0):
    """pt_intersect_host: the ray query on the host (no device) -- the per-ray code is the device kernel's own,
    run on the buffers ptp::pack_scene makes of the scene `sb`.  flags: the PT_FLAG_* of a context."""
    rays = _rays_in(rays)
    hits = np.zeros(len(rays), HIT_DTYPE)
    t, n, m, s = _f32(sb["tris"], 16), _f32(sb["nodes"], 12), _f32(sb["mats"], 16), _f32(sb["spheres"], 8)
    z = lambda a, c: a.reshape(-1) if a.size else np.zeros(c, np.float32)
    rc = lib().pt_intersect_host(z(t, 16), len(t), z(n, 12), len(n), z(m, 16), len(m), z(s, 8), len(s), int(flags),
                                 rays.ctypes.data, len(rays), hits.ctypes.data, PT_QUERY_ANY_HIT if any_hit else 0)
    if rc:
        raise PTError(rc, "pt_intersect_host: rejected scene or bad arguments")
    return hits


# ----------------------------------------------------------------------------- traced rays
def _seeds_in(seeds, n):
    if seeds is None:
        return None
    s = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
    if len(s) != n:
        raise ValueError("one seed per ray")
    return s


def _prior_in(prior, n):
    """The in/out array of a trace: a copy of the prior, or NaNs a trace that overwrites never reads."""
    if prior is None:
        return np.full((n, 4), np.nan, np.float32)
    out = np.array(prior, np.float32).reshape(-1, 4)
    if len(out) != n:
        raise ValueError("one prior RGBA per ray")
    return out


def pixel_seeds(xy):
    """pt_pixel_seeds: the pixel part of the reference's seed, y * 831266 + x * 923766 (mod 2^32), of (n, 2) pixels."""
    xy = _xy_in(xy)
    seeds = np.zeros(len(xy), np.uint32)
    rc = lib().pt_pixel_seeds(xy.ctypes.data, len(xy), seeds.ctypes.data)
    if rc:
        raise PTError(rc, "pt_pixel_seeds: bad arrays")
    return seeds


def trace_host(sb, rays, seeds=None, frame_first=1, n_frames=1, prior=None, flags=0, max_bounce=5, mode=1):
    """pt_trace_host: traced rays on the host (no device) -- the per-ray code is the device kernel's own, run on the
    buffers ptp::pack_scene makes of the scene `sb`.  flags, max_bounce, mode: what a context would hold."""
    rays = _rays_in(rays)
    seeds = _seeds_in(seeds, len(rays))
    out = _prior_in(prior, len(rays))
    t, n, m, s = _f32(sb["tris"], 16), _f32(sb["nodes"], 12), _f32(sb["mats"], 16), _f32(sb["spheres"], 8)
    z = lambda a, c: a.reshape(-1) if a.size else np.zeros(c, np.float32)
    rc = lib().pt_trace_host(z(t, 16), len(t), z(n, 12), len(n), z(m, 16), len(m), z(s, 8), len(s), int(flags),
                             int(max_bounce), int(mode), rays.ctypes.data, None if seeds is None else seeds.ctypes.data,
                             len(rays), int(frame_first), int(n_frames), int(prior is not None), out.ctypes.data)
    if rc:
        raise PTError(rc, "pt_trace_host: rejected scene or bad arguments")
    return out


# ----------------------------------------------------------------------------- camera models
def camera_rays_host(camera, xy, frame=1):
    """pt_camera_rays_host: the Camera's rays of the (n, 2) pixels xy in frame `frame`, on the host -> (RAY_DTYPE
    rays, (n,) uint32 random states after the camera's draws)."""
    xy = _xy_in(xy)
    rays, states = np.zeros(len(xy), RAY_DTYPE), np.zeros(len(xy), np.uint32)
    rc = lib().pt_camera_rays_host(C.byref(camera), xy.ctypes.data, len(xy), int(frame), rays.ctypes.data,
                                   states.ctypes.data)
    if rc:
        raise PTError(rc, "pt_camera_rays_host: bad camera, frame or arrays")
    return rays, states


def trace_camera_host(sb, camera, frame_first=1, n_frames=1, prior=None, flags=0, max_bounce=5, mode=1):
    """pt_trace_camera_host: pt_trace_camera on the host (no device) -- the per-pixel code is the device kernel's own,
    run on the buffers ptp::pack_scene makes of the scene `sb` -> (height, width, 4) float32."""
    out = _prior_in(prior, camera.pixels)
    t, n, m, s = _f32(sb["tris"], 16), _f32(sb["nodes"], 12), _f32(sb["mats"], 16), _f32(sb["spheres"], 8)
    z = lambda a, c: a.reshape(-1) if a.size else np.zeros(c, np.float32)
    rc = lib().pt_trace_camera_host(z(t, 16), len(t), z(n, 12), len(n), z(m, 16), len(m), z(s, 8), len(s), int(flags),
                                    int(max_bounce), int(mode), C.byref(camera), int(frame_first), int(n_frames),
                                    int(prior is not None), out.ctypes.data)
    if rc:
        raise PTError(rc, "pt_trace_camera_host: rejected scene or bad arguments")
    return out.reshape(camera.height, camera.width, 4)


# ----------------------------------------------------------------------------- film
PT_FILM_IMAGE, PT_FILM_MOMENTS, PT_FILM_GUIDES, PT_FILM_DENOISED, PT_FILM_IMAGE_ACES8, PT_FILM_DENOISED_ACES8 = range(6)
FILM_PLANES = {"image": (PT_FILM_IMAGE, 4, np.float32), "moments": (PT_FILM_MOMENTS, 2, np.float32),
               "guides": (PT_FILM_GUIDES, 8, np.float32), "denoised": (PT_FILM_DENOISED, 4, np.float32),
               "image_aces8": (PT_FILM_IMAGE_ACES8, 4, np.uint8), "denoised_aces8": (PT_FILM_DENOISED_ACES8, 4, np.uint8)}


class Film:
    """pt_film (include/pt_api.h): the running image, luminance moments and first-hit guides of one
    Camera on one PathTracer, on the device.  Close it before its tracer."""

    def __init__(self, tracer, camera, guide_frames=4):
        self.pt, self.camera, self.guide_frames = tracer, camera, int(guide_frames)
        self.h = C.c_void_p()
        tracer._check(lib().pt_film_create(tracer.h, C.byref(camera), self.guide_frames, C.byref(self.h)))

    def _check(self, rc):
        self.pt._check(rc)

    def close(self):
        if self.h:
            lib().pt_film_destroy(self.h)
            self.h = C.c_void_p()

    def set_camera(self, camera):
        """Another Camera of the same size; the guides are gathered anew."""
        self._check(lib().pt_film_set_camera(self.h, C.byref(camera)))
        self.camera = camera

    def expose(self, frame_first=1, n_frames=1, accumulate_first=0):
        """pt_film_expose: enqueued on the tracer's stream, not waited for."""
        self._check(lib().pt_film_expose(self.h, int(frame_first), int(n_frames), int(accumulate_first)))

    def expose_until(self, target, batch=16, max_frames=1024, frame_first=1, accumulate_first=0):
        """pt_film_expose_until -> (frames_done, summary dict)."""
        done, s = C.c_int(), NoiseStats()
        self._check(lib().pt_film_expose_until(self.h, int(frame_first), int(accumulate_first), int(batch),
                                               int(max_frames), float(target), C.byref(done), C.byref(s)))
        return done.value, s.as_dict()

    def noise(self, target):
        """pt_film_noise: the integer noise summary of every pixel as a dict (NoiseStats.as_dict)."""
        s = NoiseStats()
        self._check(lib().pt_film_noise(self.h, float(target), C.byref(s)))
        return s.as_dict()

    def denoise(self, **params):
        """pt_film_denoise.  params: fields of pt_denoise_params over its defaults, guide_frames defaulting to the
        film's.  -> dict(guided, guides_rendered, iterations, frames)."""
        params.setdefault("guide_frames", self.guide_frames)
        p, info = denoise_params(**params), DenoiseInfo()
        self._check(lib().pt_film_denoise(self.h, C.byref(p), C.byref(info)))
        self.guide_frames = int(p.guide_frames)
        return dict(guided=bool(info.guided), guides_rendered=bool(info.guides_rendered),
                    iterations=int(info.iterations), frames=int(info.frames))

    def info(self):
        """-> (frames in the moments, guides_held)."""
        n, h = C.c_int(), C.c_int()
        self._check(lib().pt_film_info(self.h, C.byref(n), C.byref(h)))
        return n.value, h.value

    def read(self, what="image"):
        """pt_film_read of a plane of FILM_PLANES (a name or a PT_FILM_* value) -> (height, width, k) array."""
        if not isinstance(what, str):
            what = [k for k, v in FILM_PLANES.items() if v[0] == int(what)][0]
        code, k, dtype = FILM_PLANES[what]
        out = np.zeros((self.camera.height, self.camera.width, k), dtype)
        self._check(lib().pt_film_read(self.h, code, out.ctypes.data, out.nbytes))
        return out

    def device(self, what="image"):
        """pt_film_device -> (device pointer, bytes) of one of the planes image, moments, guides, denoised."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(lib().pt_film_device(self.h, FILM_PLANES[what][0], C.byref(p), C.byref(n)))
        return p.value, n.value


def film_expose_host(sb, camera, guide_frames, frame_first=1, n_frames=1, accumulate_first=0, state=None, flags=0,
                     max_bounce=5, mode=1):
    """pt_film_expose_host: an exposure on the host (no device) -- the per-pixel code is the device kernel's own.
    state: what an earlier call returned, or None for a new film -> dict(image (H, W, 4), moments (H, W, 2), guides
    (H, W, 8), frames, guides_held)."""
    h, w = camera.height, camera.width
    if state is None:
        state = dict(image=np.zeros((h, w, 4), np.float32), moments=np.zeros((h, w, 2), np.float32),
                     guides=np.zeros((h, w, 8), np.float32), frames=0, guides_held=0)
    img, mom, gd = (np.array(state[k], np.float32) for k in ("image", "moments", "guides"))
    t, n, m, s = _f32(sb["tris"], 16), _f32(sb["nodes"], 12), _f32(sb["mats"], 16), _f32(sb["spheres"], 8)
    z = lambda a, c: a.reshape(-1) if a.size else np.zeros(c, np.float32)
    held = C.c_int()
    rc = lib().pt_film_expose_host(z(t, 16), len(t), z(n, 12), len(n), z(m, 16), len(m), z(s, 8), len(s), int(flags),
                                   int(max_bounce), int(mode), C.byref(camera), int(guide_frames), int(frame_first),
                                   int(n_frames), int(accumulate_first), int(state["frames"]), int(state["guides_held"]),
                                   img.reshape(-1), mom.reshape(-1), gd.reshape(-1), C.byref(held))
    if rc:
        raise PTError(rc, "pt_film_expose_host: rejected scene or bad arguments")
    frames = state["frames"] + n_frames if accumulate_first else n_frames
    return dict(image=img, moments=mom, guides=gd, frames=frames, guides_held=held.value)


def noise_host(moments, frames, target, in_footprint=None):
    """pt_noise_host: the noise summary of (..., 2) float32 moments on the host (no device) -- the
    per-pixel function is the device kernel's own code.  in_footprint: one flag per pixel."""
    m = np.ascontiguousarray(moments, np.float32).reshape(-1)
    n = m.size // 2
    fp = None
    if in_footprint is not None:
        fp = np.ascontiguousarray(np.asarray(in_footprint).reshape(-1) != 0, np.uint8)
        if fp.size != n:
            raise ValueError("in_footprint must hold one flag per pixel")
    s = NoiseStats()
    rc = lib().pt_noise_host(m if n else np.zeros(2, np.float32), None if fp is None else fp.ctypes.data, n,
                             int(frames), float(target), C.byref(s))
    if rc:
        raise PTError(rc, "pt_noise_host: frames must be >= 2")
    return s.as_dict()


def denoise_host(image, variance, guides, in_footprint=None, **params):
    """pt_denoise_host: the denoising filter on the host (no device) -- the per-tap code is the
    device kernel's own.  image (H, W, 4), variance (H, W) of the mean luminance's variance or None
    (unguided), guides (H, W, 8) as PathTracer.read_guides, in_footprint (H, W) flags or None
    -> (H, W, 4) float32."""
    img = np.ascontiguousarray(image, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("image must be (H, W, 4)")
    h, w = img.shape[:2]
    g = np.ascontiguousarray(guides, np.float32)
    if g.shape != (h, w, 8):
        raise ValueError("guides must be (H, W, 8)")
    var = None
    if variance is not None:
        var = np.ascontiguousarray(variance, np.float32)
        if var.shape != (h, w):
            raise ValueError("variance must be (H, W)")
    fp = None
    if in_footprint is not None:
        fp = np.ascontiguousarray(np.asarray(in_footprint) != 0, np.uint8)
        if fp.shape != (h, w):
            raise ValueError("in_footprint must be (H, W)")
    out = np.zeros((h, w, 4), np.float32)
    p = denoise_params(**params)
    rc = lib().pt_denoise_host(img.reshape(-1), None if var is None else var.ctypes.data, g.reshape(-1),
                               None if fp is None else fp.ctypes.data, w, h, C.byref(p), out.reshape(-1))
    if rc:
        raise PTError(rc, "pt_denoise_host: iterations 1..8, guide_frames >= 1")
    return out


def tile_retires_host(moments, frames, target, in_footprint=None):
    """pt_tile_retires_host: whether a tile of these (..., 2) float32 moments retires after
    `frames` frames (the stop rule of render_adaptive, on the host; noise_host's arguments)."""
    m = np.ascontiguousarray(moments, np.float32).reshape(-1)
    n = m.size // 2
    fp = None
    if in_footprint is not None:
        fp = np.ascontiguousarray(np.asarray(in_footprint).reshape(-1) != 0, np.uint8)
        if fp.size != n:
            raise ValueError("in_footprint must hold one flag per pixel")
    r = C.c_int()
    rc = lib().pt_tile_retires_host(m if n else np.zeros(2, np.float32), None if fp is None else fp.ctypes.data, n,
                                    int(frames), float(target), C.byref(r))
    if rc:
        raise PTError(rc, "pt_tile_retires_host: frames must be >= 2")
    return bool(r.value)


def group_plan(devices, ranks):
    """pt_group_plan (host arithmetic, no device): -> dict(devices, dev_idx, slot, max_slots,
    table) for contexts on `devices` with image `ranks`."""
    n = len(devices)
    dev = np.ascontiguousarray(devices, np.int32)
    rk = np.ascontiguousarray(ranks, np.int32)
    devs, dev_idx, slot, table = (np.zeros(n, np.int32) for _ in range(4))
    nd, ms = C.c_int(0), C.c_int(0)
    rc = lib().pt_group_plan(dev, rk, n, devs, C.byref(nd), dev_idx, slot, C.byref(ms), table)
    if rc:
        raise PTError(rc, "pt_group_plan: ranks must be 0..n-1, each once")
    return dict(devices=devs[:nd.value].tolist(), dev_idx=dev_idx, slot=slot, max_slots=ms.value, table=table)


def group_interleave_host(blocks, table, world, width, height):
    """pt_group_interleave_host: the root's interleave of gathered row blocks on the host."""
    b = np.ascontiguousarray(blocks, np.float32)
    n_blocks = b.size // (max(1, -(-height // world)) * width * 4) if width and height else 0
    out = np.zeros((height, width, 4), np.float32)
    rc = lib().pt_group_interleave_host(b.reshape(-1), n_blocks, np.ascontiguousarray(table, np.int32), world,
                                        width, height, out.reshape(-1))
    if rc:
        raise PTError(rc, "pt_group_interleave_host: table entry outside the blocks")
    return out


def gather_rgba32f(tracers, device_ptr=None):
    """pt_gather_rgba32f: one-shot group + gather."""
    t0 = tracers[0]
    arr = (C.c_void_p * len(tracers))(*[t.h for t in tracers])
    nbytes = t0.width * t0.height * 16
    if device_ptr is not None:
        rc = lib().pt_gather_rgba32f(arr, len(tracers), C.c_void_p(device_ptr), nbytes, 1)
        if rc:
            raise PTError(rc, "pt_gather_rgba32f")
        return None
    out = np.zeros((t0.height, t0.width, 4), np.float32)
    rc = lib().pt_gather_rgba32f(arr, len(tracers), out.ctypes.data, nbytes, 0)
    if rc:
        raise PTError(rc, "pt_gather_rgba32f")
    return out


def assemble_rows(parts, height):
    """Interleave per-rank local rows (rank r owns rows r, r+G, ...) into a full image."""
    G = len(parts)
    W = parts[0].shape[1]
    img = np.zeros((height, W, 4), np.float32)
    for r, p in enumerate(parts):
        img[r::G][: len(p)] = p
    return img
