"""ctypes binding of libdistraytracer.so (include/distraytracer.h).

This is the product path: every render goes through the HIP kernels. There is
no CPU fallback -- if the library is missing or no GPU is visible the calls
raise RTError.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

from . import build as _build
from .scenes import SCENE_DIR, prepare

ST_NAMES = ["camera", "shadow", "refl", "refr", "box", "tri", "quad", "implicit", "light", "photon", "texel",
            "node", "leaf", "member", "root", "top",
            # the same record loads counted per wave step where a wave loads a record once for all
            # its lanes (RT_ST_W_*, include/distraytracer.h)
            "w_node", "w_tri", "w_quad", "w_implicit", "w_light", "w_photon"]
RT_ST_N = 24
INFO_NAMES = ["objects", "lights", "bvh_internal", "bvh_leaves", "bvh_depth", "bvh_prims", "prims",
              "rays_per_pixel", "device_bytes", "triangles", "photons", "materials", "photon_mode",
              "photon_count"]


class RTError(RuntimeError):
    pass


class TextureDesc(ctypes.Structure):
    _fields_ = [("w", ctypes.c_int32), ("h", ctypes.c_int32), ("rgb", ctypes.c_void_p)]


class RenderParams(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp", ctypes.c_int32),
                ("row0", ctypes.c_int32), ("row1", ctypes.c_int32), ("row_step", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("row_band", ctypes.c_int32)]


EXPORTS = ["rt_abi_version", "rt_build_id", "rt_last_error", "rt_device_count", "rt_scene_create", "rt_scene_load_cli",
           "rt_scene_inspect_cli",
           "rt_scene_info", "rt_scene_destroy", "rt_photons_build", "rt_render", "rt_render_device",
           "rt_render_count", "rt_time_render", "rt_render_pass", "rt_refine_steps", "rt_scene_photons",
           "rt_scene_photon_map", "rt_photons_shoot",
           "rt_photons_set",
           "rt_png_name", "rt_scene_save_name", "rt_math_eval", "rt_tile_layout", "rt_tile_costs",
           "rt_render_tiles_device", "rt_render_tiles_count",
           "rt_render_pixels_device", "rt_photon_gather",
           "rt_photon_kdtree", "rt_scene_photon_kdtree",
           # ABI 6: the multi-GPU frame (rt_group_*), the kernel variants
           "rt_render_variant", "rt_rank_plan", "rt_group_unique_id", "rt_group_create", "rt_group_create_rank", "rt_group_render",
           "rt_group_sync", "rt_group_render_host", "rt_group_frame", "rt_group_info", "rt_group_plan",
           "rt_group_rank_pixels", "rt_group_kernel_ms", "rt_group_time_rank", "rt_group_count", "rt_group_rebalance",
           "rt_group_destroy", "rt_group_rccl_selftest",
           # ABI 7: communicators (RCCL / caller host transport), the group and the photon pre-pass over them
           "rt_comm_create_rccl", "rt_comm_create_host", "rt_comm_info", "rt_comm_destroy", "rt_comm_selftest",
           "rt_group_create_comm",
           "rt_photons_build_comm", "rt_photons_build_local",
           # added to ABI 7: ray queries (closest hit / occlusion of caller rays)
           "rt_trace_rays", "rt_trace_rays_device",
           # added to ABI 7: the coherence order of RT_TRACE_SORT
           "rt_trace_order", "rt_trace_order_device",
           # added to ABI 7: radiance queries (the shading tree on caller rays) and a frame's camera rays
           "rt_shade_rays", "rt_shade_rays_device", "rt_camera_rays", "rt_camera_rays_device",
           # added to ABI 7: progressive sample accumulation (a frame that converges in place)
           "rt_accum_create", "rt_accum_add", "rt_accum_samples", "rt_accum_resolve", "rt_accum_resolve_device",
           "rt_accum_error", "rt_accum_error_device", "rt_accum_state", "rt_accum_restore", "rt_accum_reset",
           "rt_accum_destroy",
           # added to ABI 7: adaptive sampling (per-pixel sample counts, selections, the selective add)
           "rt_accum_select_error", "rt_accum_select_mask", "rt_accum_select_mask_device", "rt_accum_selection",
           "rt_accum_add_selected", "rt_accum_counts", "rt_accum_counts_device", "rt_accum_restore_counts",
           # added to ABI 7: the variance-guided a-trous denoiser of an accumulated frame
           "rt_denoise_defaults", "rt_denoise_create", "rt_denoise_guides", "rt_denoise_run", "rt_denoise_run_device",
           "rt_denoise_planes", "rt_denoise_destroy",
           # added to ABI 7: the camera pose (the eye moved over the scene as uploaded)
           "rt_camera_pose_check", "rt_camera_look_at", "rt_camera_rays_pose", "rt_camera_rays_pose_device",
           "rt_accum_set_camera", "rt_accum_camera", "rt_denoise_rebuild"]

_lib = None


def lib_path() -> Path:
    """The in-tree library; DISTRAYTRACER_LIB overrides it (tuning builds, tools/variant_sweep.py)."""
    env = os.environ.get("DISTRAYTRACER_LIB")
    return Path(env) if env else _build.LIB_PATH


def lib():
    """Load the HIP library; raises RTError (never falls back) if it is absent."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: PyTorch ships its own libamdhip64 (soname libamdhip64.so.7,
        # loaded by file name), and a process that loads ours (/opt/rocm's, same soname) first and
        # torch's later holds two runtimes, the second of which sees no GPU. With torch imported
        # first the library binds to the runtime already loaded (the soname matches).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        p = lib_path()
        if not p.exists():
            raise RTError(f"{p} is missing: build it with `python -m distraytracer_old_amd.build`")
        L = ctypes.CDLL(str(p))
        L.rt_last_error.restype = ctypes.c_char_p
        if hasattr(L, "rt_build_id"):  # ABI >= 5 (older tuning builds lack it: build_id() -> "unknown")
            L.rt_build_id.restype = ctypes.c_char_p
        L.rt_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.rt_scene_load_cli.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(TextureDesc),
                                        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.rt_scene_inspect_cli.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(TextureDesc),
                                           ctypes.c_void_p, ctypes.c_int]
        L.rt_scene_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.rt_scene_destroy.argtypes = [ctypes.c_void_p]
        L.rt_photons_build.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.rt_scene_photons.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.POINTER(ctypes.c_int64)]
        L.rt_scene_photon_map.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int32)]
        L.rt_photons_shoot.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        L.rt_refine_steps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.rt_render_pass.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_int, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p]
        L.rt_photons_set.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.rt_render.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p, ctypes.c_void_p]
        L.rt_render_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
        L.rt_render_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]
        L.rt_time_render.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_double)]
        L.rt_tile_layout.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p]
        L.rt_tile_costs.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p, ctypes.c_int]
        L.rt_render_tiles_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.rt_render_pixels_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.rt_render_tiles_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(RenderParams), ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_void_p]
        L.rt_photon_kdtree.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        L.rt_scene_photon_kdtree.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.rt_photon_gather.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.rt_math_eval.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]
        L.rt_png_name.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
        L.rt_scene_save_name.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
        if hasattr(L, "rt_group_create"):  # ABI >= 6
            vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
            L.rt_rank_plan.argtypes = [vp, vp, i32, i32, dbl, i32, vp, vp]
            L.rt_group_rebalance.argtypes = [vp, i32, i32, vp]
            L.rt_render_variant.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                            ctypes.POINTER(ctypes.c_uint32)]
            L.rt_group_unique_id.argtypes = [vp, i32]
            L.rt_group_create.argtypes = [vp, i32, ctypes.POINTER(RenderParams), ctypes.c_uint32, dbl, i32,
                                          ctypes.POINTER(vp)]
            L.rt_group_create_rank.argtypes = [vp, i32, i32, vp, ctypes.POINTER(RenderParams), ctypes.c_uint32, dbl,
                                               i32, ctypes.POINTER(vp)]
            L.rt_group_render.argtypes = [vp, vp, vp]
            L.rt_group_sync.argtypes = [vp]
            L.rt_group_render_host.argtypes = [vp, vp, vp]
            L.rt_group_frame.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
            L.rt_group_info.argtypes = [vp, vp, i32]
            L.rt_group_plan.argtypes = [vp, vp, vp, i32]
            L.rt_group_rank_pixels.argtypes = [vp, i32, vp, i64]
            L.rt_group_kernel_ms.argtypes = [vp, i32, ctypes.POINTER(dbl), ctypes.POINTER(i32)]
            L.rt_group_time_rank.argtypes = [vp, i32, i32, i32, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
            L.rt_group_count.argtypes = [vp, i32, vp]
            L.rt_group_destroy.argtypes = [vp]
            L.rt_group_destroy.restype = None
            L.rt_group_rccl_selftest.argtypes = [i32, i32]
        if hasattr(L, "rt_comm_create_host"):  # ABI >= 7
            vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
            L.rt_comm_create_rccl.argtypes = [i32, i32, vp, i32, ctypes.POINTER(vp)]
            L.rt_comm_create_host.argtypes = [i32, i32, ctypes.POINTER(CommOps), ctypes.POINTER(vp)]
            L.rt_comm_info.argtypes = [vp, vp, i32]
            L.rt_comm_destroy.argtypes = [vp]
            L.rt_comm_destroy.restype = None
            L.rt_comm_selftest.argtypes = [vp, i32]
            L.rt_group_create_comm.argtypes = [vp, vp, ctypes.POINTER(RenderParams), ctypes.c_uint32, dbl, i32,
                                               ctypes.POINTER(vp)]
            L.rt_photons_build_comm.argtypes = [vp, vp, ctypes.c_uint64]
            L.rt_photons_build_local.argtypes = [vp, i32, ctypes.c_uint64]
        if hasattr(L, "rt_trace_rays"):  # added to ABI 7
            vp, i64 = ctypes.c_void_p, ctypes.c_int64
            L.rt_trace_rays.argtypes = [vp, vp, vp, i64, vp, vp]
            L.rt_trace_rays_device.argtypes = [vp, vp, vp, i64, vp, vp, vp]
        if hasattr(L, "rt_trace_order"):  # added to ABI 7
            vp, i64 = ctypes.c_void_p, ctypes.c_int64
            L.rt_trace_order.argtypes = [vp, vp, vp, i64, vp]
            L.rt_trace_order_device.argtypes = [vp, vp, vp, i64, vp, vp]
        if hasattr(L, "rt_shade_rays"):  # added to ABI 7
            vp, i64 = ctypes.c_void_p, ctypes.c_int64
            L.rt_shade_rays.argtypes = [vp, vp, vp, i64, vp, vp]
            L.rt_shade_rays_device.argtypes = [vp, vp, vp, i64, vp, vp, vp]
            L.rt_camera_rays.argtypes = [vp, vp, ctypes.c_int, vp]
            L.rt_camera_rays_device.argtypes = [vp, vp, ctypes.c_int, vp, vp]
        if hasattr(L, "rt_accum_create"):  # added to ABI 7
            vp, i64 = ctypes.c_void_p, ctypes.c_int64
            L.rt_accum_create.argtypes = [vp, vp, ctypes.c_uint32, vp]
            L.rt_accum_add.argtypes = [vp, ctypes.c_int, vp]
            L.rt_accum_samples.argtypes = [vp, vp]
            L.rt_accum_resolve.argtypes = [vp, vp, vp]
            L.rt_accum_resolve_device.argtypes = [vp, vp, vp, vp]
            L.rt_accum_error.argtypes = [vp, vp]
            L.rt_accum_error_device.argtypes = [vp, vp, vp]
            L.rt_accum_state.argtypes = [vp, vp, vp, vp]
            L.rt_accum_restore.argtypes = [vp, i64, vp, vp]
            L.rt_accum_reset.argtypes = [vp]
            L.rt_accum_destroy.argtypes = [vp]
            L.rt_accum_destroy.restype = None
        if hasattr(L, "rt_accum_add_selected"):  # added to ABI 7
            L.rt_accum_select_error.argtypes = [vp, ctypes.c_float, ctypes.c_int, vp]
            L.rt_accum_select_mask.argtypes = [vp, vp, vp]
            L.rt_accum_select_mask_device.argtypes = [vp, vp, vp, vp]
            L.rt_accum_selection.argtypes = [vp, vp]
            L.rt_accum_add_selected.argtypes = [vp, ctypes.c_int, vp]
            L.rt_accum_counts.argtypes = [vp, vp]
            L.rt_accum_counts_device.argtypes = [vp, vp, vp]
            L.rt_accum_restore_counts.argtypes = [vp, vp]
        if hasattr(L, "rt_denoise_run"):  # added to ABI 7
            L.rt_denoise_defaults.argtypes = [vp]
            L.rt_denoise_create.argtypes = [vp, vp]
            L.rt_denoise_guides.argtypes = [vp, vp, vp, vp, vp]
            L.rt_denoise_run.argtypes = [vp, vp, vp, vp]
            L.rt_denoise_run_device.argtypes = [vp, vp, vp, vp, vp]
            L.rt_denoise_planes.argtypes = [vp, vp, vp]
            L.rt_denoise_destroy.argtypes = [vp]
            L.rt_denoise_destroy.restype = None
        if hasattr(L, "rt_accum_set_camera"):  # added to ABI 7
            L.rt_camera_pose_check.argtypes = [vp]
            L.rt_camera_look_at.argtypes = [vp, vp, vp, vp]
            L.rt_camera_rays_pose.argtypes = [vp, vp, ctypes.c_int, vp, vp]
            L.rt_camera_rays_pose_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
            L.rt_accum_set_camera.argtypes = [vp, vp]
            L.rt_accum_camera.argtypes = [vp, vp, vp]
            L.rt_denoise_rebuild.argtypes = [vp]
        _lib = L
    return _lib


def _name_call(fn, *args) -> str:
    n = fn(*args, None, 0)
    if n < 0:
        raise RTError(f"{fn.__name__} failed ({n}): {lib().rt_last_error().decode()}")
    buf = ctypes.create_string_buffer(n + 1)
    fn(*args, buf, n + 1)
    return buf.value.decode()


def build_id() -> str:
    """The loaded library's build id (rt_build_id: hash of its sources and flags, build.py)."""
    return lib().rt_build_id().decode() if hasattr(lib(), "rt_build_id") else "unknown"


def png_name(save_name: str) -> str:
    """myScene.saveFile's image name for a `write` argument (myScene.java:1185-1196)."""
    return _name_call(lib().rt_png_name, save_name.encode())


def _check(rc: int, what: str):
    if rc != 0:
        raise RTError(f"{what} failed ({rc}): {lib().rt_last_error().decode()}")


def _pose(pose):
    """A pose argument as a contiguous float64 [16] (None stays None: no pose)."""
    if pose is None:
        return None
    m = np.ascontiguousarray(pose, dtype=np.float64)
    if m.size != 16:
        raise ValueError("a pose is a 4 x 4 matrix, row-major, camera -> world")
    return m.reshape(16)


def look_at(eye, target, up=(0, 1, 0)) -> np.ndarray:
    """The camera pose (float64 [4, 4], camera -> world) of an eye at `eye` that looks at `target` with `up`
    upwards (rt_camera_look_at)."""
    e, t, u = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    m = np.zeros(16, dtype=np.float64)
    _check(lib().rt_camera_look_at(e.ctypes.data, t.ctypes.data, u.ctypes.data, m.ctypes.data), "rt_camera_look_at")
    return m.reshape(4, 4)


def pose_check(pose) -> None:
    """Raises RTError unless `pose` is a valid camera pose: finite, last row 0 0 0 1, a proper rotation and a
    translation (rt_camera_pose_check)."""
    m = _pose(pose)
    _check(lib().rt_camera_pose_check(None if m is None else m.ctypes.data), "rt_camera_pose_check")


def math_eval(x, device: int = 0) -> np.ndarray:
    """Device fdlibm sin / cos / asin / acos of x (diagnostics, rt_math_eval): [n, 4] float64."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros((len(x), 4), dtype=np.float64)
    _check(lib().rt_math_eval(x.ctypes.data, out.ctypes.data, len(x), device), "rt_math_eval")
    return out


def photon_kdtree(pos) -> np.ndarray:
    """The reference's kd-tree over a photon_list (host-only, rt_photon_kdtree): int32 [n, 4] =
    (photon list index, axis, left, right) per node, DFS pre-order."""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(pos), 4), dtype=np.int32)
    _check(lib().rt_photon_kdtree(pos.ctypes.data, len(pos), out.ctypes.data), "rt_photon_kdtree")
    return out


def rank_plan(cost, world: int, heavy: float = 0.0, slots: int = 0, weight=None):
    """The deterministic multi-GPU plan of a layout's tile costs (rt_rank_plan, host only):
    (owner int32 [ntiles], order int32 [ntiles]) -- owner[t] in [0, world) renders tile t in its wave
    run, world + r marks one of rank r's split (one sample per wave) tiles; order = dispatch order.
    weight: per-tile cut factors (the runs hold equal sums of cost x weight)."""
    c = np.ascontiguousarray(cost, dtype=np.uint32)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    if w is not None and w.shape != c.shape:  # the C side reads weight[t] for every tile
        raise ValueError(f"rank_plan: weight has {w.size} entries, cost {c.size}")
    owner = np.zeros(len(c), dtype=np.int32)
    order = np.zeros(len(c), dtype=np.int32)
    _check(lib().rt_rank_plan(c.ctypes.data, None if w is None else w.ctypes.data, len(c), world, heavy, slots,
                              owner.ctypes.data, order.ctypes.data), "rt_rank_plan")
    return owner, order


def group_unique_id() -> bytes:
    """128-byte RCCL unique id for rt_group_create_rank (call on rank 0, share with the others)."""
    buf = ctypes.create_string_buffer(128)
    n = lib().rt_group_unique_id(buf, 128)
    if n < 0:
        raise RTError(f"rt_group_unique_id failed ({n}): {lib().rt_last_error().decode()}")
    return buf.raw[:n]


def rccl_selftest(device: int = 0, n: int = 4099) -> None:
    """rt_group_rccl_selftest: every RCCL call of the group's transport through a one-rank
    communicator on `device` (bindings check for one-GPU machines); raises RTError on a failure."""
    _check(lib().rt_group_rccl_selftest(device, n), "rt_group_rccl_selftest")


GROUP_RGB = 1  # RT_GROUP_RGB: exchange the float-RGB plane too
GROUP_COPY = 2  # RT_GROUP_COPY: device copies in one process (ranks may share a device)
GROUP_INFO = ["world", "local_ranks", "first_rank", "ntiles", "tiles_x", "tw", "th", "rccl", "frames", "plan_checks"]
TRANSPORT_NAMES = {0: "copy", 1: "rccl", 2: "host"}

# rt_comm_ops (include/distraytracer.h): the host transport's four blocking callbacks
_BCAST = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int)
_ALLGATHER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
_SEND = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int)
_RECV = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int)


class CommOps(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("bcast", _BCAST), ("allgather", _ALLGATHER), ("send", _SEND),
                ("recv", _RECV)]


def _host_bytes(addr: int, n: int):
    """A writable uint8 torch view of n host bytes at addr (no copy)."""
    import torch

    return torch.frombuffer((ctypes.c_uint8 * n).from_address(addr), dtype=torch.uint8)


class Comm:
    """A communicator (rt_comm_*): RCCL (`rccl`) or the host transport (`host`) whose collectives
    are torch.distributed calls on CPU tensors (gloo) -- the caller's-own-transport path, which lets
    the ranks of one-process-per-GPU groups share a device."""

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep  # the callbacks (ctypes must keep them alive while the library may call them)

    @classmethod
    def rccl(cls, rank: int, world: int, uid, device: int) -> "Comm":
        h = ctypes.c_void_p()
        u = ctypes.create_string_buffer(bytes(uid), 128) if uid is not None else None
        _check(lib().rt_comm_create_rccl(rank, world, u, device, ctypes.byref(h)), "rt_comm_create_rccl")
        return cls(h)

    @classmethod
    def host(cls, dist, group=None) -> "Comm":
        """Host transport over an initialised torch.distributed process group (gloo: CPU tensors)."""
        import torch

        rank, world = dist.get_rank(group), dist.get_world_size(group)
        errors = []

        def guard(fn):
            def call(*a):
                try:
                    fn(*a)
                    return 0
                except Exception as e:  # reported as RT_E_HIP by the library; the message kept here
                    errors.append(repr(e))
                    return 1
            return call

        def bcast(_ctx, buf, n, root):
            dist.broadcast(_host_bytes(buf, n), root, group=group)

        def allgather(_ctx, inp, out, n):
            src = _host_bytes(inp, n).clone()
            outs = [torch.empty(n, dtype=torch.uint8) for _ in range(world)]
            dist.all_gather(outs, src, group=group)
            _host_bytes(out, n * world).copy_(torch.cat(outs))

        def send(_ctx, buf, n, peer):
            dist.send(_host_bytes(buf, n).clone(), peer, group=group)

        def recv(_ctx, buf, n, peer):
            t = torch.empty(n, dtype=torch.uint8)
            dist.recv(t, peer, group=group)
            _host_bytes(buf, n).copy_(t)

        cbs = (_BCAST(guard(bcast)), _ALLGATHER(guard(allgather)), _SEND(guard(send)), _RECV(guard(recv)))
        ops = CommOps(None, *cbs)
        h = ctypes.c_void_p()
        _check(lib().rt_comm_create_host(rank, world, ctypes.byref(ops), ctypes.byref(h)), "rt_comm_create_host")
        c = cls(h, (cbs, ops))
        c.errors = errors
        return c

    def selftest(self, n: int = 1031):
        """rt_comm_selftest: all-gather, a broadcast from every rank and (host transport) the group's
        send / receive pattern, checked on the host (collective). Raises RTError on a failure."""
        rc = lib().rt_comm_selftest(self._h, n)
        if rc != 0:
            extra = f" (callback errors: {self.errors})" if getattr(self, "errors", None) else ""
            raise RTError(f"rt_comm_selftest failed ({rc}): {lib().rt_last_error().decode()}{extra}")

    def info(self) -> dict:
        v = np.zeros(4, dtype=np.int64)
        _check(lib().rt_comm_info(self._h, v.ctypes.data, 4), "rt_comm_info")
        return {"rank": int(v[0]), "world": int(v[1]), "transport": TRANSPORT_NAMES.get(int(v[2]), "?"),
                "device": int(v[3])}

    def close(self):
        if self._h:
            lib().rt_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def build_photons_local(scenes, seed: int):
    """rt_photons_build_local: the sharded photon pre-pass emulated in one process (scene q shoots
    shard q of len(scenes); scenes may repeat); every distinct scene gets the merged map."""
    arr = (ctypes.c_void_p * len(scenes))(*[s._h for s in scenes])
    _check(lib().rt_photons_build_local(arr, len(scenes), seed), "rt_photons_build_local")


class Group:
    """A multi-GPU frame (rt_group_*): one process driving N ranks (`create`) or one rank per
    process (`create_rank`). render() enqueues a frame; rank 0's frame lands in its own device
    buffers (frame()) or in caller-owned ones."""

    def __init__(self, handle, scenes):
        self._h = handle
        self._scenes = scenes  # keep the scenes alive while the group uses them

    @classmethod
    def create(cls, scenes, W, H, spp=0, seed=0x5EED0001, flags=0, rgb=False, copy=False, heavy=0.0, slots=0):
        p = params(W, H, spp, seed, None, 1, flags, 1)
        arr = (ctypes.c_void_p * len(scenes))(*[s._h for s in scenes])
        h = ctypes.c_void_p()
        gf = (GROUP_RGB if rgb else 0) | (GROUP_COPY if copy else 0)
        _check(lib().rt_group_create(arr, len(scenes), ctypes.byref(p), gf, heavy, slots, ctypes.byref(h)),
               "rt_group_create")
        return cls(h, list(scenes))

    @classmethod
    def create_comm(cls, scene, comm, W, H, spp=0, seed=0x5EED0001, flags=0, rgb=False, heavy=0.0, slots=0):
        """One rank of a one-process-per-GPU group over a communicator (rt_group_create_comm; collective).
        comm None: a one-rank group."""
        p = params(W, H, spp, seed, None, 1, flags, 1)
        h = ctypes.c_void_p()
        _check(lib().rt_group_create_comm(scene._h, comm._h if comm is not None else None, ctypes.byref(p),
                                          GROUP_RGB if rgb else 0, heavy, slots, ctypes.byref(h)),
               "rt_group_create_comm")
        return cls(h, [scene, comm])

    @classmethod
    def create_rank(cls, scene, rank, world, uid, W, H, spp=0, seed=0x5EED0001, flags=0, rgb=False, heavy=0.0,
                    slots=0):
        p = params(W, H, spp, seed, None, 1, flags, 1)
        h = ctypes.c_void_p()
        u = ctypes.create_string_buffer(bytes(uid), 128) if uid is not None else None
        _check(lib().rt_group_create_rank(scene._h, rank, world, u, ctypes.byref(p), GROUP_RGB if rgb else 0, heavy,
                                          slots, ctypes.byref(h)), "rt_group_create_rank")
        return cls(h, [scene])

    def render(self, rgb_ptr: int = 0, argb_ptr: int = 0):
        _check(lib().rt_group_render(self._h, ctypes.c_void_p(rgb_ptr or None), ctypes.c_void_p(argb_ptr or None)),
               "rt_group_render")

    def sync(self):
        _check(lib().rt_group_sync(self._h), "rt_group_sync")

    def render_host(self, W, H, rgb=True):
        """Blocking frame into host arrays (rank 0's process): (rgb [H, W, 3] float32 or None, argb [H, W])."""
        a = np.zeros((H, W), dtype=np.int32)
        c = np.zeros((H, W, 3), dtype=np.float32) if rgb else None
        _check(lib().rt_group_render_host(self._h, c.ctypes.data if rgb else None, a.ctypes.data),
               "rt_group_render_host")
        return c, a

    def frame(self):
        """Device pointers (rgb or 0, argb) of the group's own frame on rank 0's device."""
        r, a = ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().rt_group_frame(self._h, ctypes.byref(r), ctypes.byref(a)), "rt_group_frame")
        return r.value or 0, a.value or 0

    def info(self) -> dict:
        v = np.zeros(len(GROUP_INFO), dtype=np.int64)
        _check(lib().rt_group_info(self._h, v.ctypes.data, len(v)), "rt_group_info")
        return dict(zip(GROUP_INFO, v.tolist()))

    def plan(self):
        n = self.info()["ntiles"]
        owner = np.zeros(n, dtype=np.int32)
        order = np.zeros(n, dtype=np.int32)
        r = lib().rt_group_plan(self._h, owner.ctypes.data, order.ctypes.data, n)
        if r < 0:
            raise RTError(f"rt_group_plan: {lib().rt_last_error().decode()}")
        return owner, order

    def rank_tiles(self, rank: int):
        """(run tiles, split tiles) of a rank in dispatch order."""
        owner, order = self.plan()
        world = self.info()["world"]
        o = owner[order]
        return order[o == rank], order[o == world + rank]

    def rank_pixels(self, rank: int) -> np.ndarray:
        n = lib().rt_group_rank_pixels(self._h, rank, None, 0)
        if n < 0:
            raise RTError(f"rt_group_rank_pixels: {lib().rt_last_error().decode()}")
        out = np.zeros(n, dtype=np.int32)
        lib().rt_group_rank_pixels(self._h, rank, out.ctypes.data, n)
        return out

    def kernel_ms(self, rank: int):
        ms, fr = ctypes.c_double(0), ctypes.c_int(0)
        _check(lib().rt_group_kernel_ms(self._h, rank, ctypes.byref(ms), ctypes.byref(fr)), "rt_group_kernel_ms")
        return ms.value, fr.value

    def time_rank(self, rank: int, warmup: int = 3, iters: int = 20):
        """(wall ms per step, mean render ms) of one rank's pipelined step alone (RT_GROUP_COPY groups)."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        _check(lib().rt_group_time_rank(self._h, rank, warmup, iters, ctypes.byref(a), ctypes.byref(b)),
               "rt_group_time_rank")
        return a.value, b.value

    def rebalance(self, rounds: int = 2, iters: int = 5):
        """Re-cut the plan from measured rank render times (rt_group_rebalance; collective in rank
        mode); returns the ranks' render ms after the last cut."""
        out = np.zeros(self.info()["world"], dtype=np.float64)
        _check(lib().rt_group_rebalance(self._h, rounds, iters, out.ctypes.data), "rt_group_rebalance")
        return out

    def count(self, rank: int) -> dict:
        st = np.zeros(RT_ST_N, dtype=np.uint64)
        _check(lib().rt_group_count(self._h, rank, st.ctypes.data), "rt_group_count")
        return dict(zip(ST_NAMES, st[: len(ST_NAMES)].tolist()))

    def close(self):
        if self._h:
            lib().rt_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(lib().rt_device_count(ctypes.byref(n)), "rt_device_count")
    return n.value


def _tex_args(textures: dict):
    names = list(textures)
    arrs = [np.ascontiguousarray(textures[n], dtype=np.uint8) for n in names]
    cnames = (ctypes.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
    tds = (TextureDesc * max(1, len(names)))(*[TextureDesc(a.shape[1], a.shape[0], a.ctypes.data) for a in arrs])
    return names, arrs, cnames, tds


def inspect_cli(cli: str, scene_dir=SCENE_DIR, textures: dict | None = None) -> dict:
    """Host-only parse + flatten + BVH build (no GPU needed)."""
    if textures is None:
        textures = prepare(cli, Path(scene_dir))
    names, arrs, cnames, tds = _tex_args(textures)
    v = np.zeros(len(INFO_NAMES), dtype=np.int64)
    _check(lib().rt_scene_inspect_cli(str(scene_dir).encode(), cli.encode(), len(names), cnames, tds,
                                      v.ctypes.data, len(INFO_NAMES)), "rt_scene_inspect_cli")
    return dict(zip(INFO_NAMES, v.tolist()))


RENDER_GENERIC = 1  # RT_RENDER_GENERIC: the all-features kernel instead of the scene-specialised one
RENDER_ROWMAJOR = 2  # RT_RENDER_ROWMAJOR: row-major tile dispatch instead of the longest-first schedule
RENDER_NOCULL = 4  # RT_RENDER_NOCULL: no bounding-sphere culling of top-level primitives
RENDER_SHCOMPACT = 8  # RT_RENDER_SHCOMPACT: a wave's shadow rays traced compacted (same image)
RENDER_NOWAVECULL = 16  # RT_RENDER_NOWAVECULL: no wave-level shadow candidate test (same image)
RENDER_WAVEFRONT = 32  # RT_RENDER_WAVEFRONT: level-synchronous shading (same image)
RENDER_PIXEL_WAVES = 64  # RT_RENDER_PIXEL_WAVES: one pixel per wave (same image)
ACCUM_MOMENTS = 1  # RT_ACCUM_MOMENTS: the accumulator also keeps the per-channel sums of squares (error map)
ACCUM_COUNTS = 4  # RT_ACCUM_COUNTS: the accumulator also keeps a sample count per pixel (adaptive sampling)


TRACE_ANY = 1  # RT_TRACE_ANY: occlusion (calcShadow) instead of the closest hit
TRACE_LANES = 2  # RT_TRACE_LANES: per-lane reference-order traversal, all fp64
TRACE_NOCULL = 4  # RT_TRACE_NOCULL: no bounding-sphere cull, no nearest-first order
TRACE_GENERIC = 8  # RT_TRACE_GENERIC: the all-features instantiation
TRACE_SORT = 16  # RT_TRACE_SORT: rays reordered for coherence on the device, records at their own indices
HIT_HIT, HIT_INSTANCE, HIT_IN_ACCEL, HIT_BAD_RAY = 1, 2, 4, 8  # RT_HIT_*


def rays(o, d, tmax=np.inf) -> np.ndarray:
    """rt_ray array (desc.RAY_DTYPE) of origins o [n, 3], directions d [n, 3] and tmax (scalar or [n])."""
    from .desc import RAY_DTYPE

    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    r = np.zeros(len(o), dtype=RAY_DTYPE)
    r["o"] = o
    r["d"] = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    r["tmax"] = tmax
    return r


def params(W, H, spp=0, seed=0x5EED0001, rows=None, row_step=1, flags=0, row_band=1) -> RenderParams:
    r0, r1 = (0, H) if rows is None else rows
    return RenderParams(W, H, spp, r0, r1, row_step, seed, flags, row_band)


def nrows_of(p: RenderParams) -> int:
    """Rows row0 + k*row_step*row_band + j (0 <= j < row_band) below row1."""
    r1 = p.row1 if p.row1 > 0 else p.height
    step, band = max(1, p.row_step), max(1, p.row_band)
    full, rest = divmod(r1 - p.row0, step * band)
    return full * band + min(rest, band)


class Scene:
    """A scene resident on one GPU (rt_scene*)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load_cli(cls, cli: str, scene_dir=SCENE_DIR, textures: dict | None = None, device: int = 0) -> "Scene":
        if textures is None:
            textures = prepare(cli, Path(scene_dir))
        names, arrs, cnames, tds = _tex_args(textures)
        h = ctypes.c_void_p()
        _check(lib().rt_scene_load_cli(str(scene_dir).encode(), cli.encode(), len(names), cnames, tds, device,
                                       ctypes.byref(h)), "rt_scene_load_cli")
        return cls(h)

    def info(self) -> dict:
        v = np.zeros(len(INFO_NAMES), dtype=np.int64)
        _check(lib().rt_scene_info(self._h, v.ctypes.data, len(INFO_NAMES)), "rt_scene_info")
        return dict(zip(INFO_NAMES, v.tolist()))

    def save_name(self) -> str:
        """PNG name of the scene's `write` command (rt_scene_save_name)."""
        return _name_call(lib().rt_scene_save_name, self._h)

    def build_photons(self, seed: int):
        _check(lib().rt_photons_build(self._h, seed), "rt_photons_build")

    def build_photons_comm(self, comm, seed: int):
        """The photon pre-pass sharded over a communicator's ranks (rt_photons_build_comm; collective)."""
        _check(lib().rt_photons_build_comm(self._h, comm._h if comm is not None else None, seed),
               "rt_photons_build_comm")

    def shoot_photons(self, seed: int, first: int, count: int):
        """Photon shard [first, first+count) of every light -> (pos, pwr, per_light counts)."""
        nl = self.info()["lights"]
        per = np.zeros(max(1, nl), dtype=np.int64)
        _check(lib().rt_photons_shoot(self._h, seed, first, count, per.ctypes.data), "rt_photons_shoot")
        pos, pwr = self.photons()
        return pos, pwr, per[:nl]

    def set_photons(self, pos, pwr):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        pwr = np.ascontiguousarray(pwr, dtype=np.float64)
        _check(lib().rt_photons_set(self._h, pos.ctypes.data, pwr.ctypes.data, len(pos)), "rt_photons_set")

    def photon_map(self):
        """The device photon map: (nodes as raw uint8 [n_nodes, 128], root, ppos [n,3], ppwr [n,3])."""
        nn = ctypes.c_int64(0)
        root = ctypes.c_int32(0)
        _check(lib().rt_scene_photon_map(self._h, None, 0, None, None, 0, ctypes.byref(nn), ctypes.byref(root)),
               "rt_scene_photon_map")
        n = self.info()["photons"]
        nodes = np.zeros((nn.value, 128), dtype=np.uint8)
        ppos = np.zeros((n, 3)); ppwr = np.zeros((n, 3))
        _check(lib().rt_scene_photon_map(self._h, nodes.ctypes.data, nn.value, ppos.ctypes.data, ppwr.ctypes.data, n,
                                         ctypes.byref(nn), ctypes.byref(root)), "rt_scene_photon_map")
        return nodes, root.value, ppos, ppwr

    def photons(self):
        """(pos [n,3], pwr [n,3]) of the photon map in photon_list insertion order."""
        cnt = ctypes.c_int64(0)
        _check(lib().rt_scene_photons(self._h, None, None, 0, ctypes.byref(cnt)), "rt_scene_photons")
        n = cnt.value
        pos = np.zeros((n, 3)); pwr = np.zeros((n, 3))
        _check(lib().rt_scene_photons(self._h, pos.ctypes.data, pwr.ctypes.data, n, ctypes.byref(cnt)), "rt_scene_photons")
        return pos, pwr

    def render(self, W, H, spp=0, seed=0x5EED0001, rows=None, row_step=1, flags=0, row_band=1):
        p = params(W, H, spp, seed, rows, row_step, flags, row_band)
        n = nrows_of(p)
        rgb = np.zeros((n, W, 3), dtype=np.float32)
        argb = np.zeros((n, W), dtype=np.int32)
        _check(lib().rt_render(self._h, ctypes.byref(p), rgb.ctypes.data, argb.ctypes.data), "rt_render")
        return rgb, argb

    def render_argb_into(self, argb, W, H, spp=0, seed=0x5EED0001, flags=0):
        """The JNI draw() call: rt_render of the whole frame into a caller-owned
        host ARGB buffer (rndrdImg.pixels), no float plane; blocks until the pixels are there."""
        p = params(W, H, spp, seed, None, 1, flags, 1)
        assert argb.shape == (H, W) and argb.dtype == np.int32 and argb.flags.c_contiguous
        _check(lib().rt_render(self._h, ctypes.byref(p), None, argb.ctypes.data), "rt_render")

    def refine_steps(self, W, H) -> list[int]:
        """The `refine on` pass steps of a W x H render (myScene.setRefine); [1] without refine."""
        buf = np.zeros(16, dtype=np.int32)
        n = lib().rt_refine_steps(self._h, W, H, buf.ctypes.data, 16)
        if n < 0:
            raise RTError(f"rt_refine_steps: {lib().rt_last_error().decode()}")
        return buf[:n].tolist()

    def render_pass(self, W, H, step, skip_origin, rgb, argb, spp=0, seed=0x5EED0001, flags=0):
        """One refine pass into full-size host buffers rgb [H, W, 3] float32 / argb [H, W] int32 (in place)."""
        p = params(W, H, spp, seed, None, 1, flags, 1)
        assert rgb.shape == (H, W, 3) and rgb.dtype == np.float32 and rgb.flags.c_contiguous
        assert argb.shape == (H, W) and argb.dtype == np.int32 and argb.flags.c_contiguous
        _check(lib().rt_render_pass(self._h, ctypes.byref(p), step, int(bool(skip_origin)), rgb.ctypes.data,
                                    argb.ctypes.data), "rt_render_pass")

    def render_count(self, W, H, spp=0, seed=0x5EED0001, rows=None, row_step=1, row_band=1, flags=0):
        p = params(W, H, spp, seed, rows, row_step, flags, row_band)
        n = nrows_of(p)
        rgb = np.zeros((n, W, 3), dtype=np.float32)
        argb = np.zeros((n, W), dtype=np.int32)
        st = np.zeros(RT_ST_N, dtype=np.uint64)
        _check(lib().rt_render_count(self._h, ctypes.byref(p), rgb.ctypes.data, argb.ctypes.data, st.ctypes.data),
               "rt_render_count")
        return rgb, argb, dict(zip(ST_NAMES, st[: len(ST_NAMES)].tolist()))

    def variant(self, flags: int = 0) -> tuple[int, int]:
        """(timed, counted) feature masks F of the render_kernel<CNT, F> instantiations (rt_render_variant)."""
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().rt_render_variant(self._h, flags, ctypes.byref(a), ctypes.byref(b)), "rt_render_variant")
        return a.value, b.value

    def render_device(self, p: RenderParams, rgb_ptr: int, argb_ptr: int, stream: int = 0):
        """Asynchronous render into device buffers (e.g. torch tensors' data_ptr()) on a HIP stream."""
        _check(lib().rt_render_device(self._h, ctypes.byref(p), ctypes.c_void_p(rgb_ptr), ctypes.c_void_p(argb_ptr),
                                      ctypes.c_void_p(stream)), "rt_render_device")

    def tile_layout(self, p: RenderParams) -> tuple[int, int, int, int]:
        """(ntiles, tiles_x, tw, th) of a render layout (rt_tile_layout)."""
        out = np.zeros(4, dtype=np.int32)
        _check(lib().rt_tile_layout(self._h, ctypes.byref(p), out.ctypes.data), "rt_tile_layout")
        return tuple(int(x) for x in out)

    def tile_costs(self, p: RenderParams) -> np.ndarray:
        """Measured wave time of every tile of the layout (uint32 [ntiles]; calibrates if needed)."""
        n = self.tile_layout(p)[0]
        c = np.zeros(n, dtype=np.uint32)
        r = lib().rt_tile_costs(self._h, ctypes.byref(p), c.ctypes.data, n)
        if r < 0:
            raise RTError(f"rt_tile_costs failed ({r}): {lib().rt_last_error().decode()}")
        return c

    def render_tiles_device(self, p: RenderParams, tiles: np.ndarray, rgb_ptr: int, argb_ptr: int, stream: int = 0):
        """Asynchronous render of the listed tiles (host int32 list) into whole-layout device buffers."""
        t = np.ascontiguousarray(tiles, dtype=np.int32)
        _check(lib().rt_render_tiles_device(self._h, ctypes.byref(p), t.ctypes.data, len(t), ctypes.c_void_p(rgb_ptr),
                                            ctypes.c_void_p(argb_ptr), ctypes.c_void_p(stream)), "rt_render_tiles_device")

    def photon_kdtree(self) -> np.ndarray:
        """The device's copy of the reference's kd-tree: int32 [n, 4] (leaf-order photon, axis, left, right)."""
        n = self.info()["photons"]
        out = np.zeros((n, 4), dtype=np.int32)
        _check(lib().rt_scene_photon_kdtree(self._h, out.ctypes.data, n), "rt_scene_photon_kdtree")
        return out

    def photon_gather(self, pts) -> np.ndarray:
        """The render kernel's photon gather at points pts [n, 3] -> irradiance [n, 3] (rt_photon_gather)."""
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        out = np.zeros_like(pts)
        _check(lib().rt_photon_gather(self._h, pts.ctypes.data, out.ctypes.data, len(pts)), "rt_photon_gather")
        return out

    def trace(self, o, d, seed=0, first_key=0, flags=0) -> np.ndarray:
        """Closest hits of the rays (o [n, 3], d [n, 3]) -> structured array (desc.HIT_DTYPE) [n]
        (rt_trace_rays; flags: TRACE_LANES / TRACE_NOCULL / TRACE_GENERIC)."""
        from .desc import HIT_DTYPE, TraceParams

        r = rays(o, d)
        hits = np.zeros(len(r), dtype=HIT_DTYPE)
        p = TraceParams(seed, first_key, flags & ~TRACE_ANY, 0)
        _check(lib().rt_trace_rays(self._h, ctypes.byref(p), r.ctypes.data, len(r), hits.ctypes.data, None),
               "rt_trace_rays")
        return hits

    def occluded(self, o, d, tmax, seed=0, first_key=0, flags=0) -> np.ndarray:
        """calcShadow of the rays with dist = tmax (scalar or [n]; inf allowed) -> uint8 [n]: 1 blocked,
        0 free, 2 rejected ray (rt_trace_rays with RT_TRACE_ANY)."""
        from .desc import TraceParams

        r = rays(o, d, tmax)
        occ = np.zeros(len(r), dtype=np.uint8)
        p = TraceParams(seed, first_key, flags | TRACE_ANY, 0)
        _check(lib().rt_trace_rays(self._h, ctypes.byref(p), r.ctypes.data, len(r), None, occ.ctypes.data),
               "rt_trace_rays")
        return occ

    def trace_device(self, rays_ptr: int, n: int, hits_ptr: int = 0, occ_ptr: int = 0, stream: int = 0, seed=0,
                     first_key=0, flags=0):
        """Asynchronous trace of n device rt_ray (e.g. torch tensors' data_ptr()) into device rt_hit
        (closest hit) or uint8 (flags & TRACE_ANY) buffers on a HIP stream (rt_trace_rays_device)."""
        from .desc import TraceParams

        p = TraceParams(seed, first_key, flags, 0)
        _check(lib().rt_trace_rays_device(self._h, ctypes.byref(p), ctypes.c_void_p(rays_ptr or None), n,
                                          ctypes.c_void_p(hits_ptr or None), ctypes.c_void_p(occ_ptr or None),
                                          ctypes.c_void_p(stream or None)), "rt_trace_rays_device")

    def trace_order(self, o, d, tmax=np.inf, flags=0) -> np.ndarray:
        """The order a TRACE_SORT trace of the rays runs them in -> uint32 [n]: order[k] is the index of the
        ray in slot k, a permutation of each sort window's index range (rt_trace_order)."""
        from .desc import TraceParams

        r = rays(o, d, tmax)
        order = np.zeros(len(r), dtype=np.uint32)
        p = TraceParams(0, 0, flags, 0)
        _check(lib().rt_trace_order(self._h, ctypes.byref(p), r.ctypes.data, len(r), order.ctypes.data), "rt_trace_order")
        return order

    def trace_order_device(self, rays_ptr: int, n: int, order_ptr: int, stream: int = 0, flags=0):
        """Asynchronous rt_trace_order of n device rt_ray into a device uint32 [n] buffer on a HIP stream
        (rt_trace_order_device)."""
        from .desc import TraceParams

        p = TraceParams(0, 0, flags, 0)
        _check(lib().rt_trace_order_device(self._h, ctypes.byref(p), ctypes.c_void_p(rays_ptr or None), n,
                                           ctypes.c_void_p(order_ptr or None), ctypes.c_void_p(stream or None)),
               "rt_trace_order_device")

    def shade(self, o, d, seed=0, first_key=0, sample=0, flags=0, status=True):
        """The colour each ray (o [n, 3], d [n, 3]) sees -> (rgb float64 [n, 3], status uint8 [n]: 0 shaded,
        2 rejected ray with colour 0; None with status=False). Ray i is shaded under the key the render gives
        sample `sample` of pixel first_key + i (rt_shade_rays; flags: TRACE_NOCULL / TRACE_GENERIC / TRACE_SORT)."""
        from .desc import ShadeParams

        r = rays(o, d)
        rgb = np.zeros((len(r), 3), dtype=np.float64)
        st = np.zeros(len(r), dtype=np.uint8) if status else None
        p = ShadeParams(seed, first_key, flags, sample)
        _check(lib().rt_shade_rays(self._h, ctypes.byref(p), r.ctypes.data, len(r), rgb.ctypes.data,
                                   st.ctypes.data if status else None), "rt_shade_rays")
        return rgb, st

    def shade_device(self, rays_ptr: int, n: int, rgb_ptr: int, status_ptr: int = 0, stream: int = 0, seed=0,
                     first_key=0, sample=0, flags=0):
        """Asynchronous rt_shade_rays of n device rt_ray (e.g. torch tensors' data_ptr()) into a device
        float64 [n, 3] buffer and, if given, a uint8 [n] status buffer on a HIP stream (rt_shade_rays_device)."""
        from .desc import ShadeParams

        p = ShadeParams(seed, first_key, flags, sample)
        _check(lib().rt_shade_rays_device(self._h, ctypes.byref(p), ctypes.c_void_p(rays_ptr or None), n,
                                          ctypes.c_void_p(rgb_ptr or None), ctypes.c_void_p(status_ptr or None),
                                          ctypes.c_void_p(stream or None)), "rt_shade_rays_device")

    def camera_rays(self, W, H, spp=0, seed=0x5EED0001, sample=0, pose=None) -> np.ndarray:
        """The rays a W x H render at spp shoots for sample `sample` of every pixel -> desc.RAY_DTYPE [H * W],
        row-major: index = pixel key (rt_camera_rays). An untraced fisheye sample has d = 0. pose: a camera
        pose (look_at) applied to every ray (rt_camera_rays_pose)."""
        from .desc import RAY_DTYPE

        p = params(W, H, spp, seed)
        r = np.zeros(W * H, dtype=RAY_DTYPE)
        if pose is None:
            _check(lib().rt_camera_rays(self._h, ctypes.byref(p), sample, r.ctypes.data), "rt_camera_rays")
        else:
            _check(lib().rt_camera_rays_pose(self._h, ctypes.byref(p), sample, _pose(pose).ctypes.data, r.ctypes.data),
                   "rt_camera_rays_pose")
        return r

    def camera_rays_device(self, p: RenderParams, rays_ptr: int, sample: int = 0, stream: int = 0, pose=None):
        """Asynchronous rt_camera_rays into a device rt_ray [height * width] buffer on a HIP stream
        (rt_camera_rays_device; with a pose rt_camera_rays_pose_device)."""
        if pose is None:
            _check(lib().rt_camera_rays_device(self._h, ctypes.byref(p), sample, ctypes.c_void_p(rays_ptr or None),
                                               ctypes.c_void_p(stream or None)), "rt_camera_rays_device")
        else:
            _check(lib().rt_camera_rays_pose_device(self._h, ctypes.byref(p), sample, _pose(pose).ctypes.data,
                                                    ctypes.c_void_p(rays_ptr or None), ctypes.c_void_p(stream or None)),
                   "rt_camera_rays_pose_device")

    def accumulator(self, W, H, seed=0x5EED0001, flags=0, moments=False, counts=False, pose=None) -> "Accumulator":
        """A W x H frame that converges in place (rt_accum_create): samples are added in chunks and the frame
        so far resolved between them. flags: RENDER_GENERIC / RENDER_NOCULL; moments=True also keeps the sums
        of squares the error map needs, counts=True a sample count per pixel (select_* / add_selected); pose: the
        camera pose it starts with (Accumulator.set_camera)."""
        return Accumulator(self, W, H, seed, flags, moments, counts, pose)

    def render_pixels_device(self, p: RenderParams, pixels: np.ndarray, rgb_ptr: int, argb_ptr: int, stream: int = 0):
        """Asynchronous one-sample-per-wave render of the listed pixels (host int32 list) into whole-frame buffers."""
        t = np.ascontiguousarray(pixels, dtype=np.int32)
        _check(lib().rt_render_pixels_device(self._h, ctypes.byref(p), t.ctypes.data, len(t), ctypes.c_void_p(rgb_ptr),
                                             ctypes.c_void_p(argb_ptr), ctypes.c_void_p(stream)), "rt_render_pixels_device")

    def render_tiles_count(self, p: RenderParams, tiles: np.ndarray) -> dict:
        """Counters (rt_render_count's) of an instrumented render of the listed tiles only."""
        t = np.ascontiguousarray(tiles, dtype=np.int32)
        st = np.zeros(RT_ST_N, dtype=np.uint64)
        _check(lib().rt_render_tiles_count(self._h, ctypes.byref(p), t.ctypes.data, len(t), st.ctypes.data),
               "rt_render_tiles_count")
        return dict(zip(ST_NAMES, st[: len(ST_NAMES)].tolist()))

    def time_render(self, W, H, spp=0, seed=0x5EED0001, rows=None, row_step=1, warmup=1, iters=3, flags=0,
                    row_band=1) -> float:
        p = params(W, H, spp, seed, rows, row_step, flags, row_band)
        ms = ctypes.c_double(0)
        _check(lib().rt_time_render(self._h, ctypes.byref(p), warmup, iters, ctypes.byref(ms)), "rt_time_render")
        return ms.value

    def close(self):
        if self._h:
            lib().rt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Accumulator:
    """Progressive sample accumulation on one scene (rt_accum*): after add(n) calls that total N >= 2 samples,
    resolve() is Scene.render(spp=N) bit for bit, however the samples were cut into chunks. Holds a reference
    to its scene (an accumulator must be closed before its scene)."""

    def __init__(self, scene: Scene, W, H, seed=0x5EED0001, flags=0, moments=False, counts=False, pose=None):
        self._h, self._nsel = None, 0
        self.scene, self.W, self.H, self.moments, self.has_counts = scene, W, H, bool(moments), bool(counts)
        p = params(W, H, 0, seed, flags=flags)
        h = ctypes.c_void_p()
        _check(lib().rt_accum_create(scene._h, ctypes.byref(p), (ACCUM_MOMENTS if moments else 0) | (ACCUM_COUNTS if counts else 0),
                                     ctypes.byref(h)), "rt_accum_create")
        self._h = h
        if pose is not None:
            self.set_camera(pose)

    def set_camera(self, pose):
        """Look through another camera pose (look_at; None: the scene's own camera again) and start the frame
        over: everything reset() does, and every sample from now on is of the posed rays. The scene and its
        photon map are not touched (rt_accum_set_camera)."""
        m = _pose(pose)
        _check(lib().rt_accum_set_camera(self._h, None if m is None else m.ctypes.data), "rt_accum_set_camera")
        self._nsel = 0

    @property
    def camera(self):
        """The pose set_camera gave (float64 [4, 4]), None when there is none (rt_accum_camera)."""
        m = np.zeros(16, dtype=np.float64)
        on = ctypes.c_int(0)
        _check(lib().rt_accum_camera(self._h, m.ctypes.data, ctypes.byref(on)), "rt_accum_camera")
        return m.reshape(4, 4) if on.value else None

    def add(self, count: int, stream: int = 0):
        """Shade the next `count` samples of every pixel; asynchronous on `stream` (0: the scene's own)."""
        _check(lib().rt_accum_add(self._h, count, ctypes.c_void_p(stream or None)), "rt_accum_add")

    @property
    def samples(self) -> int:
        n = ctypes.c_int64(0)
        _check(lib().rt_accum_samples(self._h, ctypes.byref(n)), "rt_accum_samples")
        return n.value

    def resolve(self):
        """The frame of the samples so far -> (rgb float32 [H, W, 3], argb int32 [H, W]), as Scene.render."""
        rgb = np.zeros((self.H, self.W, 3), dtype=np.float32)
        argb = np.zeros((self.H, self.W), dtype=np.int32)
        _check(lib().rt_accum_resolve(self._h, rgb.ctypes.data, argb.ctypes.data), "rt_accum_resolve")
        return rgb, argb

    def resolve_device(self, rgb_ptr: int, argb_ptr: int, stream: int = 0):
        """resolve() into device buffers (either may be 0) on a HIP stream; the caller orders it against add."""
        _check(lib().rt_accum_resolve_device(self._h, ctypes.c_void_p(rgb_ptr or None), ctypes.c_void_p(argb_ptr or None),
                                             ctypes.c_void_p(stream or None)), "rt_accum_resolve_device")

    def error(self) -> np.ndarray:
        """The standard error of every pixel's mean, the largest of its channels -> float32 [H, W] (moments only)."""
        err = np.zeros((self.H, self.W), dtype=np.float32)
        _check(lib().rt_accum_error(self._h, err.ctypes.data), "rt_accum_error")
        return err

    def error_device(self, err_ptr: int, stream: int = 0):
        _check(lib().rt_accum_error_device(self._h, ctypes.c_void_p(err_ptr or None), ctypes.c_void_p(stream or None)),
               "rt_accum_error_device")

    def state(self):
        """The checkpoint: (samples, sum float64 [H, W, 3], sq float64 [H, W, 3] or None without moments)."""
        n = ctypes.c_int64(0)
        s = np.zeros((self.H, self.W, 3), dtype=np.float64)
        q = np.zeros((self.H, self.W, 3), dtype=np.float64) if self.moments else None
        _check(lib().rt_accum_state(self._h, ctypes.byref(n), s.ctypes.data, q.ctypes.data if self.moments else None),
               "rt_accum_state")
        return n.value, s, q

    def restore(self, samples: int, sum, sq=None):
        s = np.ascontiguousarray(sum, dtype=np.float64)
        q = None if sq is None else np.ascontiguousarray(sq, dtype=np.float64)
        if s.size != 3 * self.W * self.H or (q is not None and q.size != s.size):
            raise ValueError("restore: sum and sq are float64 [H, W, 3]")
        _check(lib().rt_accum_restore(self._h, samples, s.ctypes.data, None if q is None else q.ctypes.data),
               "rt_accum_restore")

    def reset(self):
        _check(lib().rt_accum_reset(self._h), "rt_accum_reset")

    # ---- adaptive sampling (counts=True) ----
    def select_error(self, threshold: float, max_samples: int) -> int:
        """Select the pixels with fewer than max_samples samples whose error() exceeds threshold (or is NaN, or
        that have fewer than two samples) -> how many (moments only). Blocks."""
        n = ctypes.c_int64(0)
        _check(lib().rt_accum_select_error(self._h, threshold, max_samples, ctypes.byref(n)), "rt_accum_select_error")
        self._nsel = n.value
        return n.value

    def select_mask(self, mask) -> int:
        """Select the pixels where mask [H, W] is nonzero -> how many. Blocks."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.size != self.W * self.H:
            raise ValueError("select_mask: mask is [H, W]")
        n = ctypes.c_int64(0)
        _check(lib().rt_accum_select_mask(self._h, m.ctypes.data, ctypes.byref(n)), "rt_accum_select_mask")
        self._nsel = n.value
        return n.value

    def select_mask_device(self, mask_ptr: int, stream: int = 0) -> int:
        """select_mask from a device uint8 [H, W] mask on a HIP stream -> how many. Blocks."""
        n = ctypes.c_int64(0)
        _check(lib().rt_accum_select_mask_device(self._h, ctypes.c_void_p(mask_ptr or None), ctypes.c_void_p(stream or None),
                                                 ctypes.byref(n)), "rt_accum_select_mask_device")
        self._nsel = n.value
        return n.value

    def selection(self) -> np.ndarray:
        """The current selection's pixel indices (row * W + col, int32), in its tile-major order."""
        px = np.zeros(self.W * self.H, dtype=np.int32)
        _check(lib().rt_accum_selection(self._h, px.ctypes.data), "rt_accum_selection")
        return px[: self._nsel]

    def add_selected(self, count: int, stream: int = 0):
        """Shade the next `count` samples of every selected pixel; asynchronous on `stream` (0: the scene's own)."""
        _check(lib().rt_accum_add_selected(self._h, count, ctypes.c_void_p(stream or None)), "rt_accum_add_selected")

    def counts(self) -> np.ndarray:
        """The samples each pixel has received -> int32 [H, W]."""
        c = np.zeros((self.H, self.W), dtype=np.int32)
        _check(lib().rt_accum_counts(self._h, c.ctypes.data), "rt_accum_counts")
        return c

    def counts_device(self, cnt_ptr: int, stream: int = 0):
        _check(lib().rt_accum_counts_device(self._h, ctypes.c_void_p(cnt_ptr or None), ctypes.c_void_p(stream or None)),
               "rt_accum_counts_device")

    def restore_counts(self, cnt):
        """After restore(): the per-pixel counts of a checkpoint (int32 [H, W])."""
        c = np.ascontiguousarray(cnt, dtype=np.int32)
        if c.size != self.W * self.H:
            raise ValueError("restore_counts: cnt is int32 [H, W]")
        _check(lib().rt_accum_restore_counts(self._h, c.ctypes.data), "rt_accum_restore_counts")

    def denoiser(self) -> "Denoiser":
        """The variance-guided a-trous denoiser of this frame (rt_denoise_create; moments only): builds the guides
        of the frame's centre rays once. Close it before the accumulator."""
        return Denoiser(self)

    def close(self):
        if self._h:
            lib().rt_accum_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DenoiseParams(ctypes.Structure):
    """rt_denoise_params; DenoiseParams.defaults() is rt_denoise_defaults, keyword arguments override fields."""
    _fields_ = [("levels", ctypes.c_int32), ("normal_log2", ctypes.c_int32), ("sigma_l", ctypes.c_double),
                ("sigma_z", ctypes.c_double)]

    @classmethod
    def defaults(cls, **over) -> "DenoiseParams":
        p = cls()
        _check(lib().rt_denoise_defaults(ctypes.byref(p)), "rt_denoise_defaults")
        for k, v in over.items():
            if k not in ("levels", "normal_log2", "sigma_l", "sigma_z"):
                raise TypeError(f"unknown denoise parameter {k}")
            setattr(p, k, v)
        return p


class Denoiser:
    """The denoise step of an Accumulator's frame (rt_denoise_*): an edge-avoiding a-trous filter whose colour
    edge-stop is scaled by the per-pixel variance of the mean. Holds a reference to its accumulator (a denoiser
    must be closed before it). Parameters are DenoiseParams fields given as keywords over the defaults."""

    def __init__(self, accum: Accumulator):
        self._h = None
        self.accum, self.W, self.H = accum, accum.W, accum.H
        h = ctypes.c_void_p()
        _check(lib().rt_denoise_create(accum._h, ctypes.byref(h)), "rt_denoise_create")
        self._h = h

    def rebuild(self):
        """Trace the guides again for the accumulator's current camera pose, into the same buffers: what a run
        needs after Accumulator.set_camera (rt_denoise_rebuild). Blocks."""
        _check(lib().rt_denoise_rebuild(self._h), "rt_denoise_rebuild")

    def guides(self) -> dict:
        """The guides of the frame's centre rays: normal float32 [H, W, 3], pos float32 [H, W, 3], depth float32
        [H, W], material int32 [H, W] (-1 and zeros where the ray missed or was rejected)."""
        g = {"normal": np.zeros((self.H, self.W, 3), dtype=np.float32), "pos": np.zeros((self.H, self.W, 3), dtype=np.float32),
             "depth": np.zeros((self.H, self.W), dtype=np.float32), "material": np.zeros((self.H, self.W), dtype=np.int32)}
        _check(lib().rt_denoise_guides(self._h, g["normal"].ctypes.data, g["pos"].ctypes.data, g["depth"].ctypes.data,
                                       g["material"].ctypes.data), "rt_denoise_guides")
        return g

    def run(self, **params):
        """The denoised frame of the samples so far -> (rgb float32 [H, W, 3], argb int32 [H, W]). Blocks."""
        p = DenoiseParams.defaults(**params)
        rgb = np.zeros((self.H, self.W, 3), dtype=np.float32)
        argb = np.zeros((self.H, self.W), dtype=np.int32)
        _check(lib().rt_denoise_run(self._h, ctypes.byref(p), rgb.ctypes.data, argb.ctypes.data), "rt_denoise_run")
        return rgb, argb

    def run_device(self, rgb_ptr: int, argb_ptr: int, stream: int = 0, **params):
        """run() into device buffers (either may be 0) on a HIP stream; the caller orders it against add."""
        p = DenoiseParams.defaults(**params)
        _check(lib().rt_denoise_run_device(self._h, ctypes.byref(p), ctypes.c_void_p(rgb_ptr or None), ctypes.c_void_p(argb_ptr or None),
                                           ctypes.c_void_p(stream or None)), "rt_denoise_run_device")

    def planes(self):
        """The last run's final fp64 planes -> (colour float64 [H, W, 3], variance of the mean float64 [H, W])."""
        c = np.zeros((self.H, self.W, 3), dtype=np.float64)
        v = np.zeros((self.H, self.W), dtype=np.float64)
        _check(lib().rt_denoise_planes(self._h, c.ctypes.data, v.ctypes.data), "rt_denoise_planes")
        return c, v

    def close(self):
        if self._h:
            lib().rt_denoise_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# NodeD (csrc/rt_types.h): one 64-B line per child
NODE_DTYPE = np.dtype([("lmin", "<f8", 3), ("lmax", "<f8", 3), ("left", "<i4"), ("pad", "<i4", 3),
                       ("rmin", "<f8", 3), ("rmax", "<f8", 3), ("right", "<i4"), ("padR", "<i4", 3)])
assert NODE_DTYPE.itemsize == 128


def photon_maps_equal(a, b) -> bool:
    """Two Scene.photon_map() results are the same structure: refs / ranges / counts and the
    leaf-ordered photons bit-equal, boxes equal as numbers (a zero bound may carry either sign)."""
    na, ra, pa, wa = a
    nb, rb, pb, wb = b
    if na.shape != nb.shape or ra != rb:
        return False
    x, y = na.view(NODE_DTYPE).ravel(), nb.view(NODE_DTYPE).ravel()
    ints = all(np.array_equal(x[f], y[f]) for f in ("left", "pad", "right", "padR"))
    boxes = all(np.array_equal(x[f], y[f]) for f in ("lmin", "lmax", "rmin", "rmax"))
    return ints and boxes and np.array_equal(pa.view(np.uint64), pb.view(np.uint64)) and \
        np.array_equal(wa.view(np.uint64), wb.view(np.uint64))


def argb_to_rgb8(argb: np.ndarray) -> np.ndarray:
    a = argb.view(np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8)
