"""Radiance queries and camera rays at the C-ABI boundary, without a GPU: rt_shade_rays / rt_shade_rays_device
and rt_camera_rays / rt_camera_rays_device (added to ABI 7) are exported, rt_shade_params has the header's
layout, every bad argument is refused with RT_E_INVALID and a message that starts with the entry's name before
the scene is read or a device call made, and n == 0 is RT_OK."""
import ctypes

import numpy as np
import pytest

from distraytracer_old_amd import desc, rt

RT_E_INVALID = -1
SHADE = ["rt_shade_rays", "rt_shade_rays_device"]
CAMERA = ["rt_camera_rays", "rt_camera_rays_device"]


def test_symbols_are_exported():
    L = rt.lib()
    for name in SHADE + CAMERA:
        assert hasattr(L, name), name
        assert name in rt.EXPORTS
    assert L.rt_abi_version() == 7  # additive: the version did not move


def test_shade_params_layout():
    T = desc.ShadeParams
    assert ctypes.sizeof(T) == 24
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("seed", 0), ("first_key", 8), ("flags", 16),
                                                                  ("sample", 20)]
    assert desc.STRUCTS["rt_shade_params"] is T  # test_desc.py checks every STRUCTS entry against a gcc probe


def _shade_args(scene=True, params=True, rays=True, n=4, rgb=True, status=True, flags=0):
    """Argument tuple with the chosen ones NULL. The scene is a dummy non-NULL pointer: a refused call
    (and a call with n == 0) must not read it."""
    fake = ctypes.create_string_buffer(64)
    p = desc.ShadeParams(0, 0, flags, 0)
    r = np.zeros(4, dtype=desc.RAY_DTYPE)
    c = np.zeros((4, 3), dtype=np.float64)
    s = np.zeros(4, dtype=np.uint8)
    keep = [fake, p, r, c, s]
    return keep, (ctypes.addressof(fake) if scene else None, ctypes.addressof(p) if params else None,
                  r.ctypes.data if rays else None, n, c.ctypes.data if rgb else None, s.ctypes.data if status else None)


BAD_SHADE = {
    "null scene": dict(scene=False),
    "null params": dict(params=False),
    "null rays": dict(rays=False),
    "null rgb": dict(rgb=False),
    "negative n": dict(n=-1),
    "RT_TRACE_ANY": dict(flags=rt.TRACE_ANY),
    "RT_TRACE_LANES": dict(flags=rt.TRACE_LANES),
    "unknown bit": dict(flags=1 << 31),
    "a known flag beside an unknown bit": dict(flags=rt.TRACE_SORT | (1 << 31)),
}


@pytest.mark.parametrize("entry", SHADE)
@pytest.mark.parametrize("case", list(BAD_SHADE))
def test_bad_shade_arguments_are_refused(entry, case):
    L = rt.lib()
    keep, a = _shade_args(**BAD_SHADE[case])
    if entry == "rt_shade_rays_device":
        a = a + (None,)
    assert getattr(L, entry)(*a) == RT_E_INVALID, case
    msg = L.rt_last_error().decode()
    assert msg.startswith(entry + ":") and len(msg) > len(entry) + 2, msg


@pytest.mark.parametrize("entry", SHADE)
@pytest.mark.parametrize("flags", [0, rt.TRACE_SORT | rt.TRACE_GENERIC | rt.TRACE_NOCULL])
def test_zero_rays_is_ok(entry, flags):
    L = rt.lib()
    for status in (True, False):
        keep, a = _shade_args(n=0, flags=flags, status=status)
        if entry == "rt_shade_rays_device":
            a = a + (None,)
        assert getattr(L, entry)(*a) == 0


def _camera_args(scene=True, params=True, rays=True):
    fake = ctypes.create_string_buffer(64)
    p = rt.params(2, 2, 1, 0)
    r = np.zeros(4, dtype=desc.RAY_DTYPE)
    keep = [fake, p, r]
    return keep, (ctypes.addressof(fake) if scene else None, ctypes.addressof(p) if params else None, 0,
                  r.ctypes.data if rays else None)


BAD_CAMERA = {"null scene": dict(scene=False), "null params": dict(params=False), "null rays": dict(rays=False)}


@pytest.mark.parametrize("entry", CAMERA)
@pytest.mark.parametrize("case", list(BAD_CAMERA))
def test_bad_camera_arguments_are_refused(entry, case):
    L = rt.lib()
    keep, a = _camera_args(**BAD_CAMERA[case])
    if entry == "rt_camera_rays_device":
        a = a + (None,)
    assert getattr(L, entry)(*a) == RT_E_INVALID, case
    msg = L.rt_last_error().decode()
    assert msg.startswith(entry + ":") and len(msg) > len(entry) + 2, msg
