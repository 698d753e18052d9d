"""The denoiser at the C-ABI boundary, without a GPU: the seven rt_denoise_* entries (added to ABI 7) are exported,
and every bad argument is refused with RT_E_INVALID and a message that starts with the entry's name before an
accumulator, a scene or a device is touched.

Without a device nothing can be created, so the entries get host-made handles: a zeroed buffer as the
accumulator whose first word is its accum_flags (as tests/test_accum_abi.py makes one), and a zeroed buffer as
the denoiser, whose accumulator pointer is NULL: a parameter check that went on to it would crash the test."""
import ctypes
import struct

import numpy as np
import pytest

from distraytracer_old_amd import rt

RT_E_INVALID = -1
ENTRIES = ["rt_denoise_defaults", "rt_denoise_create", "rt_denoise_guides", "rt_denoise_run", "rt_denoise_run_device",
           "rt_denoise_planes", "rt_denoise_destroy"]
RUNS = ["rt_denoise_run", "rt_denoise_run_device"]


def test_symbols_are_exported():
    L = rt.lib()
    assert len(ENTRIES) == 7
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in rt.EXPORTS
    assert L.rt_abi_version() == 7  # additive: the version did not move
    assert ctypes.sizeof(rt.DenoiseParams) == 24


def _refused(entry, rc):
    assert rc == RT_E_INVALID, entry
    msg = rt.lib().rt_last_error().decode()
    assert msg.startswith(entry + ":") and len(msg) > len(entry) + 2, msg


def _fake_accum(moments):
    buf = ctypes.create_string_buffer(256)
    struct.pack_into("<I", buf, 0, rt.ACCUM_MOMENTS if moments else 0)
    return buf


def _run(entry, d, p, out):
    args = (d, p, out.ctypes.data, None) + ((None,) if entry.endswith("_device") else ())
    return getattr(rt.lib(), entry)(*args)


def test_null_handle_is_refused():
    L = rt.lib()
    out = np.zeros(16)
    p = rt.DenoiseParams.defaults()
    _refused("rt_denoise_defaults", L.rt_denoise_defaults(None))
    _refused("rt_denoise_guides", L.rt_denoise_guides(None, out.ctypes.data, None, None, None))
    for entry in RUNS:
        _refused(entry, _run(entry, None, ctypes.addressof(p), out))
    _refused("rt_denoise_planes", L.rt_denoise_planes(None, out.ctypes.data, None))
    L.rt_denoise_destroy(None)  # a no-op


@pytest.mark.parametrize("case", ["null accumulator", "null out", "no moments"])
def test_bad_create_arguments_are_refused(case):
    a = _fake_accum(moments=case != "no moments")
    h = ctypes.c_void_p()
    rc = rt.lib().rt_denoise_create(None if case == "null accumulator" else ctypes.addressof(a),
                                    None if case == "null out" else ctypes.addressof(h))
    _refused("rt_denoise_create", rc)
    assert h.value is None  # no handle came out


BAD_PARAMS = {
    "levels -1": dict(levels=-1),
    "levels 9": dict(levels=9),
    "normal_log2 -1": dict(normal_log2=-1),
    "normal_log2 11": dict(normal_log2=11),
    "sigma_l 0": dict(sigma_l=0.0),
    "sigma_l negative": dict(sigma_l=-1.0),
    "sigma_l NaN": dict(sigma_l=float("nan")),
    "sigma_l Inf": dict(sigma_l=float("inf")),
    "sigma_z 0": dict(sigma_z=0.0),
    "sigma_z negative": dict(sigma_z=-0.5),
    "sigma_z NaN": dict(sigma_z=float("nan")),
    "sigma_z Inf": dict(sigma_z=float("inf")),
}


@pytest.mark.parametrize("entry", RUNS)
@pytest.mark.parametrize("case", ["null params"] + list(BAD_PARAMS))
def test_bad_run_parameters_are_refused(entry, case):
    d = ctypes.create_string_buffer(256)  # its accumulator is NULL: the refusal must come first
    out = np.zeros(16, dtype=np.float32)
    if case == "null params":
        _refused(entry, _run(entry, ctypes.addressof(d), None, out))
        return
    p = rt.DenoiseParams.defaults(**BAD_PARAMS[case])
    _refused(entry, _run(entry, ctypes.addressof(d), ctypes.addressof(p), out))


def test_defaults_are_values_the_run_accepts():
    p = rt.DenoiseParams()
    assert rt.lib().rt_denoise_defaults(ctypes.byref(p)) == 0
    assert 0 <= p.levels <= 8 and 0 <= p.normal_log2 <= 10
    assert np.isfinite(p.sigma_l) and p.sigma_l > 0 and np.isfinite(p.sigma_z) and p.sigma_z > 0
    assert (p.levels, p.normal_log2, p.sigma_l) == (5, 7, 4.0)  # SVGF's published values
    # a host-made accumulator without samples behind a host-made denoiser: the parameters pass, the run is then
    # refused for the missing samples (the last check that needs no device)
    a = _fake_accum(moments=True)
    d = ctypes.create_string_buffer(256)
    struct.pack_into("<Q", d, 0, ctypes.addressof(a))
    out = np.zeros(16, dtype=np.float32)
    for entry in RUNS:
        _refused(entry, _run(entry, ctypes.addressof(d), ctypes.addressof(p), out))
        assert "no samples" in rt.lib().rt_last_error().decode()
