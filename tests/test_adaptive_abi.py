"""Adaptive sampling at the C-ABI boundary, without a GPU: the nine entries added to ABI 7 are exported, the
new creation flag RT_ACCUM_COUNTS = 4 is known and bit 2 is still not, and every bad argument is refused with
RT_E_INVALID and a message that starts with the entry's name before the scene is read or a device call made.

The entries get a host-made accumulator, as in test_accum_abi.py: a zeroed buffer whose first word is the
accumulator's accum_flags and whose int64 at byte 16 is its sample count. Its scene pointer is NULL: a check
that went on to the scene would crash the test."""
import ctypes
import struct

import numpy as np
import pytest

from distraytracer_old_amd import rt

RT_E_INVALID = -1
ENTRIES = ["rt_accum_select_error", "rt_accum_select_mask", "rt_accum_select_mask_device", "rt_accum_selection",
           "rt_accum_add_selected", "rt_accum_counts", "rt_accum_counts_device", "rt_accum_restore_counts"]


def test_symbols_are_exported():
    L = rt.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in rt.EXPORTS
    assert L.rt_abi_version() == 7  # additive: the version did not move
    assert rt.ACCUM_COUNTS == 4 and rt.ACCUM_MOMENTS == 1


def _refused(entry, rc, word=None):
    assert rc == RT_E_INVALID, entry
    msg = rt.lib().rt_last_error().decode()
    assert msg.startswith(entry + ":") and len(msg) > len(entry) + 2, msg
    if word:
        assert word in msg, msg


def _create(accum_flags, W):
    fake = ctypes.create_string_buffer(64)  # a dummy non-NULL scene: a refused call must not read it
    p = rt.params(W, 6, 0, 1)
    h = ctypes.c_void_p()
    rc = rt.lib().rt_accum_create(ctypes.addressof(fake), ctypes.addressof(p), accum_flags, ctypes.addressof(h))
    assert h.value is None
    return rc


@pytest.mark.parametrize("accum_flags", [4, 5])
def test_the_counts_flag_is_known(accum_flags):
    # with a zero width the call is refused for the size, which create checks after the flags
    _refused("rt_accum_create", _create(accum_flags, 0), "image size")


@pytest.mark.parametrize("accum_flags", [2, 4 | 2, 4 | (1 << 31), 5 | (1 << 31)])
def test_unknown_bits_beside_the_counts_flag_are_refused(accum_flags):
    _refused("rt_accum_create", _create(accum_flags, 0), "accum_flags")
    _refused("rt_accum_create", _create(accum_flags, 8), "accum_flags")


def _fake_accum(counts=True, moments=True, done=0):
    buf = ctypes.create_string_buffer(512)
    struct.pack_into("<I", buf, 0, (rt.ACCUM_COUNTS if counts else 0) | (rt.ACCUM_MOMENTS if moments else 0))
    struct.pack_into("<q", buf, 16, done)
    return buf


def _calls(a, out, n):
    """entry -> a call with good arguments on the accumulator at address a"""
    L = rt.lib()
    return {
        "rt_accum_select_error": lambda: L.rt_accum_select_error(a, 0.5, 8, ctypes.addressof(n)),
        "rt_accum_select_mask": lambda: L.rt_accum_select_mask(a, out.ctypes.data, ctypes.addressof(n)),
        "rt_accum_select_mask_device": lambda: L.rt_accum_select_mask_device(a, out.ctypes.data, None, ctypes.addressof(n)),
        "rt_accum_selection": lambda: L.rt_accum_selection(a, out.ctypes.data),
        "rt_accum_add_selected": lambda: L.rt_accum_add_selected(a, 1, None),
        "rt_accum_counts": lambda: L.rt_accum_counts(a, out.ctypes.data),
        "rt_accum_counts_device": lambda: L.rt_accum_counts_device(a, out.ctypes.data, None),
        "rt_accum_restore_counts": lambda: L.rt_accum_restore_counts(a, out.ctypes.data),
    }


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_accumulator_is_refused(entry):
    out, n = np.zeros(64, dtype=np.int32), ctypes.c_int64(0)
    _refused(entry, _calls(None, out, n)[entry]())


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("entry", ENTRIES)
def test_an_accumulator_without_counts_is_refused(entry, moments):
    a = _fake_accum(counts=False, moments=moments, done=4)
    out, n = np.zeros(64, dtype=np.int32), ctypes.c_int64(0)
    _refused(entry, _calls(ctypes.addressof(a), out, n)[entry](), "RT_ACCUM_COUNTS")


BAD_SELECT_ERROR = {
    "no moments": dict(moments=False),
    "negative threshold": dict(threshold=-1e-6),
    "NaN threshold": dict(threshold=float("nan")),
    "max_samples 0": dict(max_samples=0),
    "max_samples -1": dict(max_samples=-1),
    "null selected": dict(selected=False),
}


@pytest.mark.parametrize("case", list(BAD_SELECT_ERROR))
def test_bad_select_error_arguments_are_refused(case):
    c = BAD_SELECT_ERROR[case]
    a = _fake_accum(moments=c.get("moments", True), done=4)
    n = ctypes.c_int64(0)
    _refused("rt_accum_select_error",
             rt.lib().rt_accum_select_error(ctypes.addressof(a), c.get("threshold", 0.5), c.get("max_samples", 8),
                                            ctypes.addressof(n) if c.get("selected", True) else None))


def test_null_buffers_are_refused():
    L = rt.lib()
    a = _fake_accum(done=4)
    p = ctypes.addressof(a)
    out, n = np.zeros(64, dtype=np.uint8), ctypes.c_int64(0)
    _refused("rt_accum_select_mask", L.rt_accum_select_mask(p, None, ctypes.addressof(n)), "mask")
    _refused("rt_accum_select_mask", L.rt_accum_select_mask(p, out.ctypes.data, None), "selected")
    _refused("rt_accum_select_mask_device", L.rt_accum_select_mask_device(p, None, None, ctypes.addressof(n)), "mask")
    _refused("rt_accum_select_mask_device", L.rt_accum_select_mask_device(p, out.ctypes.data, None, None), "selected")
    _refused("rt_accum_selection", L.rt_accum_selection(p, None), "pixels")
    _refused("rt_accum_counts", L.rt_accum_counts(p, None), "cnt")
    _refused("rt_accum_counts_device", L.rt_accum_counts_device(p, None, None), "cnt")
    _refused("rt_accum_restore_counts", L.rt_accum_restore_counts(p, None), "cnt")


@pytest.mark.parametrize("count", [0, -1, -(1 << 31)])
def test_add_selected_refuses_a_count_below_one(count):
    a = _fake_accum(done=4)
    _refused("rt_accum_add_selected", rt.lib().rt_accum_add_selected(ctypes.addressof(a), count, None), "count")


def test_add_selected_and_selection_are_refused_before_any_select():
    a = _fake_accum(done=4)
    out = np.zeros(64, dtype=np.int32)
    _refused("rt_accum_add_selected", rt.lib().rt_accum_add_selected(ctypes.addressof(a), 1, None), "selection")
    _refused("rt_accum_selection", rt.lib().rt_accum_selection(ctypes.addressof(a), out.ctypes.data), "selection")


@pytest.mark.parametrize("entry", ["rt_accum_resolve", "rt_accum_error"])
def test_resolve_and_error_before_any_add_are_refused_with_counts_too(entry):
    a = _fake_accum(done=0)
    out = np.zeros(16, dtype=np.float32)
    args = (ctypes.addressof(a), out.ctypes.data) + ((None,) if entry == "rt_accum_resolve" else ())
    _refused(entry, getattr(rt.lib(), entry)(*args))
