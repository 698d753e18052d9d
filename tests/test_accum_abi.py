"""Progressive sample accumulation at the C-ABI boundary, without a GPU: the eleven rt_accum_* entries (added
to ABI 7) are exported, and every bad argument is refused with RT_E_INVALID and a message that starts with the
entry's name before the scene is read or a device call made.

Without a device no accumulator can be created, so the entries that take one get a host-made one: a zeroed
buffer whose first word is the accumulator's accum_flags and whose int64 at byte 16 is its sample count (the
two fields the argument checks read; csrc/accum.hip pins their offsets). Its scene pointer is NULL: a check
that went on to the scene would crash the test."""
import ctypes
import struct

import numpy as np
import pytest

from distraytracer_old_amd import rt

RT_E_INVALID = -1
ENTRIES = ["rt_accum_create", "rt_accum_add", "rt_accum_samples", "rt_accum_resolve", "rt_accum_resolve_device",
           "rt_accum_error", "rt_accum_error_device", "rt_accum_state", "rt_accum_restore", "rt_accum_reset",
           "rt_accum_destroy"]


def test_symbols_are_exported():
    L = rt.lib()
    assert len(ENTRIES) == 11
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in rt.EXPORTS
    assert L.rt_abi_version() == 7  # additive: the version did not move
    assert rt.ACCUM_MOMENTS == 1


def _refused(entry, rc):
    assert rc == RT_E_INVALID, entry
    msg = rt.lib().rt_last_error().decode()
    assert msg.startswith(entry + ":") and len(msg) > len(entry) + 2, msg


def _create_args(scene=True, params=True, out=True, flags=0, accum_flags=0, rows=None, row_step=1, row_band=1, W=8, H=6):
    fake = ctypes.create_string_buffer(64)  # a dummy non-NULL scene: a refused call must not read it
    p = rt.params(W, H, 0, 1, rows=rows, row_step=row_step, flags=flags, row_band=row_band)
    h = ctypes.c_void_p()
    keep = [fake, p, h]
    return keep, (ctypes.addressof(fake) if scene else None, ctypes.addressof(p) if params else None, accum_flags,
                  ctypes.addressof(h) if out else None)


BAD_CREATE = {
    "null scene": dict(scene=False),
    "null params": dict(params=False),
    "null out": dict(out=False),
    "rows from 1": dict(rows=(1, 6)),
    "rows to 5": dict(rows=(0, 5)),
    "row step": dict(row_step=2),
    "row band": dict(row_band=2),
    "unknown flag bit": dict(flags=1 << 31),
    "RT_RENDER_SHCOMPACT": dict(flags=rt.RENDER_SHCOMPACT),
    "RT_RENDER_WAVEFRONT": dict(flags=rt.RENDER_WAVEFRONT),
    "RT_RENDER_PIXEL_WAVES": dict(flags=rt.RENDER_PIXEL_WAVES),
    "a known flag beside an unknown bit": dict(flags=rt.RENDER_GENERIC | rt.RENDER_ROWMAJOR),
    "unknown accum_flags bit": dict(accum_flags=2),
    "moments beside an unknown accum_flags bit": dict(accum_flags=rt.ACCUM_MOMENTS | (1 << 31)),
    "zero width": dict(W=0),
}


@pytest.mark.parametrize("case", list(BAD_CREATE))
def test_bad_create_arguments_are_refused(case):
    keep, a = _create_args(**BAD_CREATE[case])
    _refused("rt_accum_create", rt.lib().rt_accum_create(*a))
    assert keep[2].value is None  # no handle came out


def _fake_accum(moments=False, done=0):
    buf = ctypes.create_string_buffer(256)
    struct.pack_into("<I", buf, 0, rt.ACCUM_MOMENTS if moments else 0)
    struct.pack_into("<q", buf, 16, done)
    return buf


def test_null_accumulator_is_refused():
    L = rt.lib()
    out = np.zeros(16)
    n = ctypes.c_int64(0)
    _refused("rt_accum_add", L.rt_accum_add(None, 1, None))
    _refused("rt_accum_samples", L.rt_accum_samples(None, ctypes.addressof(n)))
    _refused("rt_accum_resolve", L.rt_accum_resolve(None, out.ctypes.data, None))
    _refused("rt_accum_resolve_device", L.rt_accum_resolve_device(None, out.ctypes.data, None, None))
    _refused("rt_accum_error", L.rt_accum_error(None, out.ctypes.data))
    _refused("rt_accum_error_device", L.rt_accum_error_device(None, out.ctypes.data, None))
    _refused("rt_accum_state", L.rt_accum_state(None, ctypes.addressof(n), None, None))
    _refused("rt_accum_restore", L.rt_accum_restore(None, 0, out.ctypes.data, None))
    _refused("rt_accum_reset", L.rt_accum_reset(None))
    L.rt_accum_destroy(None)  # a no-op


@pytest.mark.parametrize("count", [0, -1, -(1 << 31)])
def test_add_refuses_a_count_below_one(count):
    a = _fake_accum(done=4)
    _refused("rt_accum_add", rt.lib().rt_accum_add(ctypes.addressof(a), count, None))


def test_add_refuses_a_total_of_two_to_the_31():
    a = _fake_accum(done=(1 << 31) - 1)
    _refused("rt_accum_add", rt.lib().rt_accum_add(ctypes.addressof(a), 1, None))


def test_samples_reads_the_count_and_refuses_a_null_output():
    L = rt.lib()
    a = _fake_accum(done=37)
    n = ctypes.c_int64(0)
    assert L.rt_accum_samples(ctypes.addressof(a), ctypes.addressof(n)) == 0 and n.value == 37
    _refused("rt_accum_samples", L.rt_accum_samples(ctypes.addressof(a), None))


@pytest.mark.parametrize("entry", ["rt_accum_resolve", "rt_accum_resolve_device"])
def test_resolve_at_zero_samples_is_refused(entry):
    a = _fake_accum(done=0)
    out = np.zeros(16, dtype=np.float32)
    args = (ctypes.addressof(a), out.ctypes.data, None) + ((None,) if entry.endswith("_device") else ())
    _refused(entry, getattr(rt.lib(), entry)(*args))


@pytest.mark.parametrize("entry", ["rt_accum_error", "rt_accum_error_device"])
@pytest.mark.parametrize("case", ["no moments", "no samples", "one sample", "null err"])
def test_error_needs_moments_and_two_samples(entry, case):
    a = _fake_accum(moments=case != "no moments", done={"no samples": 0, "one sample": 1}.get(case, 16))
    out = np.zeros(16, dtype=np.float32)
    args = (ctypes.addressof(a), None if case == "null err" else out.ctypes.data) + ((None,) if entry.endswith("_device") else ())
    _refused(entry, getattr(rt.lib(), entry)(*args))


BAD_RESTORE = {
    "negative sample count": dict(moments=False, samples=-1, sum=True, sq=False),
    "negative sample count, moments": dict(moments=True, samples=-1, sum=True, sq=True),
    "2^31 samples": dict(moments=False, samples=1 << 31, sum=True, sq=False),
    "null sum": dict(moments=False, samples=3, sum=False, sq=False),
    "sq given without moments": dict(moments=False, samples=3, sum=True, sq=True),
    "sq missing with moments": dict(moments=True, samples=3, sum=True, sq=False),
}


@pytest.mark.parametrize("case", list(BAD_RESTORE))
def test_bad_restore_arguments_are_refused(case):
    c = BAD_RESTORE[case]
    a = _fake_accum(moments=c["moments"], done=5)
    s, q = np.zeros(16), np.zeros(16)
    _refused("rt_accum_restore", rt.lib().rt_accum_restore(ctypes.addressof(a), c["samples"], s.ctypes.data if c["sum"] else None,
                                                           q.ctypes.data if c["sq"] else None))
    assert struct.unpack_from("<q", a, 16)[0] == 5  # the refused call changed nothing


def test_state_refuses_sq_without_moments():
    a = _fake_accum(moments=False, done=5)
    q = np.zeros(16)
    _refused("rt_accum_state", rt.lib().rt_accum_state(ctypes.addressof(a), None, None, q.ctypes.data))
