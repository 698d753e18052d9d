"""RT_TRACE_SORT at the C-ABI boundary, without a GPU: rt_trace_order / rt_trace_order_device (added to
ABI 7) are exported, every bad argument is refused with RT_E_INVALID and a message before the scene is
read or a device call made, n == 0 is RT_OK, and the binding's flag equals the header's."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from distraytracer_old_amd import desc, rt

HEADER = Path(__file__).resolve().parent.parent / "include" / "distraytracer.h"
RT_E_INVALID = -1
ENTRIES = ["rt_trace_order", "rt_trace_order_device"]


def test_order_symbols_are_exported():
    L = rt.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in rt.EXPORTS
    assert L.rt_abi_version() == 7  # additive: the version did not move


def test_flag_equals_the_header():
    m = re.search(r"#define\s+RT_TRACE_SORT\s+(\d+)u", HEADER.read_text())
    assert m and int(m.group(1)) == rt.TRACE_SORT == 16
    others = rt.TRACE_ANY | rt.TRACE_LANES | rt.TRACE_NOCULL | rt.TRACE_GENERIC
    assert rt.TRACE_SORT & others == 0


def _args(scene=True, params=True, rays=True, n=4, order=True):
    """Argument tuple with the chosen ones NULL. The scene is a dummy non-NULL pointer: a refused call
    (and a call with n == 0) must not read it."""
    fake = ctypes.create_string_buffer(64)
    p = desc.TraceParams(0, 0, 0, 0)
    r = np.zeros(4, dtype=desc.RAY_DTYPE)
    o = np.zeros(4, dtype=np.uint32)
    keep = [fake, p, r, o]
    return keep, (ctypes.addressof(fake) if scene else None, ctypes.addressof(p) if params else None,
                  r.ctypes.data if rays else None, n, o.ctypes.data if order else None)


BAD = {
    "null scene": dict(scene=False),
    "null params": dict(params=False),
    "null rays": dict(rays=False),
    "null order": dict(order=False),
    "negative n": dict(n=-1),
    "n = 2^32": dict(n=1 << 32),
}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused(entry, case):
    L = rt.lib()
    keep, a = _args(**BAD[case])
    if entry == "rt_trace_order_device":
        a = a + (None,)
    assert getattr(L, entry)(*a) == RT_E_INVALID, case
    msg = L.rt_last_error().decode()
    assert msg.startswith(entry + ":") and len(msg) > len(entry) + 2, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_rays_is_ok(entry):
    L = rt.lib()
    keep, a = _args(n=0)
    if entry == "rt_trace_order_device":
        a = a + (None,)
    assert getattr(L, entry)(*a) == 0
