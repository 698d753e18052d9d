"""The ray-query entries at the C-ABI boundary (rt_trace_rays / rt_trace_rays_device, added to ABI 7),
without a GPU: the symbols are exported, every bad argument is refused with RT_E_INVALID and a message
before the scene is read or a device call made, the three structs have the documented layout, and the
generated scenes the GPU tests lean on mean the same to the plain-Python restatement
(tests/golden/make_kats.py) and to the oracle."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from distraytracer_old_amd import desc, rt

from tests import trace_util as tu

REPO = Path(__file__).resolve().parent.parent
RT_E_INVALID = -1


def test_trace_symbols_are_exported():
    L = rt.lib()
    for name in ("rt_trace_rays", "rt_trace_rays_device"):
        assert hasattr(L, name), name
        assert name in rt.EXPORTS
    assert L.rt_abi_version() == 7  # additive: the version did not move


def _args(scene=True, params=True, rays=True, n=4, hits=True, occ=True, flags=0):
    """Argument tuple with the chosen ones NULL. The scene is a dummy non-NULL pointer: a refused
    call must not read it."""
    keep = []
    fake = ctypes.create_string_buffer(64)
    p = desc.TraceParams(0, 0, flags, 0)
    r = np.zeros(4, dtype=desc.RAY_DTYPE)
    h = np.zeros(4, dtype=desc.HIT_DTYPE)
    o = np.zeros(4, dtype=np.uint8)
    keep += [fake, p, r, h, o]
    return keep, (ctypes.addressof(fake) if scene else None, ctypes.addressof(p) if params else None,
                  r.ctypes.data if rays else None, n, h.ctypes.data if hits else None, o.ctypes.data if occ else None)


BAD = {
    "null scene": dict(scene=False),
    "null params": dict(params=False),
    "null rays": dict(rays=False),
    "negative n": dict(n=-1),
    "closest without hits": dict(hits=False),
    "any without occluded": dict(occ=False, flags=rt.TRACE_ANY),
}


@pytest.mark.parametrize("entry", ["rt_trace_rays", "rt_trace_rays_device"])
@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused(entry, case):
    L = rt.lib()
    keep, a = _args(**BAD[case])
    if entry == "rt_trace_rays_device":
        a = a + (None,)
    assert getattr(L, entry)(*a) == RT_E_INVALID, case
    msg = L.rt_last_error().decode()
    assert entry in msg and len(msg) > len(entry) + 2, msg


@pytest.mark.parametrize("entry", ["rt_trace_rays", "rt_trace_rays_device"])
def test_zero_rays_is_ok(entry):
    L = rt.lib()
    keep, a = _args(n=0)
    if entry == "rt_trace_rays_device":
        a = a + (None,)
    assert getattr(L, entry)(*a) == 0


def test_struct_layout_matches_a_gcc_probe(tmp_path):
    want = {"rt_ray": (56, {"o": 0, "d": 24, "tmax": 48}),
            "rt_hit": (80, {"t": 0, "pos": 8, "normal": 32, "prim": 56, "top": 60, "material": 64, "args": 68,
                            "flags": 72, "pad": 76}),
            "rt_trace_params": (24, {"seed": 0, "first_key": 8, "flags": 16, "pad": 20})}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "distraytracer.h"', 'int main(void) {']
    for cname, (_, fields) in want.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("  return 0; }")
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", str(REPO / "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    mirrors = {"rt_ray": (desc.Ray, desc.RAY_DTYPE), "rt_hit": (desc.Hit, desc.HIT_DTYPE),
               "rt_trace_params": (desc.TraceParams, None)}
    for cname, (size, fields) in want.items():
        T, dt = mirrors[cname]
        assert int(got[f"{cname} size"]) == size == ctypes.sizeof(T), cname
        assert desc.STRUCTS[cname] is T
        for f, off in fields.items():
            assert int(got[f"{cname} {f}"]) == off == getattr(T, f).offset, (cname, f)
            if dt is not None:
                assert dt.fields[f][1] == off, (cname, f)


@pytest.mark.parametrize("kind", ["a", "b"])
def test_generated_scenes_mean_the_same_to_restatement_and_oracle(kind, tmp_path):
    """What the GPU test leans on: on the generated scene texts, the plain-Python findClosestRayHit and
    the oracle's camera_hits agree on every un-jittered camera ray at 48 x 48."""
    from oracle.oracle import OracleScene

    W = H = 48
    text = tu.scene_text(kind)
    (tmp_path / "gen.cli").write_text(text)
    mask = OracleScene(tmp_path, "gen.cli", {}).camera_hits(W, H)
    m = tu.make_kats()
    sc = m.load(text, W, H)
    o, d = tu.camera_rays(W, H, 60.0)
    mine = np.array([sc.closest(m.Ray(o[i], d[i], 0)) is not None for i in range(W * H)], dtype=np.uint8).reshape(H, W)
    assert 0.2 < mask.mean() < 0.95  # the scene is in view
    assert int((mine != mask).sum()) == 0
