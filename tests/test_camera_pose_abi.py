"""The camera pose at the C-ABI boundary, without a GPU: the seven entries (added to ABI 7) are exported, the two
host-only ones -- rt_camera_look_at, rt_camera_pose_check -- compute what the header says they compute, and every
bad argument is refused with RT_E_INVALID and a message that starts with the entry's name before a scene, an
accumulator or a device is touched.

Without a device nothing can be created, so the entries that take a handle get a host-made one where they need one at
all: a zeroed buffer (as tests/test_accum_abi.py makes its accumulator)."""
import ctypes

import numpy as np
import pytest

from distraytracer_old_amd import rt

RT_E_INVALID = -1
ENTRIES = ["rt_camera_pose_check", "rt_camera_look_at", "rt_camera_rays_pose", "rt_camera_rays_pose_device",
           "rt_accum_set_camera", "rt_accum_camera", "rt_denoise_rebuild"]


def test_symbols_are_exported():
    L = rt.lib()
    assert len(ENTRIES) == 7
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in rt.EXPORTS
    assert L.rt_abi_version() == 7  # additive: the version did not move


def _refused(entry, rc, names=None):
    assert rc == RT_E_INVALID, entry
    msg = rt.lib().rt_last_error().decode()
    assert msg.startswith(entry + ":") and len(msg) > len(entry) + 2, msg
    if names:
        assert names in msg, msg


# ---- rt_camera_look_at ----------------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def look_at_ref(eye, target, up):
    """The header's look-at, operation for operation, in float64."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye
    f = f / _norm(f)
    r = _cross(f, up)
    r = r / _norm(r)
    u = _cross(r, f)
    m = np.zeros((4, 4))
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, -f, eye
    m[3] = [0, 0, 0, 1]
    return m


TRIPLES = [
    ((0.4, 0.3, 1.5), (0.0, 0.0, -4.0), (0, 1, 0)),
    ((-2, 0.5, 1), (3, 1, -4), (0, 1, 0)),
    ((5.25, -3.5, 2.125), (-1, 7, 0.3), (0.1, 0.9, -0.2)),  # an up that is neither a unit vector nor orthogonal to the view
    ((1e-3, 2e5, -7), (4, 4, 4), (0, 0, 1)),
    ((0, 10, 0), (0, 0, 0), (1, 0, 0)),  # looking straight down
]


@pytest.mark.parametrize("eye,target,up", TRIPLES)
def test_look_at_equals_its_restatement(eye, target, up):
    got = rt.look_at(eye, target, up)
    want = look_at_ref(eye, target, up)
    assert got.shape == (4, 4) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    rt.pose_check(got)  # what comes out always passes the check


def test_look_at_of_the_reference_camera_is_the_identity():
    got = rt.look_at((0, 0, 0), (0, 0, -1))  # up defaults to +y
    assert (got == np.eye(4)).all(), got  # ==: -0.0 and +0.0 alike


@pytest.mark.parametrize("case,eye,target,up", [
    ("eye == target", (1, 2, 3), (1, 2, 3), (0, 1, 0)),
    ("up parallel to the view", (0, 0, 0), (0, 5, 0), (0, 1, 0)),
    ("up antiparallel to the view", (1, 1, 1), (1, 1, -3), (0, 0, 2)),
    ("zero up", (0, 0, 0), (0, 0, -1), (0, 0, 0)),
    ("NaN eye", (float("nan"), 0, 0), (0, 0, -1), (0, 1, 0)),
    ("NaN target", (0, 0, 0), (0, float("nan"), -1), (0, 1, 0)),
    ("NaN up", (0, 0, 0), (0, 0, -1), (0, 1, float("nan"))),
    ("Inf eye", (float("inf"), 0, 0), (0, 0, -1), (0, 1, 0)),
])
def test_look_at_refusals(case, eye, target, up):
    e, t, u = (np.array(v, dtype=np.float64) for v in (eye, target, up))
    out = np.full(16, 7.0)
    _refused("rt_camera_look_at", rt.lib().rt_camera_look_at(e.ctypes.data, t.ctypes.data, u.ctypes.data, out.ctypes.data))
    assert (out == 7.0).all(), case  # nothing was written
    with pytest.raises(rt.RTError, match="rt_camera_look_at"):
        rt.look_at(eye, target, up)


# ---- rt_camera_pose_check -------------------------------------------------------------------------------------
def rodrigues_pose():
    """The rotation about (1, 2, 3) / sqrt(14) by 0.7 rad with a translation: no symmetry a transposed reading keeps."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = [0.3, -0.2, 0.5]
    return m


def _check(m):
    m = np.ascontiguousarray(m, dtype=np.float64)
    return rt.lib().rt_camera_pose_check(m.ctypes.data)


def test_pose_check_accepts_rigid_poses():
    for eye, target, up in TRIPLES:
        assert _check(rt.look_at(eye, target, up)) == 0
    assert _check(rodrigues_pose()) == 0
    assert _check(np.eye(4)) == 0
    rt.pose_check(rodrigues_pose())


def _bad_poses():
    nan = rodrigues_pose()
    nan[1, 2] = float("nan")
    inf = rodrigues_pose()
    inf[0, 3] = float("inf")
    row = rodrigues_pose()
    row[3] = [0, 0, 1e-300, 1]
    row2 = rodrigues_pose()
    row2[3, 3] = 2
    scaled = 2 * np.eye(4)
    scaled[3, 3] = 1
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    mirror2 = rodrigues_pose()
    mirror2[:3, 0] = -mirror2[:3, 0]
    off = rodrigues_pose()
    off[0, 1] += 1e-6
    return [("a NaN entry", nan, "finite"), ("an Inf translation", inf, "finite"), ("a last row with a tiny entry", row, "last row"),
            ("a last row 0 0 0 2", row2, "last row"), ("2 I", scaled, "orthonormal"), ("a mirror", mirror, "reflection"),
            ("a rotation with one axis flipped", mirror2, "reflection"), ("a rotation off by 1e-6 in one entry", off, "orthonormal")]


@pytest.mark.parametrize("case,m,names", _bad_poses(), ids=[c[0] for c in _bad_poses()])
def test_pose_check_refusals_name_the_condition(case, m, names):
    _refused("rt_camera_pose_check", _check(m), names)
    with pytest.raises(rt.RTError, match="rt_camera_pose_check"):
        rt.pose_check(m)


def test_a_pose_is_sixteen_numbers():
    with pytest.raises(ValueError):
        rt.pose_check(np.eye(3))


# ---- null handles and null outputs ----------------------------------------------------------------------------
def test_null_arguments_are_refused():
    L = rt.lib()
    v = np.array([0.0, 0.0, 1.0])
    t = np.array([0.0, 0.0, -1.0])
    u = np.array([0.0, 1.0, 0.0])
    m = np.ascontiguousarray(rodrigues_pose())
    out = np.zeros(16)
    flag = ctypes.c_int(5)
    _refused("rt_camera_pose_check", L.rt_camera_pose_check(None))
    for args in ((None, t, u, out), (v, None, u, out), (v, t, None, out), (v, t, u, None)):
        _refused("rt_camera_look_at", L.rt_camera_look_at(*[None if a is None else a.ctypes.data for a in args]))
    _refused("rt_accum_set_camera", L.rt_accum_set_camera(None, m.ctypes.data))
    _refused("rt_accum_set_camera", L.rt_accum_set_camera(None, None))
    _refused("rt_accum_camera", L.rt_accum_camera(None, out.ctypes.data, ctypes.addressof(flag)))
    fake = ctypes.create_string_buffer(512)  # a zeroed accumulator: no pose
    _refused("rt_accum_camera", L.rt_accum_camera(ctypes.addressof(fake), None, ctypes.addressof(flag)))
    _refused("rt_accum_camera", L.rt_accum_camera(ctypes.addressof(fake), out.ctypes.data, None))
    _refused("rt_denoise_rebuild", L.rt_denoise_rebuild(None))
    p = rt.params(8, 6, 1)
    rays = np.zeros(8 * 6 * 7)
    scene = ctypes.create_string_buffer(64)  # a dummy non-NULL scene: a refused call must not read it
    for entry, tail in (("rt_camera_rays_pose", ()), ("rt_camera_rays_pose_device", (None,))):
        fn = getattr(L, entry)
        _refused(entry, fn(None, ctypes.addressof(p), 0, m.ctypes.data, rays.ctypes.data, *tail))
        _refused(entry, fn(ctypes.addressof(scene), None, 0, m.ctypes.data, rays.ctypes.data, *tail))
        _refused(entry, fn(ctypes.addressof(scene), ctypes.addressof(p), 0, m.ctypes.data, None, *tail))


def test_a_bad_pose_is_refused_before_the_handle_is_read():
    """An invalid pose is refused by every entry that takes one, with the failed condition named, on handles that
    could not be read: a dummy scene, a zeroed accumulator."""
    L = rt.lib()
    bad = np.ascontiguousarray(2 * np.eye(4))
    p = rt.params(8, 6, 1)
    rays = np.zeros(8 * 6 * 7)
    scene = ctypes.create_string_buffer(64)
    _refused("rt_camera_rays_pose", L.rt_camera_rays_pose(ctypes.addressof(scene), ctypes.addressof(p), 0, bad.ctypes.data,
                                                          rays.ctypes.data), "last row")
    _refused("rt_camera_rays_pose_device", L.rt_camera_rays_pose_device(ctypes.addressof(scene), ctypes.addressof(p), 0,
                                                                        bad.ctypes.data, rays.ctypes.data, None), "last row")
    fake = ctypes.create_string_buffer(512)
    bad[3, 3] = 1
    _refused("rt_accum_set_camera", L.rt_accum_set_camera(ctypes.addressof(fake), bad.ctypes.data), "orthonormal")


def test_an_accumulator_without_a_pose_reports_the_identity():
    fake = ctypes.create_string_buffer(512)
    out = np.full(16, 3.0)
    flag = ctypes.c_int(5)
    assert rt.lib().rt_accum_camera(ctypes.addressof(fake), out.ctypes.data, ctypes.addressof(flag)) == 0
    assert flag.value == 0 and np.array_equal(out.view(np.uint64), np.eye(4).reshape(16).view(np.uint64))
