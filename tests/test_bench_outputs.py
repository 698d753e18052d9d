"""bench.py --dump-outputs: what dump_outputs writes for a frame (exact values, float types, the
byte budget and its fixed seeded sample) and the device read-back it dumps from."""
import numpy as np
import pytest

import bench
from distraytracer_old_amd import rt


def _frame(H, W, seed=7):
    r = np.random.default_rng(seed)
    return r.integers(-2**31, 2**31, size=(H, W), dtype=np.int64).astype(np.int32)


def test_dump_whole_frame_is_exact(tmp_path):
    f = _frame(37, 53)
    info = bench.dump_outputs(tmp_path / "d", f)
    a = np.load(tmp_path / "d" / "argb.npy")
    c = np.load(tmp_path / "d" / "rgb.npy")
    assert a.dtype == np.float64 and a.shape == (37, 53) and np.array_equal(a.astype(np.int32), f)
    assert c.dtype == np.float32 and c.shape == (37, 53, 3) and np.array_equal(c.astype(np.uint8), rt.argb_to_rgb8(f))
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["argb.npy", "rgb.npy"]
    assert info["bytes"] == a.nbytes + c.nbytes


def test_dump_over_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 28 * 1000)
    f = _frame(64, 96)  # 64 * 96 * 20 B = 122,880 B > the budget
    one = bench.dump_outputs(tmp_path / "a", f)
    two = bench.dump_outputs(tmp_path / "b", f)
    assert one["bytes"] == two["bytes"] <= 28 * 1000
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "pixel_index.npy"))
    i = idx.astype(np.int64)
    assert len(i) == 1000 and (np.diff(i) > 0).all() and 0 <= i[0] and i[-1] < f.size
    a = np.load(tmp_path / "a" / "argb.npy")
    c = np.load(tmp_path / "a" / "rgb.npy")
    assert a.shape == (1000,) and np.array_equal(a.astype(np.int32), f.reshape(-1)[i])
    assert c.shape == (1000, 3) and np.array_equal(c.astype(np.uint8), rt.argb_to_rgb8(f.reshape(-1)[i]))


def test_plain_run_is_the_default():
    import sys
    from unittest import mock

    seen = {}

    def stop(args):
        seen.update(vars(args))
        return 0

    with mock.patch.object(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "7"]), \
            mock.patch.object(bench, "launch_ranks", stop), mock.patch.dict("os.environ"):
        import os
        os.environ.pop("WORLD_SIZE", None)
        with pytest.raises(SystemExit) as e:
            bench.main()
    assert e.value.code == 0
    assert seen["full"] is False and seen["dump_outputs"] is None and seen["steps"] == 7


@pytest.mark.gpu
def test_device_frame_read_back():
    import torch

    f = _frame(19, 31)
    t = torch.from_numpy(f).to("cuda")
    torch.cuda.synchronize()
    got = bench.device_frame_to_host(t.data_ptr(), 19, 31, t.device.index)
    assert got.dtype == np.int32 and np.array_equal(got, f)
