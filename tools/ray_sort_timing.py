"""What RT_TRACE_SORT costs and gains on the C3 scene (rt_trace_rays_device): every workload traced with and
without the flag in the same run, alternating, timed with device events after a warm-up, median of 5.

Workloads (2^22 camera rays of a 2048 x 2048 un-jittered frame; the secondary rays start at their hit points):
  camera     the camera rays row-major                                         closest, any
  shuffled   the same rays permuted                                            closest, any
  shadow     hit point -> the scene's first light, tmax = distance, permuted   any
  hemi       cosine-weighted directions about the hit normal, permuted         closest, any

    python tools/ray_sort_timing.py [--out FILE] [--log2n 22]
        event times: unsorted, sorted, and the order alone (rt_trace_order_device: bounds + keys + sort);
        then the incoherent rows again (packet mode) over the key's bit split: origin-cell and direction bits
        per axis (DISTRAYTRACER_SORT_ORG_BITS / _DIR_BITS). Writes profiles/ray_sort_timing.json.
    rocprofv3 --kernel-trace -d DIR -o sort --output-format csv -- python tools/ray_sort_timing.py --split
    python tools/ray_sort_timing.py --merge DIR/.../sort_kernel_trace.csv [--out FILE]
        the sorted call's kernel time split into bounds + keys / sort / trace: --split runs the sorted traces
        alone (packet mode, a warm-up and 5 of each workload, in a fixed sequence), --merge cuts the kernel
        trace at every indexed query kernel and adds the medians to the file.
"""
import argparse
import csv
import json
import math
import os
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from distraytracer_old_amd import desc, rt, scenes  # noqa: E402

LIGHT = np.array([3.0, 4.0, 0.0])  # c3_bun69k.cli: the first point_light
ROWS = [("camera", "closest"), ("camera", "any"), ("shuffled", "closest"), ("shuffled", "any"), ("shadow", "any"),
        ("hemi", "closest"), ("hemi", "any")]
REPS = 5
SWEEP = [(6, 8), (6, 12), (6, 16), (8, 12), (10, 12), (10, 8), (10, 4)]  # (origin, direction) bits per axis


def camera_rays(side):
    view_z = -1 * (side / 2.0) / math.tan((math.pi * 60.0 / 180.0) / 2)
    col, row = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    d = np.stack([col - side / 2.0, -1 * (row - side / 2.0), np.full((side, side), view_z)], -1).reshape(-1, 3)
    return rt.rays(np.zeros_like(d), d, np.inf)


def workloads(g, side, torch, dev):
    """name -> (device rays as a uint8 tensor, ray count)."""
    cam = camera_rays(side)
    n = len(cam)
    rng = np.random.default_rng(1)
    hits = g.trace(cam["o"], cam["d"])
    ok = (hits["flags"] & rt.HIT_HIT) != 0
    pos, nrm = hits["pos"][ok], hits["normal"][ok]
    nrm = np.where((nrm * cam["d"][ok]).sum(1, keepdims=True) > 0, -nrm, nrm)  # facing the camera ray
    to_light = LIGHT - pos
    shadow = rt.rays(pos, to_light, np.linalg.norm(to_light, axis=1))
    # cosine-weighted hemisphere about the normal: a unit-disk sample lifted, in a frame of the normal
    u1, u2 = rng.random(len(pos)), rng.random(len(pos))
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(nrm[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t = np.cross(nrm, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    hemi_d = t * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + nrm * np.sqrt(1 - u1)[:, None]
    hemi = rt.rays(pos, hemi_d, np.inf)
    w = {"camera": cam, "shuffled": cam[rng.permutation(n)], "shadow": shadow[rng.permutation(len(pos))],
         "hemi": hemi[rng.permutation(len(pos))]}
    return {k: (torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to(dev), len(v)) for k, v in w.items()}


def timed(fn, st, torch, reps=REPS):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def measure(g, w, rows, travs, st, torch, hits, occ, order):
    """Event times of each row: unsorted and sorted alternating, then the order alone."""
    out = []
    for trav, tf in travs:
        for name, query in rows:
            t_rays, n = w[name]
            qf = rt.TRACE_ANY if query == "any" else 0

            def go(extra):
                g.trace_device(t_rays.data_ptr(), n, hits_ptr=0 if qf else hits.data_ptr(), occ_ptr=occ.data_ptr() if qf else 0,
                               stream=st.cuda_stream, flags=tf | qf | extra)
            go(0), go(rt.TRACE_SORT)  # warm-up of both (and the sort scratch's allocation)
            st.synchronize()
            plain, srt = [], []
            for _ in range(REPS):
                plain += timed(lambda: go(0), st, torch, 1)
                srt += timed(lambda: go(rt.TRACE_SORT), st, torch, 1)
            g.trace_order_device(t_rays.data_ptr(), n, order.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            ordr = timed(lambda: g.trace_order_device(t_rays.data_ptr(), n, order.data_ptr(), stream=st.cuda_stream), st, torch)
            row = {"traversal": trav, "workload": name, "query": query, "rays": n,
                   "unsorted_ms": statistics.median(plain), "unsorted_ms_all": plain,
                   "sorted_ms": statistics.median(srt), "sorted_ms_all": srt,
                   "order_ms": statistics.median(ordr), "order_ms_all": ordr}
            row["speedup"] = row["unsorted_ms"] / row["sorted_ms"]
            out.append(row)
            print(f"{trav:7s} {name:9s} {query:8s} {n:8d} rays  unsorted {row['unsorted_ms']:8.3f} ms  sorted "
                  f"{row['sorted_ms']:8.3f} ms (order {row['order_ms']:.3f})  x{row['speedup']:.2f}", flush=True)
    return out


def merge(csv_path, out_path):
    """Cut the kernel trace of a --split run at every indexed query kernel: one segment per sorted call."""
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {"bounds_keys": 0.0, "sort": 0.0, "trace": 0.0}
    for r in rows:
        name, ms = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "query_kernel_idx" in name:
            cur["trace"] = ms
            calls.append(cur)
            cur = {"bounds_keys": 0.0, "sort": 0.0, "trace": 0.0}
        elif "bounds_kernel" in name or "key_kernel" in name:
            cur["bounds_keys"] += ms
        elif "rocprim" in name:
            cur["sort"] += ms
    assert len(calls) == len(ROWS) * (1 + REPS), (len(calls), "sorted calls in the trace")
    split = []
    for i, (name, query) in enumerate(ROWS):
        seg = calls[i * (1 + REPS) + 1:(i + 1) * (1 + REPS)]  # without the warm-up
        row = {"workload": name, "query": query, **{k: statistics.median(c[k] for c in seg) for k in seg[0]}}
        split.append(row)
        print(row)
    out = json.loads(Path(out_path).read_text())
    out["kernel_split_ms"] = {"source": "rocprofv3 --kernel-trace of the --split run (packet mode), median of 5 sorted calls",
                              "rows": split}
    Path(out_path).write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "ray_sort_timing.json"))
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--merge", metavar="CSV")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    import torch

    cli = scenes.CONFIGS["C3"][0]
    side = 1 << (a.log2n // 2)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    with rt.Scene.load_cli(cli) as g:
        w = workloads(g, side, torch, dev)
        nmax = max(n for _, n in w.values())
        hits = torch.zeros(nmax * desc.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        occ = torch.zeros(nmax, dtype=torch.uint8, device=dev)
        order = torch.zeros(nmax, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        if a.split:  # nothing but the sorted traces from here on: --merge counts them
            for name, query in ROWS:
                t_rays, n = w[name]
                qf = rt.TRACE_ANY if query == "any" else 0
                for _ in range(1 + REPS):
                    g.trace_device(t_rays.data_ptr(), n, hits_ptr=0 if qf else hits.data_ptr(),
                                   occ_ptr=occ.data_ptr() if qf else 0, stream=st.cuda_stream, flags=qf | rt.TRACE_SORT)
                    st.synchronize()
            return
        table = measure(g, w, ROWS, (("packet", 0), ("lanes", rt.TRACE_LANES)), st, torch, hits, occ, order)
    key_bits = []
    for ob, db in SWEEP:  # the key's bits per axis of the origin cell and of the direction, read at scene creation
        os.environ["DISTRAYTRACER_SORT_ORG_BITS"], os.environ["DISTRAYTRACER_SORT_DIR_BITS"] = str(ob), str(db)
        with rt.Scene.load_cli(cli) as g:
            sub = [r for r in ROWS if r[0] != "camera"]
            print(f"key: {ob} origin bits, {db} direction bits per axis")
            for row in measure(g, w, sub, (("packet", 0),), st, torch, hits, occ, order):
                key_bits.append({"org_bits": ob, "dir_bits": db, **{k: v for k, v in row.items() if not k.startswith("unsorted")}})
    del os.environ["DISTRAYTRACER_SORT_ORG_BITS"], os.environ["DISTRAYTRACER_SORT_DIR_BITS"]
    out = {"build_id": rt.build_id(), "scene": cli, "reps": REPS, "device": torch.cuda.get_device_name(0),
           "key_bits_default": "the library's (csrc/query.hip trace_init)", "table": table, "key_bits": key_bits}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
