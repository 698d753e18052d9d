"""The compiler's resource record of every kernel of the library, and its comparison with another build's.

Compiles every .hip translation unit with build.py's flags plus -Rpass-analysis=kernel-resource-usage (no
object is kept) and collects, per kernel, SGPRs, VGPRs, AGPRs, spills, scratch, occupancy and static LDS.

    python tools/kernel_resources.py --out records.json            # this tree's records
    python tools/kernel_resources.py --logs DIR --out records.json # from saved compiler output, DIR/<unit>.log
    python tools/kernel_resources.py --out new.json --parent parent.json --report profiles/adaptive_kernels.json
        also writes the record-by-record comparison: kernels only in this build (listed in full), kernels only
        in the parent, and every kernel of both whose record differs.
"""
import argparse
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from distraytracer_old_amd import build  # noqa: E402

FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
          "LDS Size [bytes/block]": "lds_bytes_per_block_static"}


def parse(text):
    """compiler output -> {mangled kernel name: record}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: (?:.*?:\d+:\d+: )?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: (?:.*?:\d+:\d+: )?\s*([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[FIELDS[m.group(1).strip()]] = int(m.group(2))
    return out


def compile_units():
    units = [s for s in build.SOURCES if s.endswith(".hip")]
    procs = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in units:
            cmd = [build.HIPCC, *build.COMPILE_FLAGS, *build.SOURCE_FLAGS.get(src, []), "-Rpass-analysis=kernel-resource-usage", "-c",
                   str(build.CSRC / src), "-o", str(Path(tmp) / (src + ".o"))]
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
        logs = {}
        for src, pr in procs:
            logs[src] = pr.communicate()[1]
            if pr.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}:\n" + logs[src][-2000:])
    return logs


def demangled(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    d = r.stdout.splitlines() if r.returncode == 0 else []
    return dict(zip(names, d)) if len(d) == len(names) else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--logs", help="a directory of saved compiler output, <unit>.log, instead of compiling")
    ap.add_argument("--parent", help="another build's records (this tool's --out) to compare against")
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.logs:
        logs = {p.stem + ".hip": p.read_text() for p in sorted(Path(a.logs).glob("*.log"))}
    else:
        logs = compile_units()
    rec = {"build_id": build.build_id() if not a.logs else None, "units": {u: parse(t) for u, t in logs.items()}}
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(a.out, sum(len(v) for v in rec["units"].values()), "kernel records")
    if not a.parent:
        return
    par = json.loads(Path(a.parent).read_text())
    names = sorted({k for u in rec["units"].values() for k in u} | {k for u in par["units"].values() for k in u})
    dm = demangled(names)
    added, removed, differing, same = [], [], [], 0
    for u in sorted(set(rec["units"]) | set(par["units"])):
        new, old = rec["units"].get(u, {}), par["units"].get(u, {})
        for k in sorted(set(new) | set(old)):
            if k not in old:
                added.append({"unit": u, "kernel": dm[k], **new[k]})
            elif k not in new:
                removed.append({"unit": u, "kernel": dm[k]})
            elif new[k] != old[k]:
                differing.append({"unit": u, "kernel": dm[k], "parent": old[k], "this_build": new[k]})
            else:
                same += 1
    rep = {"build_id": rec["build_id"] or build.build_id(), "parent_build_id": par.get("build_id"),
           "source": "hipcc -Rpass-analysis=kernel-resource-usage on every translation unit with build.py's flags (gfx950), this build "
                     "and its parent (tools/kernel_resources.py)",
           "compared": "SGPRs, VGPRs, AGPRs, spills, scratch, occupancy and static LDS of every kernel record of both builds, by "
                       "translation unit and mangled name",
           "records_parent": sum(len(v) for v in par["units"].values()),
           "records_this_build": sum(len(v) for v in rec["units"].values()),
           "records_identical": same, "records_differing": differing, "records_only_in_parent": removed,
           "per_unit": {u: {"parent": len(par["units"].get(u, {})), "this_build": len(rec["units"].get(u, {}))}
                        for u in sorted(set(rec["units"]) | set(par["units"]))},
           "new_kernels": added}
    if a.report:
        Path(a.report).write_text(json.dumps(rep, indent=1) + "\n")
    print("identical", same, "differing", len(differing), "only in parent", len(removed), "new", len(added))


if __name__ == "__main__":
    main()
