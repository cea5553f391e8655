#!/usr/bin/env python3
"""Tabulates per-kernel resources from hipcc's -Rpass-analysis=kernel-resource-usage remarks.

usage: resource_table.py PARENT_BUILD_LOG NEW_BUILD_LOG OUT_JSON
(each log: `make -B EXTRA=-Rpass-analysis=kernel-resource-usage` in hivemind_amd/csrc at that commit, stderr included; the objects of
hm_rollout.hip must be built one at a time or with make's -O so that their remarks do not interleave).  Exit status 1 when VGPRs,
VGPR spill, scratch, LDS or occupancy differ for any kernel; SGPR-spill differences are listed only."""
import json
import re
import subprocess
import sys

KEYS = {"VGPRs": "vgprs", "AGPRs": "agprs", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill", "ScratchSize [bytes/lane]": "scratch",
        "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
MUST = ("vgprs", "vgpr_spill", "scratch", "lds", "occupancy")
FILES = re.compile(r"^(hm_net\w*|hm_rollout|hm_search)\.hip$")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"(\S+?):\d+:\d+: remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        src, text = m.group(1), m.group(2)
        if text.startswith("Function Name: "):
            cur = None
            if FILES.match(src):
                # the three objects of hm_rollout.hip hold the same symbol names: number the repeats in order of appearance
                base = src + "::" + text[len("Function Name: "):]
                k = 0
                while f"{base}#{k}" in out:
                    k += 1
                cur = out.setdefault(f"{base}#{k}", {})
        elif cur is not None and ": " in text:
            k, v = text.split(": ", 1)
            if k in KEYS:
                cur[KEYS[k]] = int(v)
    return out


def main():
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(parent) | set(new))
    try:
        dem = dict(zip(names, subprocess.run(["c++filt"] + [n.split("::", 1)[1].rsplit("#", 1)[0] for n in names], capture_output=True, text=True, check=True).stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        dem = {}
    rows, blocking, sgpr = [], [], []
    for n in names:
        p, q = parent.get(n), new.get(n)
        rows.append({"kernel": n, "demangled": dem.get(n, ""), "parent": p, "new": q})
        if p is None or q is None or any(p.get(k) != q.get(k) for k in MUST):
            blocking.append(n)
        elif p.get("sgpr_spill") != q.get("sgpr_spill"):
            sgpr.append(n)
    json.dump({"kernels": len(names), "differ_blocking": blocking, "differ_sgpr_spill_only": sgpr, "rows": rows}, open(sys.argv[3], "w"), indent=1)
    print(f"{len(names)} kernels; blocking differences: {len(blocking)}; SGPR-spill-only differences: {len(sgpr)}")
    for n in blocking + sgpr:
        print(" ", dem.get(n, n)[:110], "\n     parent", parent.get(n), "\n     new   ", new.get(n))
    return 1 if blocking else 0


if __name__ == "__main__":
    sys.exit(main())
