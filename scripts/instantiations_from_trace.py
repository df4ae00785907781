#!/usr/bin/env python3
"""Reduce a rocprofv3 kernel trace of tests/test_gpu_instantiations.py to the
record tests/test_instantiations.py checks the dispatch model against:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- \\
        python -m pytest tests/test_gpu_instantiations.py -m gpu
    python scripts/instantiations_from_trace.py OUT --num-cus 256 --commit $(git rev-parse HEAD)

writes profiles/instantiations/launched.json: the library's kernels the run
launched (demangled, normalised as tests/instantiations.py names them) with
launch counts, the commit the tree stood on, and the device's CU count.
Kernels of other libraries (torch, RCCL) are counted, not listed.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.instantiations import normalise  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", help="a *_kernel_trace.csv, or a directory searched for them")
    ap.add_argument("--num-cus", type=int, required=True, help="compute units of the traced device")
    ap.add_argument("--commit", required=True, help="the commit the traced tree stood on")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "instantiations", "launched.json"))
    a = ap.parse_args()
    files = [a.trace] if os.path.isfile(a.trace) else sorted(
        glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        print(f"no *kernel_trace.csv under {a.trace}", file=sys.stderr)
        return 1
    ours, other = Counter(), 0
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("kernel_name") or ""
                if "cbx::" in name:
                    ours[normalise(name)] += 1
                else:
                    other += 1
    rec = {"commit": a.commit, "num_cus": a.num_cus, "traced": "tests/test_gpu_instantiations.py",
           "launches": sum(ours.values()), "other_kernel_launches": other,
           "kernels": {k: ours[k] for k in sorted(ours)}}
    os.makedirs(os.path.dirname(a.output), exist_ok=True)
    with open(a.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(ours)} kernels of the library, {rec['launches']} launches ({other} of other libraries) -> {a.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
