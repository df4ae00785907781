#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of task_barrier_kernel's TAIL == false
instantiations (the context's launches, cbx_step_and_synchronise) between two
builds of crossbow_amd/csrc/task_barrier_kernels.hip, kernel by kernel.

Each input is the device assembly of one build, cross-compiled without a GPU:

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off \
      -cuid=crossbow_task_barrier_kernels -I include --cuda-device-only -S \
      -o OUT.s crossbow_amd/csrc/task_barrier_kernels.hip

The older build has no TAIL template parameter; the newer one's kernels are
matched to it by dropping that parameter (the 8th) from the mangled name.  An
instruction may differ only in one immediate that is an offset into the hidden
kernel arguments: at or past the older argument block's size, and moved by
exactly the growth of the block.  Anything else is reported and fails.

Usage: python scripts/compare_task_barrier_asm.py OLD.s NEW.s
"""
from __future__ import annotations

import re
import sys

NAME = re.compile(r"^(_ZN3cbx\S*task_barrier_kernelI\S+):\s*(;.*)?$")
IMM = re.compile(r"\b(0x[0-9a-fA-F]+|\d+)\b")


def kernels(path):
    """{mangled name: [instruction lines]} and {name: kernel-argument bytes, hidden ones included}."""
    out, size, cur, described = {}, {}, None, None
    with open(path) as f:
        for line in f:
            m = NAME.match(line)
            if m:
                cur = m.group(1)
                out[cur] = []
                continue
            s = line.split(";", 1)[0].rstrip()
            if cur and s.startswith(".Lfunc_end"):
                cur = None
            elif cur and (s.startswith(".LBB") or (s.startswith("\t") and not s.lstrip().startswith("."))):
                # block labels carry the function's number in the file: .LBB331_5 -> .LBB_5
                out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
            m = re.match(r"\s*\.amdhsa_kernarg_size\s+(\d+)", line)
            if m and described:
                size[described] = int(m.group(1))
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                described = m.group(1)
    return out, size


def without_tail(name):
    """The older name of a TAIL == false kernel, or None for a TAIL kernel."""
    m = re.match(r"^(.*task_barrier_kernelI)((?:L[ib]\d+E|Lin\d+E)+)(E.*)$", name)
    args = re.findall(r"L[ib]n?\d+E", m.group(2))
    if len(args) != 9:
        raise SystemExit(f"{name}: expected 9 template arguments, found {len(args)}")
    if args[7] != "Lb0E":
        return None
    return m.group(1) + "".join(args[:7] + args[8:]) + m.group(3)


def same(a, b, old_size, grow):
    if a == b:
        return True
    ia, ib = IMM.findall(a), IMM.findall(b)
    if IMM.sub("#", a) != IMM.sub("#", b) or len(ia) != len(ib):
        return False
    moved = [(int(x, 0), int(y, 0)) for x, y in zip(ia, ib) if x != y]
    return len(moved) == 1 and moved[0][0] >= old_size and moved[0][1] == moved[0][0] + grow


def main():
    old, old_size = kernels(sys.argv[1])
    new, new_size = kernels(sys.argv[2])
    compared = moved = tails = 0
    bad = []
    for name, body in sorted(new.items()):
        twin = without_tail(name)
        if twin is None:
            tails += 1
            continue
        if twin not in old:
            bad.append(f"{name}: no kernel {twin} in the older build")
            continue
        grow = new_size[name] - old_size[twin]
        ref = old[twin]
        compared += 1
        if len(ref) != len(body):
            bad.append(f"{name}: {len(ref)} instructions before, {len(body)} now")
            continue
        for k, (a, b) in enumerate(zip(ref, body)):
            if not same(a, b, old_size[twin] - 256, grow):
                bad.append(f"{name}: instruction {k}: `{a}` became `{b}`")
                break
            moved += a != b
    missing = set(old) - {without_tail(n) for n in new}
    for name in sorted(missing):
        bad.append(f"{name}: gone from the newer build")
    sizes = sorted({(old_size[without_tail(n)], new_size[n]) for n in new if without_tail(n) in old_size})
    print(f"{compared} TAIL == false kernels compared with the older build's {len(old)}, "
          f"{tails} TAIL kernels beside them; kernel-argument size (with the hidden arguments) {sizes}; {moved} instructions differ only in a "
          f"hidden-argument offset; {len(bad)} other differences")
    for line in bad[:20]:
        print("  " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
