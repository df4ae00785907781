"""Build the native pieces of crossbow_amd in-tree.

* ``crossbow_amd/libcrossbow_sma.so``  -- the C-ABI library (hipcc, gfx950):
  csrc/context.hip + csrc/sync_steps.hip + csrc/sma_kernels.hip +
  csrc/averaging_kernels.hip + csrc/sma_seam.hip + csrc/stats_kernels.hip +
  csrc/variable_rate_kernels.hip + csrc/clip_kernels.hip +
  csrc/task_barrier_kernels.hip, linked against RCCL and against
* ``crossbow_amd/libcrossbow_sma_variables.so`` -- the fused task-step barrier
  with a learning rate per variable (csrc/task_barrier_variables_kernels.hip):
  a shared object of its own, built first, so the device code of
  ``libcrossbow_sma.so`` (``code_object_digest``) stays what it was.
* ``crossbow_amd/libcrossbow_sma_clipped.so`` -- the fused task-step barrier
  with gradient clipping (csrc/task_barrier_clipped_kernels.hip): likewise a
  shared object of its own, built first and linked by the library.
* ``crossbow_amd/libcrossbow_sma_clipped_variables.so`` -- the fused task-step
  barrier with both (csrc/task_barrier_clipped_variables_kernels.hip): likewise.
* ``crossbow_amd/libcrossbow_sma_elastic_steps.so`` -- the task steps fused into
  the elastic-averaging barrier (csrc/task_elastic_kernels.hip): likewise.
* ``crossbow_amd/libcrossbow_sma_ssgd_steps.so`` -- the task steps fused into
  the synchronous-SGD barrier (csrc/task_ssgd_kernels.hip): likewise.
* ``crossbow_amd/libcrossbow_sma_elastic_policies.so`` -- the per-variable, the
  clipped and the clipped per-variable task steps fused into the
  elastic-averaging barrier (csrc/task_elastic_variables_kernels.hip,
  csrc/task_elastic_clipped_kernels.hip,
  csrc/task_elastic_clipped_variables_kernels.hip, one compilation unit per
  policy): likewise.
* ``crossbow_amd/libGPU.so``           -- the JNI shim exporting Crossbow's
  ``TheGPU`` model-path natives; built only where ``jni.h`` exists (there is
  no JDK in this image).

Usage: ``python -m crossbow_amd.build [--force]``.
"""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libcrossbow_sma.so")
VARIABLES_LIB = os.path.join(PKG, "libcrossbow_sma_variables.so")
CLIPPED_LIB = os.path.join(PKG, "libcrossbow_sma_clipped.so")
CLIPPED_VARIABLES_LIB = os.path.join(PKG, "libcrossbow_sma_clipped_variables.so")
ELASTIC_STEPS_LIB = os.path.join(PKG, "libcrossbow_sma_elastic_steps.so")
SSGD_STEPS_LIB = os.path.join(PKG, "libcrossbow_sma_ssgd_steps.so")
ELASTIC_POLICIES_LIB = os.path.join(PKG, "libcrossbow_sma_elastic_policies.so")
JNI_LIB = os.path.join(PKG, "libGPU.so")
ARCH = "gfx950"


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the MI355X library needs ROCm's hipcc")


SOURCES = ("context.hip", "sync_steps.hip", "sma_kernels.hip", "averaging_kernels.hip", "sma_seam.hip",
           "stats_kernels.hip", "variable_rate_kernels.hip", "clip_kernels.hip", "task_barrier_kernels.hip")
VARIABLES_SOURCES = ("task_barrier_variables_kernels.hip",)
CLIPPED_SOURCES = ("task_barrier_clipped_kernels.hip",)
CLIPPED_VARIABLES_SOURCES = ("task_barrier_clipped_variables_kernels.hip",)
ELASTIC_STEPS_SOURCES = ("task_elastic_kernels.hip",)
SSGD_STEPS_SOURCES = ("task_ssgd_kernels.hip",)
ELASTIC_POLICIES_SOURCES = ("task_elastic_clipped_variables_kernels.hip", "task_elastic_clipped_kernels.hip",
                            "task_elastic_variables_kernels.hip")
HEADERS = ("context_internal.h", "sma_internal.h", "stream_helpers.h", "stats_internal.h", "stats_plan.h",
           "optimise_plan.h", "clip_internal.h", "bucket_pipeline.h", "task_ssgd_internal.h",
           # the fused task-step barrier's four kernel files are one text
           "task_barrier_step.h", "task_barrier_body.inc", "task_barrier_launch.h",
           # and so are the three policy kernels of the fused elastic-averaging barrier
           "task_elastic_policy.h", "task_elastic_policy_body.inc")


def _sources(names=SOURCES):
    return [os.path.join(CSRC, f) for f in names]


def _deps():
    return (_sources() + _sources(VARIABLES_SOURCES) + _sources(CLIPPED_SOURCES) +
            _sources(CLIPPED_VARIABLES_SOURCES) + _sources(ELASTIC_STEPS_SOURCES) + _sources(SSGD_STEPS_SOURCES) +
            _sources(ELASTIC_POLICIES_SOURCES) +
            [os.path.join(CSRC, f) for f in HEADERS] + [os.path.join(ROOT, "include", "crossbow_sma.h"),
                                                        os.path.abspath(__file__)])


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _jobs() -> int:
    """Compilations at a time: $MAX_JOBS, else the CPUs this process may use, 16 at the most."""
    try:
        n = int(os.environ.get("MAX_JOBS", ""))
    except ValueError:
        n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(n, 16))


def _compile_one(src, objdir, verbose):
    stem = os.path.splitext(os.path.basename(src))[0]
    obj = os.path.join(objdir, stem + ".o")
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall",
           # A fixed compilation-unit id per source instead of one hashed from
           # its path: the device code (and code_object_digest) is then the
           # same wherever the tree is built.
           f"-cuid=crossbow_{stem}",
           # fp32 results must equal the reference's cuBLAS op order bit for bit: every
           # fma is written explicitly, nothing may be contracted behind our back.
           "-ffp-contract=off",
           "-I", os.path.join(ROOT, "include"), "-c", "-o", obj, src]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return obj


def _compile(sources, objdir, verbose):
    """One object per source, in the sources' order; the compilations run side
    by side (each is one hipcc process), the first failure is raised."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=_jobs()) as pool:
        return list(pool.map(lambda src: _compile_one(src, objdir, verbose), sources))


def _link(target, objs, libs, verbose):
    tmp = target + ".tmp"
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-shared", "-o", tmp] + objs + libs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(tmp, target)


def build_lib(force: bool = False, verbose: bool = False) -> str:
    # one staleness check for all seven libraries: they share the headers
    if not force and not any(_stale(t, _deps()) for t in (LIB, VARIABLES_LIB, CLIPPED_LIB, CLIPPED_VARIABLES_LIB,
                                                          ELASTIC_STEPS_LIB, SSGD_STEPS_LIB, ELASTIC_POLICIES_LIB)):
        return LIB
    objdir = os.path.join(PKG, "build")
    os.makedirs(objdir, exist_ok=True)
    # every source of the seven objects is compiled in one pool, the slowest (the barrier kernels) first
    groups = (VARIABLES_SOURCES, CLIPPED_SOURCES, CLIPPED_VARIABLES_SOURCES, ELASTIC_STEPS_SOURCES, SSGD_STEPS_SOURCES,
              ELASTIC_POLICIES_SOURCES, tuple(reversed(SOURCES)))
    objs = _compile([src for names in groups for src in _sources(names)], objdir, verbose)
    side = (len(VARIABLES_SOURCES), len(CLIPPED_SOURCES), len(CLIPPED_VARIABLES_SOURCES), len(ELASTIC_STEPS_SOURCES),
            len(SSGD_STEPS_SOURCES), len(ELASTIC_POLICIES_SOURCES))
    at = [sum(side[:k]) for k in range(7)]
    # the objects of the per-variable, the clipped and the clipped per-variable fused barrier, of the fused
    # elastic-averaging and synchronous-SGD barriers and of the former's policies first: the library links against them
    _link(VARIABLES_LIB, objs[at[0]:at[1]], [], verbose)
    _link(CLIPPED_LIB, objs[at[1]:at[2]], [], verbose)
    _link(CLIPPED_VARIABLES_LIB, objs[at[2]:at[3]], [], verbose)
    _link(ELASTIC_STEPS_LIB, objs[at[3]:at[4]], [], verbose)
    _link(SSGD_STEPS_LIB, objs[at[4]:at[5]], [], verbose)
    _link(ELASTIC_POLICIES_LIB, objs[at[5]:at[6]], [], verbose)
    _link(LIB, list(reversed(objs[at[6]:])),
          ["-L", PKG, "-lcrossbow_sma_variables", "-lcrossbow_sma_clipped", "-lcrossbow_sma_clipped_variables",
           "-lcrossbow_sma_elastic_steps", "-lcrossbow_sma_ssgd_steps", "-lcrossbow_sma_elastic_policies",
           "-Wl,-rpath,$ORIGIN", "-lrccl", "-lrocprofiler-sdk-roctx", "-lpthread"],
          verbose)
    return LIB


def code_object_digest(path: str = LIB) -> str:
    """sha256 of the library's device code (its ``.hip_fatbin`` section: the
    gfx950 code objects of every kernel).  profiles/traffic.json stores it
    with each PMC measurement, and bench.py reports a measured HBM traffic
    only for the code object that is running (else null, with the reason)."""
    import hashlib
    import struct
    with open(path, "rb") as f:
        elf = f.read()
    if elf[:4] != b"\x7fELF" or elf[4] != 2:
        raise ValueError(f"{path}: not an ELF64 file")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)

    def section(i):
        name, _, _, _, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
        return name, off, size

    _, stroff, _ = section(shstrndx)
    for i in range(shnum):
        name, off, size = section(i)
        end = elf.index(b"\0", stroff + name)
        if elf[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(elf[off:off + size]).hexdigest()
    raise ValueError(f"{path}: no .hip_fatbin section")


def find_jni_include():
    cands = []
    jh = os.environ.get("JAVA_HOME")
    if jh:
        cands.append(os.path.join(jh, "include"))
    cands += glob.glob("/usr/lib/jvm/*/include")
    for c in cands:
        if os.path.exists(os.path.join(c, "jni.h")):
            return c
    return None


def build_jni(force: bool = False, verbose: bool = False):
    """Build libGPU.so (the JNI drop-in) when a JDK is present; else None."""
    inc = find_jni_include()
    if inc is None:
        return None
    src = os.path.join(CSRC, "jni", "TheGPU_jni.c")
    if not force and not _stale(JNI_LIB, [src, LIB]):
        return JNI_LIB
    cmd = ["gcc", "-O2", "-fPIC", "-shared", "-I", inc, "-I", os.path.join(inc, "linux"),
           "-I", os.path.join(ROOT, "include"), "-o", JNI_LIB, src, "-L", PKG, "-lcrossbow_sma",
           "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return JNI_LIB


def build(force: bool = False, verbose: bool = False) -> str:
    lib = build_lib(force, verbose)
    build_jni(force, verbose)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
