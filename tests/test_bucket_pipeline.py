"""The bucketed all-reduce pipeline without a GPU: the two bucket-geometry
rules, the narrowing of an argument struct to one bucket and the order in
which a step's kernels, collectives, records and waits are enqueued
(crossbow_amd/csrc/bucket_pipeline.h), driven by a stand-alone program under
ASan + UBSan with lanes that only record what they are asked to do."""
from __future__ import annotations

import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_pipeline_order_and_geometry_under_asan_and_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bucket_pipeline_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "crossbow_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "bucket_pipeline_test.cpp")],
                       check=True, capture_output=True, timeout=240)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.startswith("ok "), p.stdout
