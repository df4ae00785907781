"""The task steps fused into the synchronous-SGD barrier on IEEE edge values
(run with -m gpu): the catalogue of tests/edge_values.py through
cbx_ssgd_plan_step_and_optimise and cbx_step_and_synchronise_ssgd, held to
rules 1-3 of DESIGN.md's edge-value contract: bits equal off NaN, NaN-ness
equal, and what is a copy or is not written exact to the bit (every receiving
``w`` the device's own ``z``, the accumulator +0, an unwritten ``g`` its input,
signalling NaNs included).

The catalogue is put together from that file's blocks for this kernel's
operands: signed zeros and the sweep over z, the base last, the accumulator and
``w`` and ``g`` of every stepping replica; the task step's blocks
(``optimiser_scenarios`` with the accumulator as its extra operand) for the
first two stepping replicas; the barrier's blocks (``ssgd_sync_scenarios``) with
the stepping replicas' ``g`` and ``w`` at +0, so that the accumulator reaches
the barrier as the scenario wrote it.  It lies twice in every buffer: in the
float4 bulk and in the last n mod 1,024 floats, the seam's tail.  The rates are
each replica's own and non-zero, the ratio is 1/6, base momentum and weight
decay are either off (the kernel then holds nothing of them) or 0.9 and 5e-4:
none an exact 0 where it is used.  The oracle's output is checked to hold NaNs
in less than a quarter of every compared array before the device is compared.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_values as E
from tests.helpers import assert_bitexact
from tests.test_gpu_edge_values import MASKS
from tests.test_gpu_seam_step_and_optimise import DISCARD
from tests.test_gpu_seam_step_and_optimise_ssgd import SsgdBuffers, SsgdData
from tests.test_gpu_step_and_synchronise import _exp, _rates
from tests.test_gpu_step_and_synchronise_ssgd import SsgdCase, _sgpu

pytestmark = pytest.mark.gpu

N, WD, WPC = E.N, E.WD, 6
# (base momentum, weight decay)
CONFIGS = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0), "wd-only": (0.0, WD), "mom-only": (0.9, 0.0)}


def scenarios(base_last, wd, rates, steps):
    stepping = [i for i, s in enumerate(steps) if s]
    base = ["z"] + (["last"] if base_last else []) + ["acc"]
    names = base + [f"{k}{i}" for i in stepping for k in ("w", "g")]
    cover = [x for x in ("z", "last", "acc", f"w{stepping[0]}", f"g{stepping[0]}", f"g{stepping[1]}") if x in names]
    out = E.signed_zeros(names, cover) + E.sweep(names)
    for i in stepping[:2]:  # past the sweep of (w, g, acc), which the line above holds already
        out += E.optimiser_scenarios(-rates[i], 0.0, wd, f"w{i}", f"g{i}", None, extra=("acc",),
                                     zeros=False)[3 * len(E.SWEEP):]
    still = {f"{k}{i}": E.PZERO for i in stepping for k in ("w", "g")}  # fma(rate, +0, acc) is acc
    for label, vals in E.ssgd_sync_scenarios(base_last, WPC)[2 ** len(base) + len(base) * len(E.SWEEP):]:
        out.append(("barrier: " + label, {**still, **vals}))
    small = {"z": 0x00200000 | E.SIGN, "l": 0x00000100, "a": 0x00300000, "w": E.MAX_SUB, "g": 0x00400000}
    out.append(("every operand subnormal", {x: small[x[0]] for x in names}))
    return out


def write_catalogue(d, wd, rates, steps):
    st = d.st
    arrays = {"z": st.z[0], "acc": d.acc}
    if st.last is not None:
        arrays["last"] = st.last[0]
    for i in range(st.size):
        if steps[i]:
            arrays[f"w{i}"], arrays[f"g{i}"] = st.w[i], d.g[i]
    return E.apply(arrays, scenarios(st.last is not None, wd, rates, steps))


def check(read, d, d0, labels, steps, wd, keep):
    """`read(kind, i)`: the device's buffer (kind in z, blast, acc, w, g); d the
    mirror after the oracle's step, d0 before it."""
    st = d.st
    arrays = {"z": st.z[0], **{f"w[{i}]": st.w[i] for i in range(st.size)}, **{f"g[{i}]": d.g[i] for i in range(st.size)}}
    if st.last is not None:
        arrays["base last"] = st.last[0]
    for name, a in arrays.items():
        assert E.nan_fraction(a) < 0.25, f"the oracle's {name} holds {E.nan_fraction(a):.2%} NaNs"
    assert any(label and "every operand subnormal" in label for label in labels)
    z = read("z", 0)
    E.assert_edge_equal(z, st.z[0], "z", labels)
    if st.last is not None:
        E.assert_edge_equal(read("blast", 0), st.last[0], "base last", labels)
    assert_bitexact(read("acc", 0), np.zeros(N, np.float32), "acc is reset to +0")
    assert_bitexact(d.acc, np.zeros(N, np.float32), "the oracle's acc")
    for i in range(st.size):
        w = read("w", i)
        E.assert_edge_equal(w, st.w[i], f"w[{i}]", labels)
        assert_bitexact(w, z, f"w[{i}] is a copy of the device's z")
        if steps[i] and keep and wd > 0:
            E.assert_edge_equal(read("g", i), d.g[i], f"g[{i}]", labels)
        else:
            assert_bitexact(read("g", i), d0.g[i], f"g[{i}] is not written")


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_seam(config, mask, flags):
    import torch

    from crossbow_amd.seam import SmaPlan
    bmom, wd = CONFIGS[config]
    R, who = MASKS[mask]
    steps = [who is None or i in who for i in range(R)]
    rates = E.replica_rates(R)
    d, d0 = SsgdData(N, R, bmom, WPC, acc_seed=777), SsgdData(N, R, bmom, WPC, acc_seed=777)
    labels = write_catalogue(d, wd, rates, steps)
    write_catalogue(d0, wd, rates, steps)
    buf = SsgdBuffers(d)
    with SmaPlan([0], N) as plan:
        buf.call(plan, steps, rates, wd, flags)
        buf.stream.synchronize()
    with np.errstate(all="ignore"):
        d.step(steps, rates, wd, keep=True)  # the mirror steps in full; check() takes what is kept from d0
    torch.cuda.synchronize()
    table = {"z": [buf.z], "blast": [buf.blast], "acc": [buf.acc], "w": buf.w, "g": buf.g, "s": buf.s}
    check(lambda kind, i: table[kind][i].t.cpu().numpy()[:N], d, d0, labels, steps, wd, flags == 0)
    for kind, gds in table.items():
        for i, gd in enumerate(gds):
            if gd is not None:
                assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {kind}[{i}]")
    for i in range(R):
        assert_bitexact(buf.s[i].t.cpu().numpy()[:N], d0.st.s[i], f"s[{i}] is not touched")


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_context(config, mask, flags):
    # the context pads to whole kPadFloat4s: both copies of the catalogue run the float4 loop here
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    momentum, wd = CONFIGS[config]
    R, who = MASKS[mask]
    steps = [who is None or i in who for i in range(R)]
    tasks = [3 + 2 * i if steps[i] else -1 for i in range(R)]
    rates = _rates(_exp, R, tasks, momentum)
    assert all(r > 0 for r, s in zip(rates, steps) if s), rates
    d, d0 = SsgdCase(N, R, momentum, WPC), SsgdCase(N, R, momentum, WPC)
    for c in (d, d0):
        c.acc = O.fill_normal(N, 777, 0.01)  # what earlier task steps of the clock left
    labels = write_catalogue(d, wd, rates, steps)
    write_catalogue(d0, wd, rates, steps)
    gpu = _sgpu(N, R, momentum, wd, wpc=WPC)
    try:
        d.upload(gpu)
        gpu.base_write(0, BUF_GRADIENT, d.acc)
        assert gpu.lockAny() == R
        gpu.step_and_synchronise_ssgd(0, 1, 0, tasks, None, flags)
        gpu.unlockAny()
        gpu.wait()
        with np.errstate(all="ignore"):
            d.step(tasks, rates, wd, keep=True)  # the mirror steps in full; check() takes what is kept from d0
        kinds = {"w": BUF_DATA, "g": BUF_GRADIENT}

        def read(kind, i):
            if kind in ("z", "blast", "acc"):
                return gpu.base_read(0, {"z": BUF_DATA, "blast": BUF_LAST, "acc": BUF_GRADIENT}[kind])
            return gpu.replica_read(i, kinds[kind])
        check(read, d, d0, labels, steps, wd, flags == 0)
        for i in range(R):
            assert_bitexact(gpu.replica_read(i, BUF_DIFF), d0.st.s[i], f"s[{i}] is not touched")
            if d0.last[i] is not None:
                assert_bitexact(gpu.replica_read(i, BUF_LAST), d0.last[i], f"last[{i}] is not touched")
    finally:
        gpu.free()
