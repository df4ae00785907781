"""The task steps fused into the elastic-averaging barrier on IEEE edge values
(run with -m gpu): the inputs of tests/edge_values.py, as they are, through
cbx_ea_plan_step_and_optimise and cbx_step_and_synchronise_elastic, held to
rules 1-3 of DESIGN.md's edge-value contract by tests/test_gpu_edge_values.py's
own comparison (``_check_fused``): bits equal off NaN, NaN-ness equal, and a
kept ``s`` an exact copy of the old ``w``, signalling NaNs included.

The catalogue lies twice in every buffer: in the float4 bulk and in the last
n mod 1,024 floats, the seam's tail.  Alpha is 0.1, the rates are each
replica's own and non-zero, momentum and weight decay are either off (the
kernel then holds nothing of them) or 0.9 and 5e-4: none an exact 0 where it is
used.  The oracle's output is checked to hold NaNs in less than a quarter of
every compared array before the device is compared.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import edge_values as E
from tests.helpers import assert_bitexact
from tests.test_gpu_edge_values import MASKS, _check_fused
from tests.test_gpu_seam_step_and_optimise import DISCARD
from tests.test_gpu_seam_step_and_optimise_elastic import ElasticBuffers, ElasticData
from tests.test_gpu_step_and_synchronise import _exp, _rates
from tests.test_gpu_step_and_synchronise_elastic import ElasticCase, _egpu

pytestmark = pytest.mark.gpu

N, WD = E.N, E.WD
CONFIGS = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0), "wd-only": (0.0, WD), "mom-only": (0.9, 0.0)}


def _nans_within_a_quarter(d):
    st = d.st
    arrays = {"z": st.z[0]}
    for i in range(st.size):
        arrays.update({f"w[{i}]": st.w[i], f"s[{i}]": st.s[i], f"g[{i}]": d.g[i]})
        if d.last[i] is not None:
            arrays[f"last[{i}]"] = d.last[i]
    for name, a in arrays.items():
        assert E.nan_fraction(a) < 0.25, f"the oracle's {name} holds {E.nan_fraction(a):.2%} NaNs"


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_seam(config, mask, flags):
    import torch

    from crossbow_amd.seam import SmaPlan
    rmom, wd = CONFIGS[config]
    R, who = MASKS[mask]
    steps = [who is None or i in who for i in range(R)]
    rates = E.replica_rates(R)
    d, d0 = ElasticData(N, R, rmom), ElasticData(N, R, rmom)
    labels = E.fused_case(d, rmom, wd, rates, steps)
    E.fused_case(d0, rmom, wd, rates, steps)
    buf = ElasticBuffers(d)
    with SmaPlan([0], N) as plan:
        buf.call(plan, steps, rates, wd, flags)
        buf.stream.synchronize()
    with np.errstate(all="ignore"):
        d.step(steps, rates, wd, keep=flags == 0)
    _nans_within_a_quarter(d)
    torch.cuda.synchronize()
    table = {"z": [buf.z], "w": buf.w, "s": buf.s, "g": buf.g, "r": buf.last}
    _check_fused(lambda kind, i: table[kind][i].t.cpu().numpy()[:N], d, d0, labels, steps, rmom, wd, flags == 0, False)
    for kind, gds in table.items():
        for i, gd in enumerate(gds):
            if gd is not None:
                assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {kind}[{i}]")


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
    d, d0 = ElasticCase(N, R, momentum), ElasticCase(N, R, momentum)
    labels = E.fused_case(d, momentum, wd, rates, steps)
    E.fused_case(d0, momentum, wd, rates, steps)
    gpu = _egpu(N, R, momentum, wd)
    try:
        d.upload(gpu)
        assert gpu.lockAny() == R
        gpu.step_and_synchronise_elastic(0, 1, 0, tasks, None, flags)
        gpu.unlockAny()
        gpu.wait()
        with np.errstate(all="ignore"):
            d.step(tasks, rates, wd, keep=True)  # the mirror steps in full; _check_fused takes what is kept from d0
        _nans_within_a_quarter(d)
        kinds = {"w": BUF_DATA, "s": BUF_DIFF, "g": BUF_GRADIENT, "r": BUF_LAST}

        def read(kind, i):
            if kind in ("z", "blast"):
                return gpu.base_read(0, BUF_DATA if kind == "z" else BUF_LAST)
            return gpu.replica_read(i, kinds[kind])
        _check_fused(read, d, d0, labels, steps, momentum, wd, flags == 0, False)
    finally:
        gpu.free()
