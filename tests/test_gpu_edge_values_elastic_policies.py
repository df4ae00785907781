"""The clipped and per-variable task steps fused into the elastic-averaging
barrier on IEEE edge values (run with -m gpu): the fused catalogue of
tests/edge_values.py, in the bulk and in the last n mod 1,024 floats (the seam's
tail), through cbx_ea_plan_step_and_optimise_clipped_variables and
cbx_step_and_synchronise_elastic_clipped_variables, held to rules 1-3 of
DESIGN.md's edge-value contract (where the oracle has a NaN the device has a
NaN, everywhere else the 32 bits are equal, and a value that is only copied
keeps every bit) and, for the clipped step, to rule 5 of the reductions' clause:
the record is the host's S, K, scale and flags.

The scales are tests/test_gpu_edge_values_clipped.py's: S = k * FLT_MAX^2 is the
same bits in any order, so the expectation takes the host's; with the skip off
three values of max_norm give a normal scale, a subnormal scale and a scale that
rounds to zero, and with the skip on every stepping replica is skipped over
signalling NaNs with payloads.  The variables and multipliers (2^-126, 3, 2 and
0.5, none of them 1) are tests/test_gpu_edge_values_clipped_variables.py's.  The
comparisons are ``_check_fused`` of tests/test_gpu_edge_values.py (rates only)
and ``_check`` of tests/test_gpu_edge_values_clipped.py (clipping on).  The
oracle's output is asserted to hold NaNs in less than a quarter of every
compared array before the device is compared.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import averaging_common as AV
from tests import edge_values as E
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact, upload
from tests.test_gpu_edge_values import MASKS, _check_fused
from tests.test_gpu_edge_values_clipped import SCALES, _check, _steps
from tests.test_gpu_edge_values_clipped_variables import MULTS, VARS
from tests.test_gpu_seam_step_and_optimise import DISCARD, Data
from tests.test_gpu_seam_step_and_optimise_elastic import ElasticBuffers
from tests.test_optimise_plan import per_variable_step

pytestmark = pytest.mark.gpu

N, WD, ALPHA = E.N, E.WD, E.ALPHA
CONFIGS = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0), "wd-only": (0.0, WD), "mom-only": (0.9, 0.0)}
# (policy, scale): the per-variable policy has no scale; the clipped two take the three regimes and the skip
CELLS = [("variables", None)] + [(p, s) for p in ("clipped", "clipped_variables") for s in list(SCALES) + ["skipped"]]


def clips(policy):
    return policy in ("clipped", "clipped_variables")


def per_variable(policy):
    return policy in ("variables", "clipped_variables")


class EdgeData(Data):
    """Ordinary data with the catalogue written over it; the step is the policy's, the barrier the elastic one."""

    def __init__(self, policy, R, rmom, bmom):
        super().__init__(N, R, rmom, bmom)
        self.policy, self.decision = policy, {}

    def step(self, steps, rates, wd, keep=True, c=None, skip=True):
        st, pv = self.st, per_variable(self.policy)
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if steps[i] and not keep}
        self.decision = {}
        for i in range(self.R):
            if not steps[i]:
                continue
            bufs = [st.w[i], self.g[i], self.last[i], st.s[i]]
            if clips(self.policy):
                S, K = C.exact_sum_sq(self.g[i])
                scale, flags = C.decide(S, K, c, skip)
                self.decision[i] = {"sum_sq": S, "nonfinite": K, "scale": float(scale), "flags": flags}
                C.step(bufs, scale, flags, self.rmom, wd, lr=rates[i], variables=VARS if pv else None,
                       mults=MULTS if pv else None)
            else:
                per_variable_step(rates[i], MULTS, self.rmom, wd, *bufs, variables=VARS)
        AV.elastic_average(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g


def _data(policy, R, rmom, wd, bmom, rates, steps):
    d, d0 = EdgeData(policy, R, rmom, bmom), EdgeData(policy, R, rmom, bmom)
    labels = E.fused_case(d, rmom, wd, rates, steps)
    E.fused_case(d0, rmom, wd, rates, steps)
    return d, d0, labels


def _nans_within_a_quarter(d):
    st = d.st
    arrays = {"z": st.z[0]}
    for i in range(st.size):
        arrays.update({f"w[{i}]": st.w[i], f"s[{i}]": st.s[i], f"g[{i}]": d.g[i]})
        if d.last[i] is not None:
            arrays[f"last[{i}]"] = d.last[i]
    for name, a in arrays.items():
        assert E.nan_fraction(a) < 0.25, f"the oracle's {name} holds {E.nan_fraction(a):.2%} NaNs"


def _compare(policy, read, d, d0, labels, steps, rmom, wd, keep, skip, records):
    _nans_within_a_quarter(d)
    if clips(policy):
        _check(read, d, d0, labels, steps, keep, skip, records)
    else:
        _check_fused(read, d, d0, labels, steps, rmom, wd, keep, False)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("policy,scale", CELLS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_seam(config, policy, scale, mask, flags):
    import torch

    from crossbow_amd.seam import SmaPlan
    rmom, wd = CONFIGS[config]
    R, steps = _steps(mask)
    rates = E.replica_rates(R)
    skip = scale == "skipped"
    c = SCALES["normal" if skip or scale is None else scale]
    d, d0, labels = _data(policy, R, rmom, wd, 0.0, rates, steps)
    buf = ElasticBuffers(d)
    records = None
    with SmaPlan([0], N) as plan:
        if per_variable(policy):
            plan.set_variables(list(VARS), list(MULTS))
        plan.elastic_step_and_optimise_clipped_variables(
            [buf.stream.cuda_stream], [buf.z.ptr], buf.replicas(steps, rates), ALPHA, rmom, wd, 0, flags,
            slots=list(range(R)) if clips(policy) else None, max_norm=c, skip_nonfinite=skip,
            use_variables=per_variable(policy))
        buf.stream.synchronize()
        if clips(policy):
            records = [plan.clip_stats(0, i, buf.stream.cuda_stream) if steps[i] else None for i in range(R)]
    with np.errstate(all="ignore"):
        d.step(steps, rates, wd, keep=flags == 0, c=c, skip=skip)
    torch.cuda.synchronize()
    table = {"z": [buf.z], "w": buf.w, "s": buf.s, "g": buf.g, "r": buf.last}
    _compare(policy, lambda kind, i: table[kind][i].t.cpu().numpy()[:N], d, d0, labels, steps, rmom, wd, flags == 0, skip,
             records)
    for kind, gds in table.items():
        for i, gd in enumerate(gds):
            if gd is not None:
                assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {kind}[{i}]")


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("policy,scale", CELLS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_context(config, policy, scale, mask, flags):
    # the context pads to whole kPadFloat4s: both copies of the catalogue run the float4 loop here
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    from tests.test_gpu_step_and_synchronise import _exp, _rates
    from tests.test_gpu_step_and_synchronise_variables import _gpu
    momentum, wd = CONFIGS[config]
    R, steps = _steps(mask)
    tasks = [3 + 2 * i if steps[i] else -1 for i in range(R)]
    rates = _rates(_exp, R, tasks, momentum)
    assert all(r > 0 for r, s in zip(rates, steps) if s), rates
    skip = scale == "skipped"
    c = SCALES["normal" if skip or scale is None else scale]
    d, d0, labels = _data(policy, R, momentum, wd, momentum, rates, steps)
    gpu = _gpu(R, momentum, wd, _exp, variables=VARS, mults=MULTS, switch=per_variable(policy), update_type=3,
               elastic=True)
    try:
        if clips(policy):
            gpu.set_gradient_clip(c, skip)
        upload(gpu, d.st)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, d.g[i])
            if d.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, d.last[i])
        assert gpu.lockAny() == R
        gpu.step_and_synchronise_elastic_clipped_variables(0, 1, 0, tasks, None, flags)
        gpu.unlockAny()
        gpu.wait()
        with np.errstate(all="ignore"):
            d.step(steps, rates, wd, keep=flags == 0, c=c, skip=skip)
        kinds = {"w": BUF_DATA, "s": BUF_DIFF, "g": BUF_GRADIENT, "r": BUF_LAST}

        def read(kind, i):
            if kind in ("z", "blast"):
                return gpu.base_read(0, BUF_DATA if kind == "z" else BUF_LAST)
            return gpu.replica_read(i, kinds[kind])
        records = [gpu.replica_clip_stats(i) if steps[i] else None for i in range(R)] if clips(policy) else None
        _compare(policy, read, d, d0, labels, steps, momentum, wd, flags == 0, skip, records)
    finally:
        gpu.free()
