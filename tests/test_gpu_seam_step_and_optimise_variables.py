"""The sma.c seam for the fused task steps with a learning rate per variable:
cbx_sma_plan_step_and_optimise_variables over buffers the CALLER owns
(include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip, the TAIL
instantiations of task_barrier_variables_kernels.hip), on one GPU.

Expected values come from the oracle only:
``tests.test_optimise_plan.per_variable_step`` for every stepping replica in id
order, then ``O.sma_step``.  Every comparison is bit for bit over z, the base
``last``, and ``w``, ``last``, ``s`` and ``g`` of every replica.  Each device
buffer holds exactly n floats in front of 1,088 sentinel floats that must come
back untouched (tests/helpers.py, Guarded).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import GUARD
from tests.test_gpu_seam_step_and_optimise import ALPHA, CONFIGS, DISCARD, INVALID, Buffers, Data, _rates
from tests.test_optimise_plan import M, V, per_variable_step

pytestmark = pytest.mark.gpu

assert GUARD == 1088

# name: (variables, multipliers)
MODELS = {
    "tail-only-1": ((1,), (3.0,)),
    "empty-bulk-771": ((300, 0, 471), (2.0, 7.0, 0.5)),                  # three variables, one of them empty
    "V-21523": (V, M),                                                    # bulk 21,504, tail 19
    "boundary-in-tail-2051": ((1024, 1025, 2), (0.5, 2.0, 3.0)),          # bulk 2,048: 2,049 is inside the tail
    "boundary-at-bulk-end-1029": ((1024, 5), (2.0, 0.25)),                # bulk 1,024 = the boundary
}


class VarData(Data):
    def __init__(self, variables, mults, R, rmom, bmom):
        super().__init__(sum(variables), R, rmom, bmom)
        self.variables, self.mults = variables, mults

    def step(self, steps, rates, wd, keep=True):
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if steps[i] and not keep}
        for i in range(self.R):
            if steps[i]:
                per_variable_step(rates[i], self.mults, self.rmom, wd, st.w[i], self.g[i], self.last[i], st.s[i],
                                  variables=self.variables)
        copies = O.sma_step(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g
        return 1 if copies > 0 else 0


class VarBuffers(Buffers):
    def call(self, plan, steps, rates, wd, flags=0, **nulls):
        st = self.d.st
        return plan.step_and_optimise_variables([self.stream.cuda_stream], [self.z.ptr],
                                                [self.blast.ptr] if self.blast is not None else None,
                                                self.replicas(steps, rates, **nulls), ALPHA, st.momentum, self.d.rmom,
                                                wd, st.first, flags)


def _run(model, R, config, flags, steps=None, first=0, held=(), copies=()):
    from crossbow_amd.seam import SmaPlan
    variables, mults = MODELS[model]
    rmom, wd, bmom = CONFIGS[config]
    d = VarData(variables, mults, R, rmom, bmom)
    d.st.first = first
    for i in held:
        d.st.locked[i] = 0
    for i in copies:
        d.st.copy[i] = 1
    steps = [i >= first and i not in held for i in range(R)] if steps is None else steps
    rates = _rates(R)
    buf = VarBuffers(d)
    with SmaPlan([0], d.n) as plan:
        plan.set_variables(list(variables), list(mults))
        got = buf.call(plan, steps, rates, wd, flags)
        want = d.step(steps, rates, wd, keep=flags == 0)
        buf.check()
    assert got == want, (got, want)
    return buf, got


# replica momentum x weight decay in {0, 0.9} x {0, 5e-4}: CONFIGS' three plus momentum alone
CONFIGS = dict(CONFIGS, **{"mom-only": (0.9, 0.0, 0.9)})


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("R", [1, 3, 8, 9])
@pytest.mark.parametrize("model", list(MODELS))
def test_every_buffer_bitexact(model, R, config, flags):
    _run(model, R, config, flags)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("model", ["V-21523", "boundary-in-tail-2051", "empty-bulk-771"])
def test_mixed_steps(model, flags):
    _run(model, 9, "mom-wd", flags, steps=[i in (0, 3, 8) for i in range(9)])
    _run(model, 4, "base-mom-only", flags, first=1, held=(2,))


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("model", ["V-21523", "boundary-in-tail-2051", "tail-only-1"])
def test_phase_d(model, flags):
    from tests.helpers import assert_bitexact
    R, steps = 4, [True, True, False, True]
    buf, got = _run(model, R, "mom-wd", flags, steps=steps, copies=(1, 2))
    assert got == 1
    n = buf.d.n
    z = buf.z.t.cpu().numpy()[:n]
    for i in range(R):
        assert_bitexact(buf.w[i].t.cpu().numpy()[:n], z, f"w[{i}] == the new z, tail included")


def test_without_a_table_is_a_state_error_and_writes_nothing():
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    variables, mults = MODELS["boundary-in-tail-2051"]
    R, wd = 3, 5e-4
    d = VarData(variables, mults, R, 0.9, 0.9)
    buf = VarBuffers(d)
    rates = _rates(R)
    with SmaPlan([0], d.n) as plan:
        with pytest.raises(CbxError) as e:
            buf.call(plan, [True] * R, rates, wd)
        assert e.value.code == _lib.CBX_ERR_STATE, str(e.value)
        assert "cbx_sma_plan_step_and_optimise_variables" in _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")
        plan.set_variables(list(variables), list(mults))  # and the plan works once it has one
        buf.call(plan, [True] * R, rates, wd)
        d.step([True] * R, rates, wd)
        buf.check("after a good call:")


@pytest.mark.parametrize("name", list(INVALID))
def test_the_plain_calls_refusals_write_nothing(name):
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan, _ints, _ptrs
    kw = dict(INVALID[name])
    variables, mults = MODELS["boundary-in-tail-2051"]
    R, wd = 3, 5e-4
    d = VarData(variables, mults, R, 0.9, 0.9)
    d.st.first = kw.pop("first", 0)
    for i in kw.pop("held", ()):
        d.st.locked[i] = 0
    steps, flags, null_array = kw.pop("steps", [True] * R), kw.pop("flags", 0), kw.pop("null_array", None)
    buf = VarBuffers(d)
    rates = _rates(R)
    with SmaPlan([0], d.n) as plan:
        plan.set_variables(list(variables), list(mults))
        if null_array is None:
            with pytest.raises(CbxError) as e:
                buf.call(plan, steps, rates, wd, flags, **kw)
            assert e.value.code == _lib.CBX_ERR_INVALID, str(e.value)
        else:
            reps = buf.replicas(steps, rates)
            args = [plan._p, _ptrs([buf.stream.cuda_stream]), _ptrs([buf.z.ptr]), _ptrs([buf.blast.ptr]), R,
                    _ints([r[0] for r in reps]), _ptrs([r[1] for r in reps]), _ptrs([r[2] for r in reps]),
                    _ptrs([r[3] for r in reps]), _ptrs([r[4] for r in reps]), _ints([r[5] for r in reps]),
                    _ints([r[6] for r in reps]), _ints([r[7] for r in reps]), (ctypes.c_float * R)(*rates),
                    ALPHA, 0.9, 0.9, wd, 0, 0]
            args[null_array] = None
            assert plan.lib.cbx_sma_plan_step_and_optimise_variables(*args) == _lib.CBX_ERR_INVALID
        assert "cbx_sma_plan_step_and_optimise_variables" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")


def test_more_than_64_participating_replicas_is_unsupported():
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    variables, mults = MODELS["boundary-at-bulk-end-1029"]
    R, wd = 2, 0.0
    d = VarData(variables, mults, R, 0.0, 0.0)
    buf = VarBuffers(d)
    reps = buf.replicas([True] * R, _rates(R))
    with SmaPlan([0], d.n) as plan:
        plan.set_variables(list(variables), list(mults))
        with pytest.raises(CbxError) as e:
            plan.step_and_optimise_variables([buf.stream.cuda_stream], [buf.z.ptr], None,
                                             [reps[i % R] for i in range(65)], ALPHA, 0.0, 0.0, wd)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED, str(e.value)
        torch.cuda.synchronize()
        buf.check()
