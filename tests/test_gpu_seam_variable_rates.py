"""The sma.c seam of the per-variable replica step: cbx_sma_plan_set_variables
and cbx_sma_plan_optimise_variables over buffers the CALLER owns, of exactly
`elements` floats (include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip).
Each buffer here is followed by a guard of sentinel floats that no step may
touch.  Bit for bit against the oracle's replica step called once per variable
on slices (tests/test_optimise_plan.py)."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_bitexact
from tests.test_optimise_plan import LR, M, V, per_variable_step

pytestmark = pytest.mark.gpu

N = sum(V)
GUARD = 1024


class _Buffers:
    """w, g, last, s on the host and on the device; the device copies carry
    GUARD sentinel floats past the n the plan knows of."""

    def __init__(self, seed, momentum):
        import torch
        self.host = [O.fill_normal(N, seed, 0.05), O.fill_normal(N, seed + 1, 0.01),
                     O.fill_normal(N, seed + 2, 0.001) if momentum > 0 else None, O.fill_normal(N, seed + 3, 7.0)]
        self.guard = O.fill_normal(GUARD, seed + 4, 3.0)
        self.dev = [torch.from_numpy(np.concatenate([a, self.guard])).to("cuda:0") if a is not None else None
                    for a in self.host]
        for t in self.dev:
            assert t is None or t.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def ptrs(self):
        return [t.data_ptr() if t is not None else None for t in self.dev]

    def check(self, what=""):
        for name, t, a in zip(("w", "g", "last", "s"), self.dev, self.host):
            if a is None:
                continue
            got = t.cpu().numpy()
            assert_bitexact(got[:N], a, what + name)
            assert_bitexact(got[N:], self.guard, what + name + " guard")


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_whole_range_middle_range_and_no_variables(momentum, wd):
    import torch

    from crossbow_amd.seam import SmaPlan
    b = _Buffers(600, momentum)
    stream = torch.cuda.Stream()
    with SmaPlan([0], N) as plan:
        plan.set_variables(V, M)
        w, g, last, s = b.ptrs()
        plan.optimise_variables(0, stream.cuda_stream, w, g, last, s, LR, momentum, wd, 0, len(V))
        stream.synchronize()
        per_variable_step(LR, M, momentum, wd, *b.host)
        b.check("whole range: ")
        plan.optimise_variables(0, stream.cuda_stream, w, g, last, s, LR, momentum, wd, 2, 3)
        stream.synchronize()
        per_variable_step(LR, M, momentum, wd, *b.host, only={2, 3, 4})
        b.check("variables 2..4: ")
        plan.optimise_variables(0, stream.cuda_stream, w, g, last, s, LR, momentum, wd, 5, 0)
        plan.optimise_variables(0, stream.cuda_stream, w, g, last, s, LR, momentum, wd, len(V), 0)
        stream.synchronize()
        b.check("no variables: ")
        plan.optimise_variables(0, stream.cuda_stream, w, g, last, s, LR, momentum, wd, len(V) - 1, 1)
        stream.synchronize()
        per_variable_step(LR, M, momentum, wd, *b.host, only={len(V) - 1})
        b.check("the last variable, with the odd tail: ")


def test_refusals():
    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    b = _Buffers(620, 0.9)
    w, g, last, s = b.ptrs()
    with SmaPlan([0], N) as plan:
        with pytest.raises(CbxError) as e:  # no tables yet
            plan.optimise_variables(0, None, w, g, last, s, LR, 0.9, 0.0, 0, 1)
        assert e.value.code == _lib.CBX_ERR_STATE
        for bad in (V[:-1], V + (1,), (N + 1, -1), ()):
            with pytest.raises(CbxError) as e:
                plan.set_variables(bad)
            assert e.value.code == _lib.CBX_ERR_INVALID, bad
        plan.set_variables(V, M)
        for first, count in ((-1, 1), (0, len(V) + 1), (len(V), 1), (3, -1)):
            with pytest.raises(CbxError) as e:
                plan.optimise_variables(0, None, w, g, last, s, LR, 0.9, 0.0, first, count)
            assert e.value.code == _lib.CBX_ERR_INVALID, (first, count)
        with pytest.raises(CbxError) as e:  # momentum without `last`
            plan.optimise_variables(0, None, w, g, None, s, LR, 0.9, 0.0, 0, 1)
        assert e.value.code == _lib.CBX_ERR_INVALID
        with pytest.raises(CbxError) as e:
            plan.optimise_variables(0, None, w + 4, g, last, s, LR, 0.9, 0.0, 0, 1)
        assert e.value.code == _lib.CBX_ERR_INVALID
        with pytest.raises(CbxError) as e:
            plan.optimise_variables(1, None, w, g, last, s, LR, 0.9, 0.0, 0, 1)
        assert e.value.code == _lib.CBX_ERR_INVALID
    b.check("after the refusals: ")


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_no_multipliers_equals_optimise_buffers(momentum):
    import torch

    from crossbow_amd.seam import SmaPlan, optimise_buffers
    a, b = _Buffers(640, momentum), _Buffers(640, momentum)
    stream = torch.cuda.Stream()
    with SmaPlan([0], N) as plan:
        plan.set_variables(V)
        plan.optimise_variables(0, stream.cuda_stream, *a.ptrs(), LR, momentum, 5e-4, 0, len(V))
        w, g, last, s = b.ptrs()
        optimise_buffers(stream.cuda_stream, w, g, last, s, N, LR, momentum, 5e-4)
        stream.synchronize()
    O.sma_optimise(np.float32(-LR), momentum, 5e-4, *a.host)
    a.check("all multipliers 1: ")
    for x, y, name in zip(a.dev, b.dev, ("w", "g", "last", "s")):
        if x is not None:
            assert_bitexact(x.cpu().numpy()[:N], y.cpu().numpy()[:N], name + " against cbx_sma_optimise_buffers")


def test_replacing_the_tables_between_two_steps():
    import torch

    from crossbow_amd.seam import SmaPlan
    b = _Buffers(660, 0.9)
    stream = torch.cuda.Stream()
    # the same floats cut differently, with other multipliers
    V2 = (4, 35, 8189, 13295)
    M2 = (0.5, 3.0, 1.0, 0.0)
    assert sum(V2) == N
    with SmaPlan([0], N) as plan:
        w, g, last, s = b.ptrs()
        plan.set_variables(V, M)
        plan.optimise_variables(0, stream.cuda_stream, w, g, last, s, LR, 0.9, 5e-4, 0, len(V))
        plan.set_variables(V2, M2)  # blocks: the first step is done
        plan.optimise_variables(0, stream.cuda_stream, w, g, last, s, LR, 0.9, 5e-4, 1, 3)
        stream.synchronize()
    per_variable_step(LR, M, 0.9, 5e-4, *b.host)
    per_variable_step(LR, M2, 0.9, 5e-4, *b.host, variables=V2, only={1, 2, 3})
    b.check()
