"""The sma.c seam for the fused task steps with layer-wise adaptive rates:
``cbx_sma_plan_step_and_optimise_adaptive`` over buffers the caller owns (the TAIL instantiations of
task_barrier_adaptive_kernels.hip).  The reference and the data are those of
tests/test_gpu_step_and_synchronise_adaptive.py; every device buffer holds exactly n floats in front of
sentinel floats that must come back untouched (tests/helpers.py, Guarded).  Three replicas, the middle one
only joins.  Lists: the ragged ones (a bulk and a tail), 771 (a 768-float bulk, 3 tail floats), 200 (tail only).
"""
from __future__ import annotations

import numpy as np
import pytest

from tests.edge_values import assert_edge_equal
from tests.helpers import Guarded
from tests.test_gpu_adaptive_rate import EPS, RAGGED, SHAPES, _check_records, _mults
from tests.test_gpu_step_and_synchronise_adaptive import ALPHA, CASES, ETA, State, _context, _fused

pytestmark = pytest.mark.gpu

STEPS, RATES, SLOTS = [1, 0, 1], [0.05, 0.0, 0.03], [2, 0, 1]
LISTS = dict(SHAPES, tail=(200,))


def _seam(variables, momentum, wd, mode, multipliers, flags):
    """One fused call through the seam, checked against the host; returns the stepping replicas' records."""
    import torch
    from crossbow_amd.seam import SmaPlan
    state, mults, V = State(variables, 3, momentum), _mults(variables, multipliers), len(variables)
    dev = {name: Guarded(a, tag) for tag, (name, a) in enumerate(state.want().items())}
    stream = torch.cuda.Stream().cuda_stream
    reps = [(0, dev[f"w[{i}]"].ptr, dev[f"s[{i}]"].ptr, dev[f"g[{i}]"].ptr,
             dev[f"last[{i}]"].ptr if momentum > 0 else None, 1, 0, STEPS[i], RATES[i]) for i in range(3)]
    with SmaPlan([0], sum(variables)) as plan:
        plan.set_variables(list(variables), mults)
        plan.set_adaptive(state.enable, slots=3)
        plan.step_and_optimise_adaptive([stream], [dev["z"].ptr], [dev["base last"].ptr] if momentum > 0 else None,
                                        reps, ALPHA, momentum, momentum, wd, 0, flags, slots=SLOTS, trust=ETA,
                                        epsilon=EPS, mode=mode)
        recs = [plan.adaptive_stats(0, SLOTS[i], stream, V) for i in range(3)]
    want = state.step([0 if s else -1 for s in STEPS], RATES, mults, wd, mode, keep=flags == 0)
    for name, a in state.want().items():
        host = dev[name].t.cpu().numpy()
        assert_edge_equal(host[:a.size], a, name)
        assert np.array_equal(host[a.size:].view(np.uint32), dev[name].sentinel.view(np.uint32)), f"behind {name}"
    for i in (0, 2):
        _check_records(recs[i], want[i])
    assert not recs[1].view(np.uint8).any()  # the joiner's slot
    return [recs[0].tobytes(), recs[2].tobytes()]


# the seam runs one launch shape, so the option cases without theirs
@pytest.mark.parametrize("momentum, wd, mode, multipliers, flags", [c[:5] for c in CASES])
@pytest.mark.parametrize("variables", ["ragged", "ragged0", "small", "tail"])
def test_every_buffer_and_record_through_the_seam(variables, momentum, wd, mode, multipliers, flags):
    _seam(LISTS[variables], momentum, wd, mode, multipliers, flags)


def test_the_records_are_the_same_bytes_through_both_doors():
    momentum, wd, mode = 0.9, 1e-4, 1
    state, mults = State(RAGGED, 3, momentum), _mults(RAGGED, True)
    gpu = _context(RAGGED, state.enable, 3, momentum, wd, mults)
    try:
        gpu.set_variable_learning_rates(True)
        gpu.set_adaptive_rate(ETA, EPS, mode)
        state.upload(gpu)
        _fused(gpu, [3, -1, 7])
        context = [gpu.replica_adaptive_stats(i, len(RAGGED)).tobytes() for i in (0, 2)]
    finally:
        gpu.free()
    assert context == _seam(RAGGED, momentum, wd, mode, True, 0)


@pytest.mark.parametrize("slots, code", [(None, "INVALID"), ([0, 0, 3], "INVALID"), ([0, 0, 0], "INVALID"),
                                         ([-1, 0, 1], "INVALID"), ("no tables", "STATE")])
def test_bad_slots_and_a_plan_without_tables(slots, code):
    import torch
    from crossbow_amd import _lib
    from crossbow_amd.seam import SmaPlan
    t = [torch.zeros(771, device="cuda:0") for _ in range(8)]
    reps = [(0, t[i].data_ptr(), t[3 + i].data_ptr() if i < 3 else 0, t[6].data_ptr(), None, 1, 0, STEPS[i], RATES[i])
            for i in range(3)]
    with SmaPlan([0], 771) as plan:
        plan.set_variables([771], [1.0])
        if slots == "no tables":
            slots = SLOTS
        else:
            plan.set_adaptive([True], slots=3)
        with pytest.raises(_lib.CbxError) as e:
            plan.step_and_optimise_adaptive([torch.cuda.current_stream().cuda_stream], [t[7].data_ptr()], None, reps,
                                            ALPHA, 0.0, 0.0, 0.0, 0, 0, slots=slots, trust=ETA, epsilon=EPS, mode=0)
        assert e.value.code == getattr(_lib, "CBX_ERR_" + code), str(e.value)
    assert not any(x.any() for x in t)
