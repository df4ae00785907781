"""``cbx_ea_plan_step_and_optimise_adaptive`` over buffers the caller owns (the TAIL instantiations of
task_elastic_adaptive_kernels.hip), with the reference and the data of
tests/test_gpu_step_and_synchronise_elastic_adaptive.py.  Every device buffer holds exactly n floats in front
of sentinel floats that must come back untouched.  Three replicas, the middle one only joins."""
from __future__ import annotations

import numpy as np
import pytest

from tests.edge_values import assert_edge_equal
from tests.helpers import Guarded
from tests.test_gpu_adaptive_rate import EPS, RAGGED, SHAPES, _check_records, _mults
from tests.test_gpu_step_and_synchronise_adaptive import ALPHA, CASES, ETA
from tests.test_gpu_step_and_synchronise_elastic_adaptive import ElasticState, _fused, context

pytestmark = pytest.mark.gpu

STEPS, RATES, SLOTS = [1, 0, 1], [0.05, 0.0, 0.03], [2, 0, 1]


def _seam(variables, momentum, wd, mode, multipliers, flags):
    """One fused call through the seam, checked against the host; returns the stepping replicas' records."""
    import torch
    from crossbow_amd.seam import SmaPlan
    state, mults, V = ElasticState(variables, 3, momentum), _mults(variables, multipliers), len(variables)
    dev = {name: Guarded(a, tag) for tag, (name, a) in enumerate(state.want().items())}
    stream = torch.cuda.Stream().cuda_stream
    reps = [(0, dev[f"w[{i}]"].ptr, dev[f"s[{i}]"].ptr, dev[f"g[{i}]"].ptr,
             dev[f"last[{i}]"].ptr if momentum > 0 else None, 1, STEPS[i], RATES[i]) for i in range(3)]
    with SmaPlan([0], sum(variables)) as plan:
        plan.set_variables(list(variables), mults)
        plan.set_adaptive(state.enable, slots=3)
        plan.elastic_step_and_optimise_adaptive([stream], [dev["z"].ptr], reps, ALPHA, momentum, wd, 0, flags,
                                                slots=SLOTS, trust=ETA, epsilon=EPS, mode=mode)
        recs = [plan.adaptive_stats(0, SLOTS[i], stream, V) for i in range(3)]
    want = state.step([0 if s else -1 for s in STEPS], RATES, mults, wd, mode, keep=flags == 0)
    for name, a in state.want().items():  # the base model's last is not passed: it comes back as it went
        host = dev[name].t.cpu().numpy()
        assert_edge_equal(host[:a.size], a, name)
        assert np.array_equal(host[a.size:].view(np.uint32), dev[name].sentinel.view(np.uint32)), f"behind {name}"
    for i in (0, 2):
        _check_records(recs[i], want[i])
    assert not recs[1].view(np.uint8).any()  # the joiner's slot
    return [recs[0].tobytes(), recs[2].tobytes()]


@pytest.mark.parametrize("momentum, wd, mode, multipliers, flags", [c[:5] for c in CASES])
@pytest.mark.parametrize("variables", ["ragged", "small"])
def test_every_buffer_and_record_through_the_seam(variables, momentum, wd, mode, multipliers, flags):
    _seam(SHAPES[variables], momentum, wd, mode, multipliers, flags)


def test_the_records_are_the_same_bytes_through_both_doors():
    momentum, wd, mode = 0.9, 1e-4, 1
    state, mults = ElasticState(RAGGED, 3, momentum), _mults(RAGGED, True)
    gpu = context(RAGGED, state.enable, 3, momentum, wd, mults)
    try:
        gpu.set_variable_learning_rates(True)
        gpu.set_adaptive_rate(ETA, EPS, mode)
        state.upload(gpu)
        _fused(gpu, [3, -1, 7])
        records = [gpu.replica_adaptive_stats(i, len(RAGGED)).tobytes() for i in (0, 2)]
    finally:
        gpu.free()
    assert records == _seam(RAGGED, momentum, wd, mode, True, 0)
