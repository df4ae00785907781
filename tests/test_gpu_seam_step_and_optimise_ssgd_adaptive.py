"""``cbx_ssgd_plan_step_and_optimise_adaptive`` over buffers the caller owns (the TAIL instantiations of
task_ssgd_adaptive_kernels.hip), with the reference and the data of
tests/test_gpu_step_and_synchronise_ssgd_adaptive.py.  Every device buffer holds exactly n floats in front of
sentinel floats that must come back untouched."""
from __future__ import annotations

import numpy as np
import pytest

from tests.edge_values import assert_edge_equal
from tests.helpers import Guarded
from tests.test_gpu_adaptive_rate import EPS, RAGGED, SHAPES, _check_records, _mults
from tests.test_gpu_step_and_synchronise_adaptive import CASES, ETA
from tests.test_gpu_step_and_synchronise_ssgd_adaptive import PATHS, SETS, SsgdState, run_normal

pytestmark = pytest.mark.gpu

SLOT = 1


def _seam(state, tasks, rates, wd, mode, flags, eta=ETA, exact=True):
    """One call through the seam, checked against the host; returns the records' bytes."""
    import torch
    from crossbow_amd.seam import SmaPlan
    V, momentum = len(state.variables), state.st.momentum
    passed = {k: a for k, a in state.everything().items() if k[0] not in "sl"}  # z, base last and gradient, w and g
    dev = {name: Guarded(a, tag) for tag, (name, a) in enumerate(passed.items())}
    stream = torch.cuda.Stream().cuda_stream
    reps = [(0, dev[f"w[{i}]"].ptr, dev[f"g[{i}]"].ptr, 1, int(t >= 0), rates[i]) for i, t in enumerate(tasks)]
    with SmaPlan([0], sum(state.variables)) as plan:
        plan.set_variables(list(state.variables), _mults(state.variables, True))  # the multipliers play no part
        plan.set_adaptive(state.enable, slots=2)
        plan.ssgd_step_and_optimise_adaptive([stream], [dev["z"].ptr], [dev["base last"].ptr] if momentum > 0 else None,
                                             [dev["base gradient"].ptr], reps, momentum, wd, state.wpc, state.st.first,
                                             flags, slot=SLOT, trust=eta, epsilon=EPS, mode=mode)
        recs = plan.adaptive_stats(0, SLOT, stream, V)
        assert not plan.adaptive_stats(0, 1 - SLOT, stream, V).view(np.uint8).any()  # the other slot
    _check_records(recs, state.step(tasks, rates, wd, mode, flags == 0, device=None if exact else recs, eta=eta))
    for name in passed:
        a, host = state.everything()[name], dev[name].t.cpu().numpy()
        assert_edge_equal(host[:a.size], a, name)
        assert np.array_equal(host[a.size:].view(np.uint32), dev[name].sentinel.view(np.uint32)), f"behind {name}"
    return recs.tobytes()


@pytest.mark.parametrize("momentum, wd, mode, flags", [(c[0], c[1], c[2], c[4]) for c in CASES])
@pytest.mark.parametrize("variables, replicas", PATHS + [("small", "joiner")])
def test_every_buffer_and_record_through_the_seam(variables, replicas, momentum, wd, mode, flags):
    tasks, first, wpc = SETS[replicas]
    state = SsgdState(SHAPES[variables], len(tasks), momentum, wpc, first)
    _seam(state, tasks, [0.05 - 0.003 * i for i in range(len(tasks))], wd, mode, flags)


def test_normal_data_gives_the_same_records_through_both_doors():
    _, records, rates = run_normal()
    state = SsgdState(RAGGED, 3, 0.9, 3, exact=False)
    assert _seam(state, (3, 5, -1), rates, 1e-4, 1, 0, eta=0.002, exact=False) == records
