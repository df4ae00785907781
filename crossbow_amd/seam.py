"""Python view of the sma.c seam (include/crossbow_sma.h, ``cbx_sma_plan_*``):
the SMA step and the replica optimiser step over device buffers the caller
owns, for a Crossbow build that keeps its own model manager and replaces only
``crossbowSynchronisationSMA`` (clib-multigpu/synch/sma.c:233-248) and
``crossbowKernelOptimiserSMA`` (kernels/optimisers/sma.cu:3-100), or with
tau = 1 both in one launch (``SmaPlan.step_and_optimise``), and in the
same way the synchronous-SGD, elastic-averaging (synch/synchronouseamsgd.c)
and Polyak-Ruppert (synch/polyakruppert.c) barriers.

Pointers and streams are plain integers (``tensor.data_ptr()``,
``torch.cuda.Stream().cuda_stream``, or raw ``hipMalloc`` results).  Torch-free:
``lib`` is a bound library (``crossbow_amd._lib.load()`` by default, or a
build bound through ``crossbow_amd._abi.bind``).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple


def _default_lib():
    from . import _lib
    return _lib.load()


def _raise(lib, rc: int, what: str) -> int:
    if rc < 0:
        msg = f"{what}: {lib.cbx_last_error().decode(errors='replace')}"
        try:
            from ._abi import CbxError
        except ImportError:  # loaded as a standalone file (the torch-free test workers)
            raise RuntimeError(f"{rc} {msg}") from None
        raise CbxError(rc, msg)
    return rc


def _ptrs(values: Sequence[Optional[int]]):
    arr = (ctypes.c_void_p * max(1, len(values)))()
    for k, v in enumerate(values):
        arr[k] = v or None
    return arr


def _ints(values: Sequence[int]):
    arr = (ctypes.c_int * max(1, len(values)))()
    for k, v in enumerate(values):
        arr[k] = int(v)
    return arr


class SmaPlan:
    """``cbx_sma_plan_create`` over HIP devices ``devices`` for buffers of
    ``elements`` floats; ``comms`` = the caller's ncclComm_t handles (ints), or
    None to let the plan create them (ncclCommInitAll, more than one device)."""

    def __init__(self, devices: Sequence[int], elements: int, comms: Optional[Sequence[int]] = None, lib=None,
                 buckets: int = 0):
        self.lib = lib if lib is not None else _default_lib()
        self.G = len(devices)
        p = ctypes.c_void_p()
        _raise(self.lib, self.lib.cbx_sma_plan_create(ctypes.byref(p), _ints(devices), self.G, elements,
                                                      _ptrs(comms) if comms is not None else None),
               "cbx_sma_plan_create")
        self._p = p
        if buckets:
            self.set_buckets(buckets)

    def step(self, streams: Sequence[int], z: Sequence[int], last: Optional[Sequence[Optional[int]]],
             replicas: Sequence[Tuple[int, int, int, int, int]], alpha: float, momentum: float,
             first: int = 0) -> int:
        """One SMA step.  ``replicas[id]`` = (device index, w, s, locked, copy).
        Returns 1 when Phase D ran."""
        dev = [r[0] for r in replicas]
        return _raise(self.lib, self.lib.cbx_sma_plan_step(
            self._p, _ptrs(streams), _ptrs(z), _ptrs(last) if last is not None else None, len(replicas),
            _ints(dev), _ptrs([r[1] for r in replicas]), _ptrs([r[2] for r in replicas]),
            _ints([r[3] for r in replicas]), _ints([r[4] for r in replicas]), ctypes.c_float(alpha),
            ctypes.c_float(momentum), first), "cbx_sma_plan_step")

    def step_and_optimise(self, streams: Sequence[int], z: Sequence[int], last: Optional[Sequence[Optional[int]]],
                          replicas: Sequence[Tuple[int, int, Optional[int], Optional[int], Optional[int], int, int, int,
                                                   float]],
                          alpha: float, momentum: float, replica_momentum: float, weight_decay: float,
                          first: int = 0, flags: int = 0) -> int:
        """The stepping replicas' task steps and the SMA step in one launch
        (``cbx_sma_plan_step_and_optimise``; one device, one rank).
        ``replicas[id]`` = (device index, w, s, g, rlast, locked, copy, step,
        learning_rate): ``step`` != 0 means the replica's gradient ``g`` is
        applied first, at ``learning_rate`` (positive), with ``rlast`` its
        momentum buffer (None without replica momentum).  ``flags`` is 0 or
        ``STEP_DISCARD_TASK_OUTPUTS``, under which a stepping replica's ``s``
        may be None.  The caller orders ``streams[0]`` behind the gradients.
        Returns 1 when Phase D ran."""
        return self._step_and_optimise("cbx_sma_plan_step_and_optimise", streams, z, last, replicas, alpha, momentum,
                                       replica_momentum, weight_decay, first, flags)

    def step_and_optimise_variables(self, streams, z, last, replicas, alpha: float, momentum: float,
                                    replica_momentum: float, weight_decay: float, first: int = 0,
                                    flags: int = 0) -> int:
        """``step_and_optimise`` with a learning rate per variable
        (``cbx_sma_plan_step_and_optimise_variables``): variable v of a
        stepping replica steps at ``learning_rate * multipliers[v]`` of the
        table ``set_variables`` installed.  Same arguments."""
        return self._step_and_optimise("cbx_sma_plan_step_and_optimise_variables", streams, z, last, replicas, alpha,
                                       momentum, replica_momentum, weight_decay, first, flags)

    def step_and_optimise_clipped(self, streams, z, last, replicas, alpha: float, momentum: float,
                                  replica_momentum: float, weight_decay: float, first: int = 0, flags: int = 0,
                                  slots: Optional[Sequence[int]] = None, max_norm: float = 0.0,
                                  skip_nonfinite: bool = False) -> int:
        """``step_and_optimise`` with the clipped step of ``optimise_clipped``
        (``cbx_sma_plan_step_and_optimise_clipped``): stepping replica id is
        clipped to ``max_norm`` (0: none) through the record of ``slots[id]``,
        whose norm pass the call runs on ``streams[0]`` first, and skipped when
        ``skip_nonfinite`` and its gradient holds a NaN or an infinity.  Two
        stepping replicas take two slots.  Otherwise the same arguments."""
        return self._step_and_optimise("cbx_sma_plan_step_and_optimise_clipped", streams, z, last, replicas, alpha,
                                       momentum, replica_momentum, weight_decay, first, flags,
                                       (_ints(slots) if slots is not None else None, ctypes.c_float(max_norm),
                                        1 if skip_nonfinite else 0))

    def step_and_optimise_clipped_variables(self, streams, z, last, replicas, alpha: float, momentum: float,
                                            replica_momentum: float, weight_decay: float, first: int = 0,
                                            flags: int = 0, slots: Optional[Sequence[int]] = None,
                                            max_norm: float = 0.0, skip_nonfinite: bool = False) -> int:
        """``step_and_optimise_clipped`` with a learning rate per variable
        (``cbx_sma_plan_step_and_optimise_clipped_variables``): the clipped
        step at ``learning_rate * multipliers[v]`` of the table
        ``set_variables`` installed.  Same arguments."""
        return self._step_and_optimise("cbx_sma_plan_step_and_optimise_clipped_variables", streams, z, last, replicas,
                                       alpha, momentum, replica_momentum, weight_decay, first, flags,
                                       (_ints(slots) if slots is not None else None, ctypes.c_float(max_norm),
                                        1 if skip_nonfinite else 0))

    def _step_and_optimise(self, name, streams, z, last, replicas, alpha, momentum, replica_momentum, weight_decay,
                           first, flags, clip=()) -> int:
        rate = (ctypes.c_float * max(1, len(replicas)))(*[float(r[8]) for r in replicas])
        return _raise(self.lib, getattr(self.lib, name)(
            self._p, _ptrs(streams), _ptrs(z), _ptrs(last) if last is not None else None, len(replicas),
            _ints([r[0] for r in replicas]), _ptrs([r[1] for r in replicas]), _ptrs([r[2] for r in replicas]),
            _ptrs([r[3] for r in replicas]), _ptrs([r[4] for r in replicas]), _ints([r[5] for r in replicas]),
            _ints([r[6] for r in replicas]), _ints([r[7] for r in replicas]), rate, *clip, ctypes.c_float(alpha),
            ctypes.c_float(momentum), ctypes.c_float(replica_momentum), ctypes.c_float(weight_decay), first,
            ctypes.c_uint(flags)), name)

    def ssgd_step(self, streams: Sequence[int], z: Sequence[int], last: Optional[Sequence[Optional[int]]],
                  acc: Sequence[int], replicas: Sequence[Tuple[int, int, int]], momentum: float, wpc: int,
                  first: int = 0) -> None:
        """One synchronous-SGD barrier (update model WORKER).  ``replicas[id]`` =
        (device index, w, locked)."""
        _raise(self.lib, self.lib.cbx_ssgd_plan_step(
            self._p, _ptrs(streams), _ptrs(z), _ptrs(last) if last is not None else None, _ptrs(acc),
            len(replicas), _ints([r[0] for r in replicas]), _ptrs([r[1] for r in replicas]),
            _ints([r[2] for r in replicas]), ctypes.c_float(momentum), wpc, first), "cbx_ssgd_plan_step")

    def ssgd_step_and_optimise(self, streams: Sequence[int], z: Sequence[int], last: Optional[Sequence[Optional[int]]],
                               acc: Sequence[int], replicas: Sequence[Tuple[int, int, Optional[int], int, int, float]],
                               momentum: float, weight_decay: float, wpc: int, first: int = 0,
                               flags: int = 0) -> None:
        """The stepping replicas' task steps and the synchronous-SGD barrier in
        one launch (``cbx_ssgd_plan_step_and_optimise``; one device, one rank).
        ``replicas[id]`` = (device index, w, g, locked, step, learning_rate);
        ``g`` may be None for a replica that only joins.  ``last`` may be None
        when ``momentum`` is 0.  The caller orders ``streams[0]`` behind the
        gradients."""
        rate = (ctypes.c_float * max(1, len(replicas)))(*[float(r[5]) for r in replicas])
        _raise(self.lib, self.lib.cbx_ssgd_plan_step_and_optimise(
            self._p, _ptrs(streams), _ptrs(z), _ptrs(last) if last is not None else None, _ptrs(acc),
            len(replicas), _ints([r[0] for r in replicas]), _ptrs([r[1] for r in replicas]),
            _ptrs([r[2] for r in replicas]), _ints([r[3] for r in replicas]), _ints([r[4] for r in replicas]), rate,
            ctypes.c_float(momentum), ctypes.c_float(weight_decay), wpc, first, ctypes.c_uint(flags)),
            "cbx_ssgd_plan_step_and_optimise")

    def elastic_step(self, streams: Sequence[int], z: Sequence[int],
                     replicas: Sequence[Tuple[int, int, Optional[int], int]], alpha: float, first: int = 0) -> None:
        """One elastic-averaging barrier (``cbx_ea_plan_step``).  ``replicas[id]``
        = (device index, w, s, locked); ``s`` may be None (0) with one rank,
        where the difference is taken from ``w``."""
        s = [r[2] for r in replicas]
        _raise(self.lib, self.lib.cbx_ea_plan_step(
            self._p, _ptrs(streams), _ptrs(z), len(replicas), _ints([r[0] for r in replicas]),
            _ptrs([r[1] for r in replicas]), _ptrs(s) if any(s) else None, _ints([r[3] for r in replicas]),
            ctypes.c_float(alpha), first), "cbx_ea_plan_step")

    def elastic_step_and_optimise(self, streams: Sequence[int], z: Sequence[int],
                                  replicas: Sequence[Tuple[int, int, Optional[int], Optional[int], Optional[int], int,
                                                           int, float]],
                                  alpha: float, replica_momentum: float, weight_decay: float, first: int = 0,
                                  flags: int = 0) -> None:
        """The stepping replicas' task steps and the elastic-averaging barrier
        in one launch (``cbx_ea_plan_step_and_optimise``; one device, one
        rank).  ``replicas[id]`` = (device index, w, s, g, rlast, locked, step,
        learning_rate), as for ``step_and_optimise`` without ``copy``; ``s``
        may be None for a replica that only joins, or that steps under
        ``STEP_DISCARD_TASK_OUTPUTS``.  The caller orders ``streams[0]`` behind
        the gradients."""
        rate = (ctypes.c_float * max(1, len(replicas)))(*[float(r[7]) for r in replicas])
        _raise(self.lib, self.lib.cbx_ea_plan_step_and_optimise(
            self._p, _ptrs(streams), _ptrs(z), len(replicas), _ints([r[0] for r in replicas]),
            _ptrs([r[1] for r in replicas]), _ptrs([r[2] for r in replicas]), _ptrs([r[3] for r in replicas]),
            _ptrs([r[4] for r in replicas]), _ints([r[5] for r in replicas]), _ints([r[6] for r in replicas]), rate,
            ctypes.c_float(alpha), ctypes.c_float(replica_momentum), ctypes.c_float(weight_decay), first,
            ctypes.c_uint(flags)), "cbx_ea_plan_step_and_optimise")

    def elastic_step_and_optimise_clipped_variables(self, streams: Sequence[int], z: Sequence[int], replicas,
                                                    alpha: float, replica_momentum: float, weight_decay: float,
                                                    first: int = 0, flags: int = 0,
                                                    slots: Optional[Sequence[int]] = None, max_norm: float = 0.0,
                                                    skip_nonfinite: bool = False,
                                                    use_variables: bool = False) -> None:
        """``elastic_step_and_optimise`` with the clipped step of
        ``optimise_clipped``, a learning rate per variable, or both
        (``cbx_ea_plan_step_and_optimise_clipped_variables``).  Clipping is on
        iff ``slots`` is given: stepping replica id is clipped to ``max_norm``
        (0: none) through the record of ``slots[id]``, whose norm pass the call
        runs on ``streams[0]`` first, and skipped when ``skip_nonfinite`` and
        its gradient holds a NaN or an infinity.  ``use_variables``: variable v
        steps at ``learning_rate * multipliers[v]`` of the table
        ``set_variables`` installed.  Otherwise the same arguments; with
        neither it is ``elastic_step_and_optimise``."""
        rate = (ctypes.c_float * max(1, len(replicas)))(*[float(r[7]) for r in replicas])
        _raise(self.lib, self.lib.cbx_ea_plan_step_and_optimise_clipped_variables(
            self._p, _ptrs(streams), _ptrs(z), len(replicas), _ints([r[0] for r in replicas]),
            _ptrs([r[1] for r in replicas]), _ptrs([r[2] for r in replicas]), _ptrs([r[3] for r in replicas]),
            _ptrs([r[4] for r in replicas]), _ints([r[5] for r in replicas]), _ints([r[6] for r in replicas]), rate,
            _ints(slots) if slots is not None else None, ctypes.c_float(max_norm), 1 if skip_nonfinite else 0,
            1 if use_variables else 0, ctypes.c_float(alpha), ctypes.c_float(replica_momentum),
            ctypes.c_float(weight_decay), first, ctypes.c_uint(flags)),
            "cbx_ea_plan_step_and_optimise_clipped_variables")

    def polyak_step(self, streams: Sequence[int], z: Sequence[int], last: Optional[Sequence[Optional[int]]],
                    replicas: Sequence[Tuple[int, int, int, int]], alpha: float, clock: int, first: int = 0) -> int:
        """One Polyak-Ruppert barrier (``cbx_pr_plan_step``).  ``replicas[id]`` =
        (device index, w, locked, copy).  Returns how many locked replicas from
        ``first`` on had ``copy`` raised and now equal their device's z."""
        return _raise(self.lib, self.lib.cbx_pr_plan_step(
            self._p, _ptrs(streams), _ptrs(z), _ptrs(last) if last is not None else None, len(replicas),
            _ints([r[0] for r in replicas]), _ptrs([r[1] for r in replicas]), _ints([r[2] for r in replicas]),
            _ints([r[3] for r in replicas]), ctypes.c_float(alpha), clock, first), "cbx_pr_plan_step")

    def average_batchnorm(self, elements: Sequence[int], mean: Sequence[int], variance: Sequence[int],
                          updated: Sequence[int]) -> None:
        """BN running-statistics averaging; ``mean``/``variance``/``updated`` are
        indexed [k * layers + l] (k: position in the plan's devices)."""
        _raise(self.lib, self.lib.cbx_sma_plan_average_batchnorm(
            self._p, len(elements), _ints(elements), _ptrs(mean), _ptrs(variance), _ints(updated)),
            "cbx_sma_plan_average_batchnorm")

    def buffer_stats(self, k: int, stream: int, ref: int, bufs: Sequence[int],
                     var_elements: Optional[Sequence[int]] = None, per_variable: bool = False):
        """``cbx_sma_plan_buffer_stats`` on the plan's device ``k``: the
        statistics of ``ref`` and of each of ``bufs`` against it (device
        pointers of ``elements`` floats).  Returns ``(ref, bufs)`` as numpy
        structured arrays of shapes () and (len(bufs),); with ``per_variable``
        also ``(ref_vars, buf_vars)`` of shapes (V,) and (len(bufs), V)."""
        import numpy as np
        fields = [("sum", "<f8"), ("sum_sq", "<f8"), ("dist_sq", "<f8"), ("nonfinite", "<u8"),
                  ("max_abs", "<f4"), ("reserved", "<u4")]
        dt = np.dtype(fields)
        nv = len(var_elements) if var_elements else 0
        V = max(1, nv)
        ve = (ctypes.c_longlong * V)(*(var_elements or [0]))
        r, o = np.zeros(1, dtype=dt), np.zeros(max(1, len(bufs)), dtype=dt)
        rv, ov = np.zeros(V, dtype=dt), np.zeros((max(1, len(bufs)), V), dtype=dt)
        bs = self.lib.cbx_sma_plan_buffer_stats.argtypes[8]

        def p(a):
            return ctypes.cast(a.ctypes.data, bs)
        _raise(self.lib, self.lib.cbx_sma_plan_buffer_stats(
            self._p, k, stream or None, ref, _ptrs(bufs), len(bufs), ve if nv else None, nv, p(r), p(o),
            p(rv) if per_variable else None, p(ov) if per_variable else None), "cbx_sma_plan_buffer_stats")
        o, ov = o[:len(bufs)], ov[:len(bufs)]
        return (r[0], o, rv, ov) if per_variable else (r[0], o)

    def set_variables(self, var_elements: Sequence[int], multipliers: Optional[Sequence[float]] = None) -> None:
        """``cbx_sma_plan_set_variables``: the variables' float counts in offset
        order (summing to ``elements``) and their learning-rate multipliers
        (None: all 1).  Blocks; calling it again replaces the tables."""
        nv = len(var_elements)
        ve = (ctypes.c_longlong * max(1, nv))(*var_elements)
        if multipliers is not None and len(multipliers) != nv:
            raise ValueError(f"{len(multipliers)} multipliers for {nv} variables")
        mu = (ctypes.c_float * max(1, nv))(*multipliers) if multipliers is not None else None
        _raise(self.lib, self.lib.cbx_sma_plan_set_variables(self._p, ve, mu, nv), "cbx_sma_plan_set_variables")

    def optimise_variables(self, k: int, stream: int, w: int, g: int, last: Optional[int], s: int,
                           learning_rate: float, momentum: float, weight_decay: float, first_var: int,
                           nvars: int) -> None:
        """``cbx_sma_plan_optimise_variables``: one task's optimiser step on
        variables [first_var, first_var + nvars) of buffers on plan device
        ``k``, each variable with its own rate; asynchronous on ``stream``."""
        _raise(self.lib, self.lib.cbx_sma_plan_optimise_variables(
            self._p, k, stream or None, w, g, last or None, s, ctypes.c_float(learning_rate),
            ctypes.c_float(momentum), ctypes.c_float(weight_decay), first_var, nvars),
            "cbx_sma_plan_optimise_variables")

    def optimise_clipped(self, k: int, slot: int, stream: int, w: int, g: int, last: Optional[int], s: int,
                         learning_rate: float, momentum: float, weight_decay: float, max_norm: float,
                         skip_nonfinite: bool = False, use_variables: bool = False) -> None:
        """``cbx_sma_plan_optimise_clipped``: one task's optimiser step with
        gradient clipping by global L2 norm (``max_norm``; 0: none) and the
        non-finite skip, on plan device ``k``; asynchronous on ``stream``.
        ``slot`` in [0, 64) names the plan-owned record and slab."""
        _raise(self.lib, self.lib.cbx_sma_plan_optimise_clipped(
            self._p, k, slot, stream or None, w, g, last or None, s, ctypes.c_float(learning_rate),
            ctypes.c_float(momentum), ctypes.c_float(weight_decay), ctypes.c_float(max_norm),
            1 if skip_nonfinite else 0, 1 if use_variables else 0), "cbx_sma_plan_optimise_clipped")

    def gradient_norm(self, k: int, slot: int, stream: int, g: int, max_norm: float = 0.0,
                      skip_nonfinite: bool = False, loads: int = -1):
        """``cbx_sma_plan_gradient_norm``: the norm pass and the reduce alone
        over ``g`` (blocking).  Returns (the slot's record, pass ms, reduce
        ms), the times from the two dispatches' own timestamps."""
        a, b = ctypes.c_float(-1), ctypes.c_float(-1)
        _raise(self.lib, self.lib.cbx_sma_plan_gradient_norm(
            self._p, k, slot, stream or None, g, ctypes.c_float(max_norm), 1 if skip_nonfinite else 0, loads,
            ctypes.byref(a), ctypes.byref(b)), "cbx_sma_plan_gradient_norm")
        return self.clip_stats(k, slot, stream), a.value, b.value

    def clip_stats(self, k: int, slot: int, stream: int) -> dict:
        """``cbx_sma_plan_clip_stats``: the slot's record (blocks on
        ``stream``), as a dict of the fields of ``cbx_clip_stats``."""
        out = self.lib.cbx_sma_plan_clip_stats.argtypes[4]._type_()
        _raise(self.lib, self.lib.cbx_sma_plan_clip_stats(self._p, k, slot, stream or None, ctypes.byref(out)),
               "cbx_sma_plan_clip_stats")
        return {name: getattr(out, name) for name, _ in out._fields_}

    def set_buckets(self, buckets: int) -> None:
        """G > 1: buckets of the all-reduce pipeline (0 = default 8, 1 = in order)."""
        _raise(self.lib, self.lib.cbx_sma_plan_set_buckets(self._p, buckets), "cbx_sma_plan_set_buckets")

    def set_timing(self, on: bool) -> None:
        """One rank: every step's fused launch stamps its own start and stop."""
        _raise(self.lib, self.lib.cbx_sma_plan_set_timing(self._p, 1 if on else 0), "cbx_sma_plan_set_timing")

    def timing_history(self, count: int):
        """Kernel ms of the last ``count`` (at most 256) timed steps, oldest first."""
        buf = (ctypes.c_float * max(1, count))()
        got = _raise(self.lib, self.lib.cbx_sma_plan_timing_history(self._p, buf, count),
                     "cbx_sma_plan_timing_history")
        return [buf[k] for k in range(got)]

    def free(self) -> None:
        if self._p:
            self.lib.cbx_sma_plan_free(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def optimise_buffers(stream: int, w: int, g: int, last: Optional[int], s: int, elements: int,
                     learning_rate: float, momentum: float, weight_decay: float, lib=None) -> None:
    """``cbx_sma_optimise_buffers``: one task's replica optimiser step."""
    lib = lib if lib is not None else _default_lib()
    _raise(lib, lib.cbx_sma_optimise_buffers(stream or None, w, g, last or None, s, elements,
                                             ctypes.c_float(learning_rate), ctypes.c_float(momentum),
                                             ctypes.c_float(weight_decay)), "cbx_sma_optimise_buffers")


def ssgd_accumulate_buffers(stream: int, w: Optional[int], g: int, acc: int, elements: int, learning_rate: float,
                            weight_decay: float, lib=None) -> None:
    """``cbx_ssgd_accumulate_buffers``: one task's synchronous-SGD step."""
    lib = lib if lib is not None else _default_lib()
    _raise(lib, lib.cbx_ssgd_accumulate_buffers(stream or None, w or None, g, acc, elements,
                                                ctypes.c_float(learning_rate), ctypes.c_float(weight_decay)),
           "cbx_ssgd_accumulate_buffers")
