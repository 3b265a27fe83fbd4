"""Host-side mirror of the per-frame joint pose+flow optimisers (thin ctypes wrapper).

``Flow2Batch`` corresponds to one call of ``Optimizer::PoseOptimizationFlow2Cam`` (camera) or
to the per-object loop over ``Optimizer::PoseOptimizationFlow2`` in ``Tracking::Track``
(reference src/Tracking.cc:697, 785-1001): all problems of a batch run in ONE kernel launch.

``Flow2Batch.reserve`` + ``set`` are the slots the frame pipeline uses (``vdo_flow2_batch_reserve`` / ``vdo_flow2_batch_set``):
capacities fixed once, every slot (re)defined or emptied before each run, results packed by the current sizes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K


class Flow2Batch:
    def __init__(self, ctx, problems):
        self.ctx = ctx
        self.problems = list(problems)
        self._keep = []
        arr = (K.Flow2ProblemC * len(self.problems))()
        for i, p in enumerate(self.problems):
            s, keep = K.flow2_to_c(p)
            arr[i] = s
            self._keep.append(keep)
        self._arr = arr
        self._h = C.c_void_p()
        K.check(K.lib().vdo_flow2_batch_create(ctx._h, len(self.problems), arr, C.byref(self._h)))
        ctx._retain()                                 # vdo_flow2_batch_destroy waits on the context's stream: the context must outlive the batch (ba.Context)

    @classmethod
    def reserve(cls, ctx, capacities):
        """A batch of ``len(capacities)`` empty slots of at most ``capacities[k]`` correspondences each: define them with :meth:`set`."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.problems = [None] * len(capacities)      # None: an empty slot (0 correspondences)
        self._keep = [None] * len(capacities)
        self._h = C.c_void_p()
        caps = np.ascontiguousarray(capacities, dtype=np.int32)
        K.check(K.lib().vdo_flow2_batch_reserve(ctx._h, len(caps), K._ip(caps), C.byref(self._h)))
        ctx._retain()
        return self

    def set(self, k, problem):
        """(Re)define slot ``k`` of a reserved batch; ``None`` empties it.  A refused call (:class:`VdoError`) leaves the slot as it was."""
        if problem is None:
            K.check(K.lib().vdo_flow2_batch_set(self._h, k, None))
        else:
            s, keep = K.flow2_to_c(problem)
            K.check(K.lib().vdo_flow2_batch_set(self._h, k, C.byref(s)))      # (the library copies the inputs into the slot)
        self.problems[k] = problem

    def set_T0(self, k, T0):
        """Rewrites the initial pose of slot ``k`` (vdo_flow2_batch_set_T0): the next run starts from it."""
        T = np.ascontiguousarray(T0, dtype=np.float64).reshape(16)
        L = K.lib()
        L.vdo_flow2_batch_set_T0.argtypes = [C.c_void_p, C.c_int, K.c_double_p]
        K.check(L.vdo_flow2_batch_set_T0(self._h, k, K._dp(T)))

    def run(self):
        K.check(K.lib().vdo_flow2_batch_run(self._h))

    def fetch(self):
        n = len(self.problems)
        res = (K.Flow2ResultC * n)()
        sizes = [p.n if p is not None else 0 for p in self.problems]
        flows = [np.zeros((m, 2)) for m in sizes]
        inl = [np.zeros(m, np.uint8) for m in sizes]
        fp = (K.c_double_p * n)(*[K._dp(f) for f in flows])
        ip = (K.c_uint8_p * n)(*[a.ctypes.data_as(K.c_uint8_p) for a in inl])
        K.check(K.lib().vdo_flow2_batch_fetch(self._h, res, fp, ip))
        out = []
        for i in range(n):
            out.append(dict(T=np.array(res[i].T).reshape(4, 4), n_inliers=res[i].n_inliers, iterations=res[i].iterations,
                            trials=res[i].trials, stop_reason=res[i].stop_reason, initial_chi2=res[i].initial_chi2,
                            final_chi2=res[i].final_chi2, final_lambda=res[i].final_lambda, flow=flows[i], inliers=inl[i]))
        return out

    def close(self):
        if self._h:
            K.lib().vdo_flow2_batch_destroy(self._h)
            self._h = C.c_void_p()
            self.ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
