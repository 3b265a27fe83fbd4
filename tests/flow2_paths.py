"""Catalogue of per-frame LM problems chosen for the Levenberg branch they reach (tests/test_flow2_paths.py asserts from the
oracle's trial log that each one does; tests/test_flow2_paths_gpu.py runs k_flow2_lm on them).

Every case is ``synth.make_flow2_problem`` plus at most two edits (``max_iterations``, one NaN in the measured flow).  Classes:

  rejection   runs of rejected trials inside an iteration (lambda *= ni; ni *= 2 more than once), an accepted trial after them,
              and rejections again in a later iteration.  Sizes: a cluster of 2 and of 3 workgroups on the register store, and
              2300 correspondences (more than one per thread: the memory store on a full cluster).
  iter_cap    the loop ends at max_iterations (0, 1, 3, and one object problem at its own 200): stop reason 0; 0 classifies the
              errors of the initial estimate.
  nonfinite   one NaN in the measured flow: every trial chi2 is NaN, nothing is ever accepted, every iteration re-linearises
              (the kernel's ``if (!built)``) and the loop ends at the problem's own 200-iteration cap.
  trial_cap   an iteration of 10 trials (ref_quirks = 0, 4 or 5 correspondences).  The cap is only ever hit at the rounding floor,
              so these trajectories are NOT stable under one-ulp changes of the inputs: they are compared between the kernel's two
              stores (same bits by construction), never trajectory for trajectory with the oracle.

``stable`` means: 8 copies with every obs / flow / depth double moved one ulp up or down at random give the same iterations,
trials, stop reason, trials per iteration and inlier flags, and a pose within 1e-11 (tests/test_flow2_paths.py).  Only such a
case can be compared with an implementation that sums in another order.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from vdo_slam_amd import synth

REJECTION, ITER_CAP, NONFINITE, TRIAL_CAP = "rejection", "iter_cap", "nonfinite", "trial_cap"
CLASSES = (REJECTION, ITER_CAP, NONFINITE, TRIAL_CAP)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    cls: str
    stable: bool
    n: int
    seed: int
    is_object: bool
    quirks: int
    sigma: float | None = None          # init_sigma_t (init_sigma_r = sigma / 10); None: the generator's defaults
    max_iterations: int | None = None   # None: the generator's (100 camera / 200 object)
    nan_at: int | None = None           # index of the correspondence whose measured flow x is NaN

    def build(self) -> synth.Flow2Problem:
        kw = {} if self.sigma is None else dict(init_sigma_t=self.sigma, init_sigma_r=self.sigma / 10)
        p = synth.make_flow2_problem(self.n, seed=self.seed, is_object=self.is_object, **kw)
        p.ref_quirks = self.quirks
        if self.max_iterations is not None:
            p.max_iterations = self.max_iterations
        if self.nan_at is not None:
            p.flow[self.nan_at, 0] = np.nan
        return p


def _kind(is_object):
    return "obj" if is_object else "cam"


def _rejection():
    # (quirks, n, seed, object): init_sigma_t = 5.0.  What the oracle does on them is pinned in tests/test_flow2_paths.py.
    rows = [(0, 260, 0, True), (0, 260, 1, False), (0, 260, 7, True), (0, 520, 2, False), (0, 520, 3, False), (0, 2300, 6, True), (0, 2300, 7, True),
            (1, 260, 2, False), (1, 260, 5, False), (1, 260, 3, True), (1, 520, 2, False), (1, 520, 1, True), (1, 2300, 0, False), (1, 2300, 5, True),
            (0, 2300, 10, False)]      # (the last one: rejection runs in three separate iterations on the memory store)
    return [Case(f"rej_q{q}_n{n}_s{s}_{_kind(o)}", REJECTION, True, n, s, o, q, sigma=5.0) for q, n, s, o in rows]


def _iter_cap():
    own = Case("cap200_q1_n3", ITER_CAP, True, 3, 14, True, 1)      # an object problem that runs into its own 200 iterations (the survey saw them at 3 and 4 points only)
    return [Case(f"cap{m}_q{q}_n{n}", ITER_CAP, True, n, 7, True, q, max_iterations=m) for n in (260, 2300) for q in (0, 1) for m in (0, 1, 3)] + [own]


def _nonfinite():
    # 3: inside chunk 0; 129: the last of chunk 0 (260 points on 2 workgroups), whose Hll diagonal crosses the cluster exchange; 259: the last point
    return [Case(f"nan{i}_q{q}_n260", NONFINITE, True, 260, 7, True, q, nan_at=i) for q in (0, 1) for i in (3, 129, 259)]


def _trial_cap():
    rows = [(4, 1, False, 1.0), (4, 5, True, 5.0), (4, 9, True, 1.0), (5, 3, False, 5.0), (5, 7, False, 5.0), (5, 10, True, 1.0)]
    return [Case(f"tcap_n{n}_s{s}_{_kind(o)}", TRIAL_CAP, False, n, s, o, 0, sigma=sg) for n, s, o, sg in rows]


CASES = _rejection() + _iter_cap() + _nonfinite() + _trial_cap()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases(cls=None, stable=None, quirks=None):
    return [c for c in CASES if (cls is None or c.cls == cls) and (stable is None or c.stable == stable) and (quirks is None or c.quirks == quirks)]
