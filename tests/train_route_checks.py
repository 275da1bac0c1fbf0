"""The checks the training-route tests share (test_gpu_train_routes.py for the SDAV step, test_gpu_da_train_routes.py
for the DA step): a step is held to the oracle's STEP -- the change of each tensor against -lr * gradient, at 1e-9 of
the oracle's largest change -- and {loss, cd, cs, cc} each to 1e-10 of the oracle's own value.  Test infrastructure: no
test_* names here, so importing it from both files collects nothing twice."""
import numpy as np


def step_delta_ratio(before, after, dref):
    """max |(after - before) - dREF| / max |dREF| over one tensor."""
    before, after, dref = (np.asarray(a, dtype=np.float64) for a in (before, after, dref))
    scale = float(np.abs(dref).max())
    assert scale > 0.0, "the oracle does not move this tensor: nothing to compare"
    return float(np.abs((after - before) - dref).max()) / scale


def assert_step_delta(before, after, dref, bound=1e-9, what=""):
    """The change a step made to one parameter tensor is the oracle's change to within `bound` of its largest entry."""
    r = step_delta_ratio(before, after, dref)
    assert r <= bound, "%s: |dGPU - dREF| / max|dREF| = %.3g > %.0e" % (what, r, bound)
    return r


def assert_loss_parts(got, want, rel=1e-10, cc_floor=0.0):
    """{loss, cd, cs, cc}, each against its own oracle value.  cc_floor: an absolute allowance for cc alone (see
    CC_FLOOR in the two test files)."""
    for name, g, w in zip(("loss", "cd", "cs", "cc"), np.asarray(got), want):
        tol = rel * abs(w) + (cc_floor if name == "cc" else 0.0)
        assert abs(g - w) <= tol, "%s: %.17g vs %.17g" % (name, g, w)
