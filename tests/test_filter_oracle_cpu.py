"""The exact-integer model of the int8 arg-min filter (filter_oracle.py) and the data the GPU tests feed the kernels
(test_gpu_filter_verdicts.py), checked without a GPU:

  * the model IS the filter the header of csrc/gram_i8.hip describes: every d2 within Ed of the true |v_b|^2 - 2 v_a . v_b,
    every decided cell's arg-min the true one;
  * the data are sharp: a fifth of the cells undecided, dozens of cells exactly at the window's edge on either side,
    frame pairs with and without an undecided cell;
  * five subtly wrong variants of the arithmetic (a digit product lost, a k-step lost, rounding or truncating shifts) each
    change the undecided count of at least 3 frame pairs -- the observable the GPU tests compare with ==.

Chosen per shape (filter_oracle.SHAPES; N, P, H: amp, ncol, seed) and what the model shows there:

  shape            amp    ncol seed   W   undecided / cells     at W   at W + 1
  (16, 30, 1)      14000  1    3      6    1365 /   3600        105     131
  (20, 16, 63)     3000   2    1      6     373 /   3040         68      98
  (16, 32, 64)     3000   2    1      6     500 /   3840         96     129
  (40, 7, 65)      3000   2    1      6     830 /   5460        121     114
  (60, 2, 255)     1500   2    2      7     539 /   3540         64      54
  (44, 30, 256)    3000   2    1      8    5392 /  28380        694     830
  (24, 13, 257)    2500   2    1      8     751 /   3588        117      93
  (24, 30, 2500)   3000   8    1     25    2827 /   8280        142      72
  (300, 1, 64)     3000   2    1      6       0 /  44850          -       -      (P == 1: never undecided)
"""
from fractions import Fraction

import numpy as np
import pytest

import filter_oracle as fo

ALL_SHAPES = tuple(fo.SHAPES)
TABLE = {   # shape: (W, undecided, at W, at W + 1) -- the docstring's table, asserted below
    (16, 30, 1): (6, 1365, 105, 131), (20, 16, 63): (6, 373, 68, 98), (16, 32, 64): (6, 500, 96, 129),
    (40, 7, 65): (6, 830, 121, 114), (60, 2, 255): (7, 539, 64, 54), (44, 30, 256): (8, 5392, 694, 830),
    (24, 13, 257): (8, 751, 117, 93), (24, 30, 2500): (25, 2827, 142, 72), (300, 1, 64): (6, 0, 0, 0),
}


def true_d2(v, q):
    """|v_b|^2 - 2 v_a . v_b [a, b] of the fp64 values v to ~1e-13: v 2^24 = q + e exactly (e = v 2^24 - q is exact in
    fp64), q . q' in exact integers (12-bit halves through fp64 BLAS: every sum below 2^24 H), the terms with e -- 2^-24 of
    the whole -- in fp64."""
    e = v * 16777216.0 - q
    assert np.abs(e).max() <= 0.5
    qh = (q + 2048) >> 12
    ql = q - (qh << 12)
    mm = lambda a, b: np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)
    hl = mm(qh, ql)
    qq = (mm(qh, qh) << 24) + ((hl + hl.T) << 12) + mm(ql, ql)
    qf = q.astype(np.float64)
    qe = qf @ e.T
    dot = (qq.astype(np.float64) + (qe + qe.T + e @ e.T)) * 2.0 ** -48
    return np.diag(dot)[None, :] - 2.0 * dot


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_model_is_the_filter_the_header_describes(shape):
    x, m, r = fo.shape_model(shape)
    n, p, h = shape
    assert float(m.sv) == pytest.approx(fo.VMAX * h, rel=1e-12) and r.W == fo.window(fo.VMAX * h, h)
    c, inv = fo.centre_scale_matrix(x.reshape(n * p, h))
    cs, invs = fo.centre_scale_stream(h, 0.0, 1.0)
    assert np.array_equal(c, np.full(h, 0.5)) and inv == 0.996 and np.array_equal(c, cs) and inv == invs
    t = true_d2(m.v, m.q)
    # (the evaluation above against exact rational arithmetic, on a few cells)
    rng = np.random.RandomState(5)
    for a, b in rng.randint(0, n * p, size=(6, 2)):
        va, vb = [Fraction(f) for f in m.v[a].tolist()], [Fraction(f) for f in m.v[b].tolist()]
        exact = sum(f * f for f in vb) - 2 * sum(f * g for f, g in zip(va, vb))
        assert abs(float(Fraction(t[a, b]) - exact)) <= 1e-12
    ed = fo.bound_ed(m.sv, h)
    worst = np.abs(r.d2 * 2.0 ** -15 - t).max()
    assert worst + 1e-12 <= ed, (worst, ed)
    # every cell the model decides: bi is the first minimum of the true distances
    t4 = t.reshape(n, p, n, p).transpose(0, 2, 1, 3)
    tb = np.take_along_axis(t4, r.bi[..., None], axis=3)
    idx = np.arange(p)[None, None, None, :]
    beaten = np.where(idx < r.bi[..., None], t4 <= tb + 2e-12, t4 < tb - 2e-12)
    decided = np.triu(np.ones((n, n), dtype=bool), 1)[:, :, None] & ~r.undecided
    assert not (beaten.any(axis=3) & decided).any()
    assert (r.W, r.total, r.at_w, r.at_w1) == TABLE[shape]
    assert np.array_equal(r.pair_map, (r.pair_count > 0).astype(np.uint8)) and not np.tril(r.pair_count).any()
    assert np.array_equal(fo.stream_query_counts(r), r.undecided.sum(axis=(0, 2)))
    if p == 1:
        assert r.total == 0
    print(fo.summary_line(r, "model"))


@pytest.mark.parametrize("shape", fo.SHARP_SHAPES, ids=str)
def test_data_are_sharp(shape):
    x, m, r = fo.shape_model(shape)
    n = shape[0]
    assert x.min() == 0.0 and x.max() == 1.0 and np.array_equal(x * 2.0 ** 20, np.rint(x * 2.0 ** 20))
    share = r.total / r.cells
    assert 0.05 <= share <= 0.40, share
    assert r.at_w >= 20 and r.at_w1 >= 20, (r.at_w, r.at_w1)
    counts = r.pair_count[np.triu_indices(n, 1)]
    assert (counts == 0).mean() >= 0.10 and (counts > 0).mean() >= 0.10
    if shape in fo.PAIR_SHAPES:
        assert len(fo.boundary_pairs(r)) >= 10


@pytest.mark.parametrize("variant", fo.VARIANTS[1:])
@pytest.mark.parametrize("shape", fo.SHARP_SHAPES, ids=str)
def test_wrong_variants_change_frame_pair_counts(shape, variant):
    """A kernel that computed `variant` instead could not pass the GPU tests' == on the per-pair observables."""
    x, m, r = fo.shape_model(shape)
    w = m.verdicts(variant)
    changed = int((w.pair_count != r.pair_count).sum())
    assert changed >= 3, (shape, variant, changed)
    if shape in fo.STREAM_SHAPES:                                   # ... nor the stream tests' per-query counts
        assert (fo.stream_query_counts(w) != fo.stream_query_counts(r)).any()


@pytest.mark.parametrize("shape", fo.PAIR_SHAPES, ids=str)
def test_three_frame_subsets_keep_every_verdict(shape):
    """The sentinel frame pins range, scale and sv: the model run on (sentinel frame, i, j) alone counts what the whole
    data set's model counts for those three pairs."""
    x, m, r = fo.shape_model(shape)
    for i, j in fo.boundary_pairs(r)[:8]:
        frames = fo.subset_frames(i, j)
        sub = fo.filter_verdicts(x[frames])
        assert sub.W == r.W and sub.total == fo.subset_count(r, frames)
        assert np.array_equal(sub.pair_count, r.pair_count[np.ix_(frames, frames)])


def test_copy_rule_counts_fewer():
    key = ("copies",) + fo.PAIR_SHAPES[0]
    x, m, r = fo.shape_model(key)
    n = x.shape[0]
    assert np.array_equal(x[:, 1], x[:, 0]) and np.array_equal(x[:, 5], x[:, 4]) and np.array_equal(x[n - 1], x[2])
    assert m.copy[:, 1].all() and m.copy[:, 5].all() and m.copy[0, 2] and m.copy.sum() == 2 * n + 1
    without = m.verdicts(copies=False)
    assert without.total > r.total > 0
    assert (without.pair_count >= r.pair_count).all()
    # the window first, then the copies: a cell whose only runner-up inside the window is the best patch's twin is decided
    twin_only = without.undecided & ~r.undecided
    assert twin_only.any()
    print(fo.summary_line(r, "copies") + "; %d without the copy rule" % without.total)


def test_never_undecided():
    flat = np.full((5, 4, 70), 0.25)
    r = fo.filter_verdicts(flat)
    assert r.total == 0 and not r.pair_map.any()
    x, m, r1 = fo.shape_model((300, 1, 64))
    assert r1.total == 0 and (r1.gap == -1).all()


def test_unambiguity_check_raises():
    # a single column whose |v|^2 2^15 sits at a half-integer, and one that is far from any
    v = np.array([[np.sqrt(10.5 / 32768.0)]])
    assert abs(v[0, 0] ** 2 * 32768.0 - 10.5) < 1e-12 and len(fo.ambiguous_rows(v)) == 1
    with pytest.raises(fo.Ambiguous, match="half-integer"):
        fo.assert_unambiguous(v)
    assert len(fo.ambiguous_rows(np.array([[0.3]]))) == 0
    fo.assert_unambiguous(np.array([[0.3]]))
    # rows whose sum of |v| puts the window's ceil argument on an integer: (2 Ed(sv) + 1e-8) 32768 = 5 at 300 columns
    h = 300
    sv = (5.0 - fo.window_arg(0.0, h)) / (2.0 * 2.0 ** -23 * 32768.0)
    assert 0.0 < sv < fo.VMAX * h and abs(fo.window_arg(sv, h) - 5.0) < 1e-12
    with pytest.raises(fo.Ambiguous, match="ceil"):
        fo.assert_unambiguous(np.full((2, h), sv / h))
    fo.assert_unambiguous(np.full((2, h), 0.9 * sv / h))
