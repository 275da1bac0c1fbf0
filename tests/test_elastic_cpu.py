"""CPU checks of the elastic sequence search: the NumPy oracle (tests/elastic_oracle.py) against a literal enumeration of
every path, hand-worked cases of the recursion in include/dlc.h (dlc_sequence_elastic_topk), its stated consequences, and
what the search is for -- a planted revisit at a changing speed, which no straight line follows."""
import itertools
import math
import struct

import numpy as np
import pytest

import elastic_oracle as eo
import sequence_oracle as so


def order_key(x):
    """Total order of the doubles as dlc_topk_rows_f64 ranks them: by the number, -0.0 below +0.0."""
    return (x, math.copysign(1.0, x))


def enumerate_paths(m, L, d_min, d_max, n, limit0, limit_step, lower):
    """(E, span) cell by cell: all (d_max - d_min + 1)^(L-1) step sequences, every path summed oldest row first in Python
    ints / floats; the best sum wins and, among equal sums, the path whose steps are lowest from the NEWEST row back --
    what "the lowest d among equals" chooses level by level.  For data without NaN partial sums and without wrapping."""
    rows = m.shape[0]
    is_int = m.dtype == np.int64
    lim = [min(max(limit0 + r * limit_step, 0), n) for r in range(rows)]
    E = np.full((rows, n), -1 if is_int else np.nan, np.int64 if is_int else np.float64)
    span = np.full((rows, n), -1, np.int32)
    for r in range(L - 1, rows):
        for j in range(n):
            best = None
            for steps in itertools.product(range(d_min, d_max + 1), repeat=L - 1):   # steps[0]: between rows r and r - 1
                cols = [j]
                for d in steps:
                    cols.append(cols[-1] - d)                      # cols[s]: the column in row r - s
                if any(not 0 <= c < lim[r - s] for s, c in enumerate(cols)):
                    continue
                total = None
                for s in range(L - 1, -1, -1):                      # oldest row first
                    e = int(m[r - s, cols[s]]) if is_int else float(m[r - s, cols[s]])
                    total = e if total is None else total + e
                merit = total if is_int else order_key(total)
                if lower:
                    merit = -merit if is_int else tuple(-c for c in merit)
                cand = (merit, tuple(-d for d in steps))            # larger = better; then the lower steps, newest first
                if best is None or cand > best[0]:
                    best = (cand, total, j - cols[-1])
            if best is not None:
                E[r, j], span[r, j] = best[1], best[2]
    return E, span


CASES = [(steps, lower, kind) for steps in ((0, 2), (0, 1), (1, 2), (0, 3), (1, 1), (2, 2)) for lower in (False, True)
         for kind in ("i64", "f64")]


@pytest.mark.parametrize("steps,lower,kind", CASES)
def test_oracle_equals_the_enumeration_of_all_paths(steps, lower, kind):
    """Ties between paths are frequent (small integers), so the tie rule is exercised: with the recursion, the lowest d at
    the last level wins among equal sums, then the lowest d one level down, ... -- and a prefix that is best for its own
    cell is best for every chain through it, since the addition is monotone and these sums are exact."""
    rng = np.random.RandomState(sum(steps) * 10 + lower + (kind == "f64") * 2)
    L, rows, n = 4, 7, 11
    if kind == "i64":
        m = rng.randint(-3, 4, size=(rows, n)).astype(np.int64)
    else:
        m = rng.randint(-8, 9, size=(rows, n)) / 4.0               # exact in fp64 in any order
    for limit0, step in ((n, 0), (5, 1)):
        e, sp = eo.elastic_scores(m, L, steps[0], steps[1], n, limit0, step, lower)
        le, lsp = enumerate_paths(m, L, steps[0], steps[1], n, limit0, step, lower)
        assert so.same_bits(e, le)
        assert (sp >= 0).any()
        # the span of the chosen chain: equal sums may be reached by chains of different spans, and the recursion's
        # choice is the level-by-level lowest d, which is the enumeration's tie rule
        assert np.array_equal(sp, lsp)


def test_hand_worked_example():
    """3 x 5, L = 3, steps (0, 1), higher is better.
        row 0:  1  5  2  0  3        A_0 = 1 5 2 0 3                    spans 0 0 0 0 0
        row 1:  4  0  1  7  1        P_1 = 1 5 5 2 3 (d: 0 0 1 1 0)     A_1 = 5 5 6 9 4      spans 0 0 1 1 0
        row 2:  0  2  2  1  9        P_2 = 5 5 6 9 9 (d: 0 0 0 0 1)     A_2 = 5 7 8 10 18    spans 0 0 1 1 2
    (column 1 at level 1: A_0(1) = 5 against A_0(0) = 1 -> d = 0; column 1 at level 2: 5 = 5 -> the lowest d, 0.)"""
    m = np.array([[1, 5, 2, 0, 3], [4, 0, 1, 7, 1], [0, 2, 2, 1, 9]], dtype=np.int64)
    e, sp = eo.elastic_scores(m, 3, 0, 1)
    assert e[:2].tolist() == [[-1] * 5] * 2 and sp[:2].tolist() == [[-1] * 5] * 2
    assert e[2].tolist() == [5, 7, 8, 10, 18] and sp[2].tolist() == [0, 0, 1, 1, 2]
    s, i, v = eo.elastic_topk(m, 3, 3, 0, 1)
    assert s[2].tolist() == [18, 10, 8] and i[2].tolist() == [4, 3, 2] and v[2].tolist() == [2, 1, 1]
    # lower is better: P_1 = 1 1 2 0 0 (d: 0 1 0 0 1), A_1 = 5 1 3 7 1, spans 0 1 0 0 1;
    #                  P_2 = 5 1 1 3 1 (d: 0 0 1 1 0), A_2 = 5 3 3 4 10, spans 0 1 2 1 1
    e, sp = eo.elastic_scores(m, 3, 0, 1, lower_is_better=True)
    assert e[2].tolist() == [5, 3, 3, 4, 10] and sp[2].tolist() == [0, 1, 2, 1, 1]
    # with the rows' limits 3, 4, 5 (limit0 = 3, limit_step = 1) column 3 of row 0 and column 4 of rows 0, 1 are gone
    e, sp = eo.elastic_scores(m, 3, 0, 1, limit0=3, limit_step=1)
    assert e[2].tolist() == [5, 7, 8, 10, 18] and sp[2].tolist() == [0, 0, 1, 1, 2]
    e, sp = eo.elastic_scores(m, 3, 1, 1, limit0=3, limit_step=1)   # fixed step 1: columns 0, 1 have no chain
    assert e[2].tolist() == [-1, -1, 3, 7, 18] and sp[2].tolist() == [-1, -1, 2, 2, 2]


@pytest.mark.parametrize("steps", [(0, 2), (1, 3), (2, 2), (0, 8)])
def test_all_equal_matrix_takes_the_lowest_step(steps):
    L, n = 5, 60
    for m in (np.full((8, n), 3, np.int64), np.full((8, n), 0.5)):
        e, sp = eo.elastic_scores(m, L, steps[0], steps[1])
        first = (L - 1) * steps[0]                                  # columns left of it have no chain
        assert (sp[L - 1:, first:] == first).all() and (sp[L - 1:, :first] == -1).all() and (sp[:L - 1] == -1).all()
        assert (e[L - 1:, first:] == m[0, 0] * L).all()
        s, i, v = eo.elastic_topk(m, 4, L, steps[0], steps[1])
        assert i[L - 1].tolist() == list(range(first, first + 4))  # ties -> the lower column


@pytest.mark.parametrize("d", [0, 1, 2])
def test_fixed_step_equals_the_linear_search(d):
    rng = np.random.RandomState(10 + d)
    m = rng.randint(-1000, 1000, size=(40, 90)).astype(np.int64)
    L = 6
    line = [[s * d for s in range(L)]]
    for lower, limit0, step in ((False, None, 0), (True, -5, 3), (True, 95, -1)):
        s, i, v = eo.elastic_topk(m, 7, L, d, d, None, limit0, step, lower, 2)
        ls, li, lv = so.sequence_topk(m, 7, L, line, None, limit0, step, lower, 2)
        assert np.array_equal(s, ls) and np.array_equal(i, li)
        assert np.array_equal(v, np.where(li >= 0, (L - 1) * d, -1))
        e, sp = eo.elastic_scores(m, L, d, d, None, limit0, step, lower)
        le, _ = so.sequence_scores(m, L, line, None, limit0, step, lower)
        assert np.array_equal(e, le)


def test_length_one_is_the_plain_topk():
    rng = np.random.RandomState(4)
    m = rng.standard_normal((5, 30))
    m[1, 3], m[2, 4], m[2, 5] = np.nan, np.inf, -0.0
    for lower in (False, True):
        s, i, v = eo.elastic_topk(m, 6, 1, 0, 2, None, 25, -4, lower)
        ls, li, lv = so.sequence_topk(m, 6, 1, [[0]], None, 25, -4, lower)
        assert so.same_bits(s, ls) and np.array_equal(i, li) and np.array_equal(v, np.where(li >= 0, 0, -1))


def test_nan_signed_zero_and_opposite_infinities():
    nan, inf = np.nan, np.inf
    # a NaN element is no predecessor and no cell: the chain goes round it where the steps allow
    m = np.array([[1.0, nan, 4.0], [nan, 2.0, 1.0]])
    e, sp = eo.elastic_scores(m, 2, 0, 1)
    #   A_0 = 1 nan 4 (valid: yes no yes);  P_1 = 1, 1 (d = 1), 4;  A_1 = nan (element), 3, 5
    assert np.isnan(e[1, 0]) and e[1, 1:].tolist() == [3.0, 5.0] and sp[1].tolist() == [-1, 1, 0]
    # -0.0 ranks below +0.0: the predecessor +0.0 at d = 1 beats -0.0 at d = 0 when higher is better, and -0.0 + -0.0
    # keeps its sign
    m = np.array([[0.0, -0.0], [-0.0, -0.0]])
    e, sp = eo.elastic_scores(m, 2, 0, 1)
    assert [struct.pack(">d", x)[0] for x in e[1]] == [0, 0] and sp[1].tolist() == [0, 1]    # 0.0 + -0.0 = +0.0, twice
    e, sp = eo.elastic_scores(m, 2, 0, 1, lower_is_better=True)
    assert [struct.pack(">d", x)[0] for x in e[1]] == [0, 0x80] and sp[1].tolist() == [0, 0]  # column 1: -0.0 + -0.0
    # one (+inf, -inf) window, higher is better, L = 3, steps (0, 1):
    #   row 0:  +inf  1      A_0 = +inf 1
    #   row 1:  -inf  2      P_1 = +inf, +inf (d = 1)    A_1 = NaN (not valid), +inf                 spans -, 1
    #   row 2:   5    7      P_2 = none, +inf (d = 0)    A_2 = not valid, +inf                        spans -, 1
    # The recursion decides: the path 1 -> 2 -> 7 = 10 through column 1 alone is finite, but P_1(1) chose +inf, and the
    # cell's value is +inf; column 0's only chains run through the NaN.
    m = np.array([[inf, 1.0], [-inf, 2.0], [5.0, 7.0]])
    e, sp = eo.elastic_scores(m, 3, 0, 1)
    assert np.isnan(e[2, 0]) and e[2, 1] == inf and sp[2].tolist() == [-1, 1]
    # lower is better: P_1 = +inf, 1 (d = 0)   A_1 = NaN, 3    P_2 = none, 3   A_2 = not valid, 10
    e, sp = eo.elastic_scores(m, 3, 0, 1, lower_is_better=True)
    assert np.isnan(e[2, 0]) and e[2, 1] == 10.0 and sp[2].tolist() == [-1, 0]
    s, i, v = eo.elastic_topk(m, 2, 3, 0, 1, lower_is_better=True)
    assert s[2].tolist() == [10.0, inf] and i[2].tolist() == [1, -1] and v[2].tolist() == [0, -1]


def test_int64_wraps():
    big = np.iinfo(np.int64).max
    m = np.array([[big, 0], [1, 0]], dtype=np.int64)
    e, sp = eo.elastic_scores(m, 2, 0, 1)
    # column 0: big + 1 wraps to the minimum.  Column 1: P_1 = max(A_0(1) = 0, A_0(0) = big) = big (d = 1), + 0
    assert e[1].tolist() == [np.iinfo(np.int64).min, big] and sp[1].tolist() == [0, 1]


def test_planted_revisit_at_a_changing_speed():
    """300 int8 frames: frames 220-279 revisit key-frames 40.. at 0, 1 or 2 key-frames per frame, and every revisiting
    frame has a closer alias at a scattered older index (elastic_oracle.planted_elastic_revisit).  Under the reference's
    distance (exclusion 30, L = 10) the single-frame arg-min is the alias every time; straight lines follow the revisit
    for about half of the 51 frames whose chain lies inside it, 21 slopes no better than five; the elastic search with
    steps (0, 2) finds every one, with the span the true chain has."""
    from deeploopcloser_amd.sequence import slope_offsets
    from oracle import distance as od
    x, true, alias, first = eo.planted_elastic_revisit()
    dist = np.array([[od.calculate_distance(a, b) for b in x] for a in x], dtype=np.int64)
    L, args = 10, dict(limit0=-30, limit_step=1, lower_is_better=True)
    _, i1, _ = so.sequence_topk(dist, 1, 1, [[0]], **args)
    assert np.array_equal(i1[first:first + 60, 0], alias) and int((i1[first:first + 60, 0] == true).sum()) == 0
    want = true[L - 1:]
    _, il, _ = so.sequence_topk(dist, 1, L, slope_offsets(L), **args)
    linear = int((il[first + L - 1:first + 60, 0] == want).sum())
    _, iw, _ = so.sequence_topk(dist, 1, L, slope_offsets(L, 0.0, 2.0, 0.1), **args)
    wide = int((iw[first + L - 1:first + 60, 0] == want).sum())
    _, ie, se = eo.elastic_topk(dist, 1, L, 0, 2, **args)
    elastic = ie[first + L - 1:first + 60, 0]
    print("true place found of 51: linear %d, 21 slopes %d, elastic %d" % (linear, wide, int((elastic == want).sum())))
    assert want.size == 51 and np.array_equal(elastic, want)
    assert np.array_equal(se[first + L - 1:first + 60, 0], true[L - 1:] - true[:60 - (L - 1)])
    assert linear <= 30 and linear == PLANTED_LINEAR and wide == PLANTED_WIDE


PLANTED_LINEAR, PLANTED_WIDE = 26, 28          # the counts of this construction (pinned: the generator is seeded)
