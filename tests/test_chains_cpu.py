"""CPU checks of the chains' NumPy oracle (tests/chains_oracle.py) itself: against a literal enumeration of every path,
the consequences include/dlc.h states for dlc_sequence_elastic_chains / dlc_sequence_chains, and what the chains are for --
the per-frame correspondences of a planted revisit at a changing speed."""
import itertools
import math

import numpy as np
import pytest

import chains_oracle as co
import elastic_oracle as eo
import sequence_oracle as so


def order_key(x):
    """Total order of the doubles as dlc_topk_rows_f64 ranks them: by the number, -0.0 below +0.0."""
    return (x, math.copysign(1.0, x))


def enumerate_best_paths(m, L, d_min, d_max, n, limit0, limit_step, lower):
    """chain [rows, n, L] (-1: no path) cell by cell: all (d_max - d_min + 1)^(L-1) step sequences, every path summed oldest
    row first in Python ints / floats; the best sum wins and, among equal sums, the path whose steps are lowest from the
    NEWEST row back -- what "the lowest d among equals" chooses level by level (the approach of
    test_elastic_cpu.enumerate_paths, keeping the path).  Also the best sums, as a dict.  For data without NaN partial sums
    and without wrapping."""
    rows = m.shape[0]
    is_int = m.dtype == np.int64
    lim = [min(max(limit0 + r * limit_step, 0), n) for r in range(rows)]
    chain = np.full((rows, n, L), -1, np.int32)
    sums = {}
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
                    best = (cand, total, cols[::-1])
            if best is not None:
                chain[r, j], sums[(r, j)] = best[2], best[1]
    return chain, sums


def all_columns(rows, n):
    return np.broadcast_to(np.arange(n, dtype=np.int64), (rows, n)).copy()


CASES = [(steps, lower, kind) for steps in ((0, 2), (0, 1), (1, 2), (0, 3), (1, 1), (2, 2)) for lower in (False, True)
         for kind in ("i64", "f64")]


@pytest.mark.parametrize("steps,lower,kind", CASES)
def test_oracle_chain_is_the_best_path_of_the_enumeration(steps, lower, kind):
    """Small integers: ties between paths are frequent, so the tie rule is exercised.  The oracle's chain attains the best
    path sum and, among equal sums, is the path the recursion's tie rule picks (sums are exact here, so a prefix that is
    best for its own cell is best for every chain through it)."""
    rng = np.random.RandomState(sum(steps) * 10 + lower + (kind == "f64") * 2)
    L, rows, n = 4, 7, 11
    if kind == "i64":
        m = rng.randint(-3, 4, size=(rows, n)).astype(np.int64)
    else:
        m = rng.randint(-8, 9, size=(rows, n)) / 4.0               # exact in fp64 in any order
    for limit0, step in ((n, 0), (5, 1)):
        want, sums = enumerate_best_paths(m, L, steps[0], steps[1], n, limit0, step, lower)
        chain, cells = co.elastic_chains(m, all_columns(rows, n), L, steps[0], steps[1], n, limit0, step, lower)
        assert (chain >= 0).any()
        assert np.array_equal(chain, want)
        total = co.sum_oldest_first(cells)
        for (r, j), s in sums.items():
            assert total[r, j] == s


@pytest.mark.parametrize("steps", [(0, 2), (1, 3), (2, 2), (0, 8)])
def test_all_equal_matrix_takes_the_lowest_step(steps):
    L, n = 5, 60
    for m in (np.full((8, n), 3, np.int64), np.full((8, n), 0.5)):
        chain, cells = co.elastic_chains(m, all_columns(8, n), L, steps[0], steps[1])
        first = (L - 1) * steps[0]                                  # columns left of it have no chain
        assert (chain[:L - 1] == -1).all() and (chain[L - 1:, :first] == -1).all()
        want = np.arange(first, n)[:, None] - (L - 1 - np.arange(L))[None, :] * steps[0]
        assert all(np.array_equal(chain[r, first:], want) for r in range(L - 1, 8))
        assert (cells[L - 1:, first:] == m[0, 0]).all()


@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("kind", ["i64", "f64", "f32"])
def test_stated_consequences(kind, lower):
    """chain[0] == j - span everywhere, the steps lie in [d_min, d_max], every column is below its row's limit, and the
    cells summed oldest first are E bit for bit (inexact fp64 sums included)."""
    rng = np.random.RandomState(3 + lower)
    rows, n, L, steps = 20, 70, 7, (0, 3)
    m = {"i64": lambda: rng.randint(-10 ** 6, 10 ** 6, size=(rows, n)).astype(np.int64),
         "f64": lambda: rng.standard_normal((rows, n)), "f32": lambda: rng.standard_normal((rows, n)).astype(np.float32)}[kind]()
    if kind != "i64":
        m[5, 7], m[9, 30], m[12, 40], m[13, 41] = np.nan, np.inf, 0.0, -0.0
    for limit0, step, row0 in ((None, 0, 0), (-8, 3, 2), (75, -1, L - 1)):
        e, span = eo.elastic_scores(m, L, steps[0], steps[1], None, limit0, step, lower, row0)
        idx = all_columns(rows - row0, n)
        chain, cells = co.elastic_chains(m, idx, L, steps[0], steps[1], None, limit0, step, lower, row0)
        valid = span >= 0
        assert valid.any() and not valid.all()
        assert np.array_equal(chain[..., L - 1], np.where(valid, idx, -1))
        assert np.array_equal(chain[..., 0], np.where(valid, idx - span, -1))
        assert (chain[~valid] == -1).all()
        d = np.diff(chain[valid], axis=1)
        assert d.min() >= steps[0] and d.max() <= steps[1]
        lim = so.limits(rows, n, n if limit0 is None else limit0, step)
        rho = (row0 + np.arange(rows - row0))[:, None, None] - (L - 1) + np.arange(L)[None, None, :]
        assert (chain[valid] < lim[np.where(valid[..., None], rho, 0)][valid]).all() and (chain[valid] >= 0).all()
        assert so.same_bits(np.where(valid, co.sum_oldest_first(cells), -1 if kind == "i64" else np.nan), e)


def test_length_one_chain_is_the_cell():
    m = np.arange(12, dtype=np.int64).reshape(3, 4)
    chain, cells = co.elastic_chains(m, [[0, 3], [2, -1], [4, 1]], 1, 0, 2, limit0=3, limit_step=0)
    assert chain[..., 0].tolist() == [[0, -1], [2, -1], [-1, 1]] and cells[..., 0].tolist() == [[0, -1], [6, -1], [-1, 9]]


def test_hand_worked_example():
    """The example of test_elastic_cpu.test_hand_worked_example: 3 x 5, L = 3, steps (0, 1), higher is better.
        row 0:  1  5  2  0  3        d_0 = 0 0 0 0 0
        row 1:  4  0  1  7  1        d_1 = 0 0 1 1 0
        row 2:  0  2  2  1  9        d_2 = 0 0 0 0 1
    column 4: level 2 steps back 1 to column 3, level 1 steps back 1 to column 2: chain 2 3 4, cells 2 7 9 = 18."""
    m = np.array([[1, 5, 2, 0, 3], [4, 0, 1, 7, 1], [0, 2, 2, 1, 9]], dtype=np.int64)
    chain, cells = co.elastic_chains(m, [[0], [0], [4]], 3, 0, 1)
    assert chain[:2].tolist() == [[[-1] * 3]] * 2
    assert chain[2, 0].tolist() == [2, 3, 4] and cells[2, 0].tolist() == [2, 7, 9]
    chain, cells = co.elastic_chains(m, [[2, 3, 1]], 3, 0, 1, row0=2)
    assert chain[0].tolist() == [[1, 2, 2], [2, 3, 3], [1, 1, 1]] and cells[0].tolist() == [[5, 1, 2], [2, 7, 1], [5, 0, 2]]


@pytest.mark.parametrize("kind", ["i64", "f64"])
def test_line_chains(kind):
    """The winning line's columns; the cells summed newest first are S bit for bit, the slope the search's."""
    from deeploopcloser_amd.sequence import slope_offsets
    rng = np.random.RandomState(11)
    rows, n, L = 14, 50, 6
    m = rng.randint(-99, 100, size=(rows, n)).astype(np.int64) if kind == "i64" else rng.standard_normal((rows, n))
    off = slope_offsets(L)
    for lower, limit0, step, row0 in ((False, None, 0, 0), (True, 30, 2, 3)):
        s, slope = so.sequence_scores(m, L, off, None, limit0, step, lower, row0)
        idx = all_columns(rows - row0, n)
        chain, cells, v = co.line_chains(m, idx, L, off, None, limit0, step, lower, row0)
        valid = slope >= 0
        assert valid.any() and not valid.all() and np.array_equal(v, slope)
        assert np.array_equal(chain[..., L - 1], np.where(valid, idx, -1)) and (chain[~valid] == -1).all()
        assert np.array_equal(chain[valid], idx[valid][:, None] - off[slope[valid]][:, ::-1])
        assert so.same_bits(np.where(valid, co.sum_newest_first(cells), -1 if kind == "i64" else np.nan), s)


def test_planted_revisit_chains_are_the_true_correspondences():
    """elastic_oracle.planted_elastic_revisit under the reference's distance (exclusion 30, L = 10, steps (0, 2), the steps
    the fixture was built for): at every one of the 51 frames whose chain lies inside the revisit -- the last revisiting
    frame included -- the top candidate's chain is true[...] for the 10 frames it covers, frame by frame: the aliases,
    each closer than the true place on its own frame, never enter a chain."""
    from oracle import distance as od
    x, true, alias, first = eo.planted_elastic_revisit()
    dist = np.array([[od.calculate_distance(a, b) for b in x] for a in x], dtype=np.int64)
    L, args = 10, dict(limit0=-30, limit_step=1, lower_is_better=True)
    s, idx, span = eo.elastic_topk(dist, 1, L, 0, 2, **args)
    chain, cells = co.elastic_chains(dist, idx, L, 0, 2, **args)
    last = first + 59
    assert np.array_equal(chain[last, 0], true[60 - L:])
    for i in range(L - 1, 60):
        assert np.array_equal(chain[first + i, 0], true[i - (L - 1):i + 1]), i
    assert np.array_equal(co.sum_oldest_first(cells)[first + L - 1:first + 60, 0], s[first + L - 1:first + 60, 0])
