"""CPU checks of place tracking: the NumPy oracle (tests/track_oracle.py) against a literal enumeration of every labelling,
its independence of the batching, the elastic search as its special case (include/dlc.h: dlc_track_rows, CONSEQUENCE),
and what the filter is for -- a traversal most of whose frames close no loop."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import elastic_oracle as eo
import sequence_oracle as so
import track_oracle as to


def enumerate_labellings(m, steps, jump, gate, null_score, lower, lim):
    """(V [rows][n], U [rows]) as Python ints, None = no labelling ends there: every sequence of states (a column below
    its row's limit, or -1 = nowhere when there is a no-loop state) of rows 0 .. r, summed: the cells of the places and
    null_score per nowhere, worsened per transition by 0 for a step in [d_min, d_max], `jump` for any other place and
    `gate` between a place and nowhere."""
    rows, n = m.shape
    states = list(range(n)) + ([-1] if null_score is not None else [])
    sign = 1 if lower else -1
    better = (lambda a, b: a < b) if lower else (lambda a, b: a > b)
    V = [[None] * n for _ in range(rows)]
    U = [None] * rows
    for r in range(rows):
        for seq in itertools.product(states, repeat=r + 1):
            if any(s >= lim[t] for t, s in enumerate(seq)):
                continue
            total = 0
            for t, s in enumerate(seq):
                total += null_score if s < 0 else int(m[t, s])
                if t:
                    p = seq[t - 1]
                    if (p < 0) != (s < 0):
                        total += sign * gate
                    elif s >= 0 and not steps[0] <= s - p <= steps[1]:
                        total += sign * jump
            if seq[-1] < 0:
                if U[r] is None or better(total, U[r]):
                    U[r] = total
            elif V[r][seq[-1]] is None or better(total, V[r][seq[-1]]):
                V[r][seq[-1]] = total
    return V, U


@pytest.mark.parametrize("seed", range(40))
def test_oracle_equals_the_enumeration_of_all_labellings(seed):
    rng = np.random.RandomState(seed)
    rows, n = int(rng.randint(1, 5)), int(rng.randint(1, 5))
    m = rng.randint(-4, 5, size=(rows, n)).astype(np.int64)
    d_min = int(rng.randint(0, 3))
    steps = (d_min, d_min + int(rng.randint(0, 3)))
    jump, gate = int(rng.randint(0, 4)), int(rng.randint(0, 4))
    null_score = int(rng.randint(-2, 3)) if seed % 3 else None
    lower = bool(seed & 1)
    limit0, step = (n, 0) if seed % 4 == 0 else (int(rng.randint(-1, n + 1)), int(rng.randint(-1, 2)))
    lim = so.limits(rows, n, limit0, step)
    o = to.track_rows(m, to.State(n, True), steps, jump, gate, np.nan if null_score is None else null_score, n, limit0, step, lower)
    V, U = enumerate_labellings(m, steps, jump, gate, null_score, lower, lim)
    want_v = np.array([[to.I64_MIN if v is None else v for v in row] for row in V], dtype=np.int64)
    want_u = np.array([to.I64_MIN if u is None else u for u in U], dtype=np.int64)
    assert np.array_equal(o["dense"], want_v) and np.array_equal(o["U"], want_u)
    assert np.array_equal(o["back"] == to.ABSENT, want_v == to.I64_MIN)
    # G, g and the filtered place follow from V and U
    for r in range(rows):
        there = [c for c in range(n) if V[r][c] is not None]
        if not there:
            assert o["g"][r] == -1 and o["G"][r] == to.I64_MIN and o["place"][r] == -1
            continue
        best = (min if lower else max)(V[r][c] for c in there)
        g = min(c for c in there if V[r][c] == best)
        beats = U[r] is None or (best < U[r] if lower else best > U[r])
        assert o["g"][r] == g and o["G"][r] == best and o["place"][r] == (g if beats else -1)
    # the back-traced labelling from every present end state attains the state's sum
    for end in list(range(n)) + [-1]:
        value = (U if end < 0 else [row[end] for row in V])[rows - 1]
        path = to.backtrace(o["back"], o["backU"], o["g"], end)
        if value is None:
            assert (path == to.NO_PATH).all()
            continue
        assert path[-1] == end and (path >= -1).all()
        total, sign = 0, 1 if lower else -1
        for t, s in enumerate(path):
            assert s < lim[t]
            total += null_score if s < 0 else int(m[t, s])
            if t:
                p = path[t - 1]
                if (p < 0) != (s < 0):
                    total += sign * gate
                elif s >= 0 and not steps[0] <= s - p <= steps[1]:
                    total += sign * jump
        assert total == value


def random_rows(rng, kind, rows, n):
    if kind == "i64":
        return rng.randint(-5, 6, size=(rows, n)).astype(np.int64)
    m = rng.standard_normal((rows, n))
    m[rng.rand(rows, n) < 0.03] = np.nan
    return m.astype(np.float32) if kind == "f32" else m


@pytest.mark.parametrize("kind,lower,null_score", [("i64", False, 4), ("f64", True, -1.5), ("f32", False, 1.5)])
def test_the_result_does_not_depend_on_the_batching(kind, lower, null_score):
    rng = np.random.RandomState(5)
    rows, n = 23, 37
    m = random_rows(rng, kind, rows, n)
    kw = dict(steps=(0, 2), jump=2, gate=1, null_score=null_score, lower_is_better=lower)
    whole_state = to.State(n, kind == "i64")
    whole = to.track_rows(m, whole_state, limit0=20, limit_step=1, **kw)
    assert (whole["place"] >= 0).any() and (whole["place"] < 0).any()
    for batch in (1, 3, 7):
        state, parts = to.State(n, kind == "i64"), []
        for lo in range(0, rows, batch):
            parts.append(to.track_rows(m[lo:lo + batch], state, limit0=20 + lo, limit_step=1, **kw))
        for name, want in whole.items():
            assert so.same_bits(np.concatenate([p[name] for p in parts]), want), (batch, name)
        assert so.same_bits(state.V, whole_state.V) and np.array_equal(state.head(), whole_state.head())


@pytest.mark.parametrize("steps,lower", [((0, 2), False), ((1, 3), True), ((2, 2), False)])
def test_row_L_minus_1_equals_the_elastic_search(steps, lower):
    """jump = 2^40 and no no-loop state: a chain of moves beats anything with a jump in it, so wherever the elastic search
    offers a cell of row L - 1 the tracker's V is that cell's score."""
    rng = np.random.RandomState(11)
    L, n = 6, 41
    m = rng.randint(-1000, 1000, size=(L, n)).astype(np.int64)
    for limit0, step in ((n, 0), (30, 2), (45, -1)):
        o = to.track_rows(m, to.State(n, True), steps, 1 << 40, 0, np.nan, n, limit0, step, lower)
        e, span = eo.elastic_scores(m, L, steps[0], steps[1], n, limit0, step, lower)
        offered = span[L - 1] >= 0
        assert offered.any() and np.array_equal(o["dense"][L - 1][offered], e[L - 1][offered])
        assert (o["backU"] == to.ABSENT).all() and (o["U"] == to.I64_MIN).all()
        assert (o["place"] == o["g"]).all()                        # without a no-loop state the filter always names a place


def test_signed_zero_nan_and_the_first_row():
    # the first row takes the origin, which is +0.0: 0.0 + -0.0 = +0.0
    m = np.array([[-0.0, np.nan, 1.0]])
    s = to.State(3, False)
    o = to.track_rows(m, s, (0, 1), 1.0, 1.0, 0.5)
    assert o["back"][0].tolist() == [to.ORIGIN, to.ABSENT, to.ORIGIN] and np.isnan(o["dense"][0, 1])
    assert not np.signbit(o["dense"][0, 0]) and o["g"][0] == 2 and o["place"][0] == 2
    assert o["U"][0] == 0.5 and o["backU"][0] == to.ORIGIN and s.seen == 1
    # second row: column 0 stays (d = 0: 0.0) or jumps (1.0 - 1.0 = 0.0) or leaves nowhere (0.5 - 1.0): the move wins the tie
    o = to.track_rows(np.array([[0.0, 5.0, np.nan]]), s, (0, 1), 1.0, 1.0, 0.5)
    assert o["back"][0].tolist() == [0, 1, to.ABSENT] and o["dense"][0, :2].tolist() == [0.0, 5.0]
    assert o["U"][0] == 1.0 and o["backU"][0] == 0 and o["place"][0] == 1
    # a row that offers nothing: only nowhere survives, and the next row comes out of it
    o = to.track_rows(np.full((1, 3), np.nan), s, (0, 1), 1.0, 1.0, 0.5)
    assert o["g"][0] == -1 and o["place"][0] == -1 and o["U"][0] == 4.5 and o["backU"][0] == to.JUMP
    o = to.track_rows(np.array([[1.0, 1.0, 1.0]]), s, (0, 1), 1.0, 1.0, 0.5)
    assert o["back"][0].tolist() == [to.FROM_NULL] * 3 and o["dense"][0].tolist() == [4.5] * 3 and o["place"][0] == -1


def thresholded(m, truth):
    """The fewest frames any single threshold on a row's maximum gets wrong (the place is the row's arg-max)."""
    best, arg = m.max(axis=1), m.argmax(axis=1)
    return min(int((np.where(best >= t, arg, -1) != truth).sum()) for t in np.concatenate([best, [np.inf]]))


PLANTED_SEEDS = (0, 1, 2)


@pytest.mark.parametrize("seed", PLANTED_SEEDS)
def test_planted_traversal(seed):
    """120 frames against 100 key-frames, two revisits at a changing speed in N(0, 1) noise: the back-traced labelling
    differs from the truth in at most 2 frames; the best single threshold on the row maximum misses many times that."""
    m, truth = to.planted_traversal(seed)
    place, path, G, U = to.track_places(m, (0, 2), 4.0, 4.0, 2.0)
    missed, single = int((path != truth).sum()), thresholded(m, truth)
    print("seed %d: back-traced path misses %d frames, filtered place %d, best threshold %d"
          % (seed, missed, int((place != truth).sum()), single))
    assert missed <= 2
    assert single >= 5 * max(missed, 1)


def test_cli_argument_rules():
    """--track needs --sequence and three numbers, JUMP and GATE not negative; --track-steps needs --track and 0 <= DMIN <= DMAX <= 8
    (refused while the arguments are parsed: no GPU is touched)."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = ("--network", "seqslam", "--metric", "sad", "--sequence", "2")
    for args in (("--track", "1:1:1"), common + ("--track", "-1:1"), common + ("--track-steps", "0:2", "--track", "1:1:1:1"),
                 common + ("--track", "1:1:1", "--track-steps", "0:9")):
        bad = subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                             capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
        assert bad.returncode == 2 and "error:" in bad.stderr and "--track" in bad.stderr, args
