"""CPU checks of the ground-truth evaluation: tests/evaluate_oracle.py (the NumPy restatement the GPU tests compare with)
against brute-force Python loops, evaluate.ground_truth / pr_curve_queries / PRCurve on hand-made cases, the two new
entry points of the C ABI as far as they go without a GPU, and the CLI's new argument errors."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import evaluate_oracle as eo

VALUES = {"f64": [-2.5, -0.0, 0.0, 1.0, 1.5, 3.25, -1e-300, 1e300],
          "f32": [-2.5, -0.0, 0.0, 1.0, 1.5, 3.25, -1e-30, 1e30],
          "i64": [-5, -1, 0, 3, 7, 1 << 40, -(1 << 50), 9]}
DTYPES = {"f64": np.float64, "f32": np.float32, "i64": np.int64}


def small_case(rng, kind, rows, n):
    m = np.asarray(VALUES[kind], DTYPES[kind])[rng.randint(0, 8, size=(rows, n))]
    if kind != "i64":
        m[rng.randint(0, 6, size=m.shape) == 0] = np.nan
        m[0, 0], m[-1, -1] = np.inf, -np.inf
    return m, (rng.randint(0, 3, size=(rows, n)) == 0).astype(np.uint8) * 7


def below(a, b):
    """a < b in the order of the numbers with -0.0 below +0.0, in plain Python."""
    if isinstance(a, int):
        return a < b
    za, zb = (struct.pack(">d", v)[0] >> 7 for v in (a, b))        # the sign bits
    return a < b or (a == b == 0.0 and za > zb)


def offered(m, r, j, lim, absent):
    v = m[r, j].item()
    return j < lim and v == v and not (absent is not None and v == absent)


# ---- the oracle against loops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "f32", "i64"])
@pytest.mark.parametrize("lower", [False, True])
def test_oracle_bins_are_direct_counts(kind, lower):
    rng = np.random.RandomState(7 + lower)
    m, truth = small_case(rng, kind, 5, 11)
    own = np.asarray(VALUES[kind], DTYPES[kind])
    table = eo.sort_thresholds(np.concatenate([own, own[:3]]), kind == "i64")       # the data's own values: the tie side
    assert table.size == 8                                                          # -0.0 and +0.0 are two thresholds
    for limit0, step, absent in ((None, 0, None), (3, 2, None), (9, -3, 3 if kind == "i64" else None)):
        pos, neg = eo.pr_cell_counts(m, truth, table, limit0=limit0, limit_step=step, lower_is_better=lower, absent=absent)
        lim = eo.limits(5, 11, limit0, step)
        cells = [(m[r, j].item(), truth[r, j] != 0) for r in range(5) for j in range(11) if offered(m, r, j, lim[r], absent)]
        assert pos.sum() + neg.sum() == len(cells) and pos.size == neg.size == 9
        for i, t in enumerate(table.tolist()):
            # x >= t_i <=> bin > i;  lower is better: x <= t_i <=> bin <= i
            reported = [(x, p) for x, p in cells if (not below(t, x) if lower else not below(x, t))]
            tp, fp = sum(p for _, p in reported), sum(not p for _, p in reported)
            assert (tp, fp) == ((pos[:i + 1].sum(), neg[:i + 1].sum()) if lower else (pos[i + 1:].sum(), neg[i + 1:].sum()))
        t2, tp, fp, positives = eo.curve_from_counts(pos, neg, table, lower)
        assert positives == sum(p for _, p in cells) and (np.diff(tp) >= 0).all() and (np.diff(fp) >= 0).all()


@pytest.mark.parametrize("kind", ["f64", "f32", "i64"])
@pytest.mark.parametrize("lower", [False, True])
def test_oracle_rank_is_the_position_in_a_stable_sort(kind, lower):
    import functools
    rng = np.random.RandomState(11 + lower)
    m, truth = small_case(rng, kind, 6, 13)
    truth[2] = 0                                                                    # a row without a positive
    for limit0, step, absent in ((None, 0, None), (2, 2, None), (13, -3, 3 if kind == "i64" else None)):
        rank, idx, npos = eo.positive_rank_rows(m, truth, limit0=limit0, limit_step=step, lower_is_better=lower, absent=absent)
        lim = eo.limits(6, 13, limit0, step)
        for r in range(6):
            cols = [j for j in range(13) if offered(m, r, j, lim[r], absent)]
            better = (lambda a, b: below(a, b)) if lower else (lambda a, b: below(b, a))
            cmp = lambda a, b: -1 if better(m[r, a].item(), m[r, b].item()) else (1 if better(m[r, b].item(), m[r, a].item()) else 0)
            ranking = sorted(cols, key=functools.cmp_to_key(cmp))                   # stable: ties keep the lower column first
            places = [s for s, j in enumerate(ranking) if truth[r, j]]
            assert npos[r] == len(places)
            assert (rank[r], idx[r]) == ((places[0], ranking[places[0]]) if places else (-1, -1))
        assert (rank[2], idx[2], npos[2]) == (-1, -1, 0)


# ---- ground_truth -----------------------------------------------------------------------------------------------------------
def test_ground_truth_against_a_loop():
    from deeploopcloser_amd import evaluate as ev
    big = 1 << 30
    rng = np.random.RandomState(3)
    q = np.concatenate([rng.randint(-20, 21, size=(9, 2)), [[big, big], [-big, -big], [big, -big], [0, 0]]]).astype(np.int64)
    k = np.concatenate([rng.randint(-20, 21, size=(12, 2)), [[-big, -big], [big, big], [-big, big], [3, 4]]]).astype(np.int64)
    # 3037000499^2 < 2^63 = the squared distance of opposite corners <= 3037000500^2; 2^31 reaches along one axis only
    for radius in (0, 5, 17, 1 << 31, 3037000499, 3037000500, 1 << 40):
        got = ev.ground_truth(torch.from_numpy(q), torch.from_numpy(k), radius)
        assert got.dtype == torch.uint8 and got.shape == (13, 16) and got.device.type == "cpu"
        want = [[int(eo.within(a, b, radius)) for b in k] for a in q]
        assert got.tolist() == want, radius
    got = ev.ground_truth(q[:, 0], k[:, 0], 7)                                      # frame indices: the 1-D case, NumPy in
    assert got.tolist() == [[int(abs(int(a) - int(b)) <= 7) for b in k[:, 0]] for a in q[:, 0]]
    wide = ev.ground_truth(np.arange(3000), np.arange(5000), 2)                     # several row tiles
    assert wide.shape == (3000, 5000) and int(wide.sum()) == 5 * 3000 - 2 - 1
    for bad in (lambda: ev.ground_truth(q, k[:, 0], 1), lambda: ev.ground_truth(q, k, -1), lambda: ev.ground_truth(q, k, 1.5),
                lambda: ev.ground_truth(q.astype(np.float64), k, 1), lambda: ev.ground_truth(q + big, k, 1),
                lambda: ev.ground_truth(q[:, :1], k[:, :1], 1)):
        with pytest.raises(ValueError):
            bad()


# ---- pr_curve_queries and the summary numbers -------------------------------------------------------------------------------
def summary(curve):
    return curve.average_precision, curve.recall_at_full_precision, curve.best_f1


def same_as_oracle(curve, scores, ids, hit, has, lower):
    t, tp, fp, positives = eo.queries_curve(scores, ids, hit, has, lower)
    assert np.array_equal(curve.thresholds, t) and np.array_equal(curve.tp, tp) and np.array_equal(curve.fp, fp)
    assert curve.positives == positives and curve.tp.dtype == curve.fp.dtype == np.int64
    p, r = eo.precision_recall(tp, fp, positives)
    assert np.array_equal(curve.precision, p) and np.array_equal(curve.recall, r)
    assert summary(curve) == (eo.average_precision(tp, fp, positives), eo.recall_at_full_precision(tp, fp, positives),
                              eo.best_f1(tp, fp, positives, t))


def test_queries_hand_made_cases():
    from deeploopcloser_amd import evaluate as ev
    yes, no = np.ones(4, bool), np.zeros(4, bool)
    s, i = np.array([0.9, 0.8, 0.8, 0.1]), np.array([3, 1, 2, 0])
    # all correct: precision 1 throughout, everything found at the loosest threshold
    c = ev.pr_curve_queries(s, i, yes, yes)
    assert c.thresholds.tolist() == [0.9, 0.8, 0.1] and c.tp.tolist() == [1, 3, 4] and c.fp.tolist() == [0, 0, 0]
    assert summary(c) == (1.0, 1.0, (1.0, 0.1)) and c.precision.tolist() == [1.0] * 3 and c.recall.tolist() == [0.25, 0.75, 1.0]
    same_as_oracle(c, s, i, yes, yes, False)
    # none reported
    c = ev.pr_curve_queries(s, np.full(4, -1), no, yes)
    assert len(c) == 0 and c.positives == 4 and summary(c) == (0.0, 0.0, (0.0, None))
    same_as_oracle(c, s, np.full(4, -1), no, yes, False)
    # a wrong match at the top score: no recall at full precision
    hit = np.array([False, True, True, True])
    c = ev.pr_curve_queries(s, i, hit, yes)
    assert c.tp.tolist() == [0, 2, 3] and c.fp.tolist() == [1, 1, 1] and c.recall_at_full_precision == 0.0
    assert c.precision.tolist() == [0.0, 2 / 3, 0.75] and c.average_precision == 0.5 * (2 / 3) + 0.25 * 0.75
    assert c.best_f1 == (2 * 3 / (2 * 3 + 1 + 1), 0.1)
    same_as_oracle(c, s, i, hit, yes, False)
    # positives == 0: recall 0 everywhere, every report a false positive
    c = ev.pr_curve_queries(s, i, no, no)
    assert c.positives == 0 and c.recall.tolist() == [0.0] * 3 and c.fp.tolist() == [1, 3, 4] and summary(c) == (0.0, 0.0, (0.0, 0.9))
    same_as_oracle(c, s, i, no, no, False)
    # lower is better, integer scores, a row without a candidate, a query without a true match
    s, i = np.array([40, 10, 10, 70, 55], np.int64), np.array([2, 0, -1, 1, 3])
    hit, has = np.array([True, True, False, False, True]), np.array([True, True, True, False, True])
    c = ev.pr_curve_queries(s, i, hit, has, lower_is_better=True)
    assert c.thresholds.tolist() == [10, 40, 55, 70] and c.tp.tolist() == [1, 2, 3, 3] and c.fp.tolist() == [0, 0, 0, 1]
    assert c.positives == 4 and c.recall_at_full_precision == 0.75 and c.best_f1 == (6 / 7, 55)
    same_as_oracle(c, s, i, hit, has, True)
    rng = np.random.RandomState(5)
    for lower in (False, True):
        s, i = rng.randint(0, 6, size=40).astype(np.float64), rng.randint(-1, 9, size=40)
        s[rng.randint(0, 40, size=3)] = np.nan
        hit, has = rng.randint(0, 2, size=40) == 1, rng.randint(0, 3, size=40) > 0
        same_as_oracle(ev.pr_curve_queries(s, i, hit & has, has, lower), s, i, hit & has, has, lower)
    with pytest.raises(ValueError):
        ev.pr_curve_queries(s, i[:5], hit, has)


def test_evaluator_flags_against_loops():
    """LoopClosureEvaluator.add on hand-made candidate lists (host arrays): hit, any-of-k and has_positive."""
    from deeploopcloser_amd import evaluate as ev
    rng = np.random.RandomState(9)
    positions = rng.randint(0, 6, size=(30, 2)).astype(np.int64)
    judge = ev.LoopClosureEvaluator(positions, 2, 3, lower_is_better=True)
    flags, scores, ids = [], [], []
    for first in range(0, 30, 7):
        b = min(7, 30 - first)
        i = np.stack([rng.randint(-1, max(1, first + r)) * np.ones(2, np.int64) + [0, 1] for r in range(b)])
        i = np.clip(i, -1, 29)
        s = rng.randint(0, 50, size=(b, 2)).astype(np.int64)
        judge.add(s, i, first)
        flags.append(eo.detector_flags(positions, 2, 3, first, i))
        scores.append(s[:, 0])
        ids.append(i[:, 0])
    hit, any_hit, has = (np.concatenate([f[c] for f in flags]) for c in range(3))
    curve, candidates_recall = judge.result()
    assert judge.queries == 30 and has.any() and hit.any()
    same_as_oracle(curve, np.concatenate(scores), np.concatenate(ids), hit, has, True)
    assert candidates_recall == any_hit.sum() / has.sum()
    assert ev.pr_line(30, curve) == eo.pr_line(30, curve.tp, curve.fp, curve.positives, curve.thresholds)
    with pytest.raises(ValueError):
        judge.add(s, i, 29)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeploopcloser_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deeploopcloser_amd", "csrc"), "-j4"])
    return _lib.load()


def test_library_exports_and_host_side_checks(lib):
    from deeploopcloser_amd import _lib
    import deeploopcloser_amd as dlc
    for name in ("dlc_pr_cell_counts", "dlc_pr_cell_counts_workspace_bytes", "dlc_positive_rank_rows",
                 "dlc_positive_rank_rows_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dlc_pr_cell_counts(None, _lib.DLC_F64, p, 1, 1, 1, 1, 0, 0, 0, 0, p, 1, p, 1, p, p, p, 64, None) == _lib.DLC_ERR_BAD_ARG
    assert lib.dlc_positive_rank_rows(None, _lib.DLC_F64, p, 1, 1, 1, 1, 0, 0, 0, 0, p, 1, p, p, p, p, 64, None) == _lib.DLC_ERR_BAD_ARG
    w = lib.dlc_pr_cell_counts_workspace_bytes
    assert w(20000, 20000, 1000) > 0 and w(20000, 20000, 1000) % 256 == 0 and w(1, 1, 1) == 256
    assert w(20000, 20000, 4096) <= 32 << 20 and w(1 << 40, (1 << 31) - 1, 4096) <= 32 << 20
    for rows, n, t in ((8, 50, 0), (8, 50, 4097), (8, 1 << 31, 5), (0, 50, 5), (8, 0, 5), (8, 50, -1)):
        assert w(rows, n, t) == 0, (rows, n, t)
    w = lib.dlc_positive_rank_rows_workspace_bytes
    assert w(20000, 20000) == 20000 * 32 and w(1, 1) == 256 and w(3, 70_001) == (3 * 69 * 32 + 255) // 256 * 256
    for rows, n in ((8, 1 << 31), (0, 50), (8, 0)):
        assert w(rows, n) == 0, (rows, n)
    assert lib.dlc_abi_version() == 20
    for name in ("ground_truth", "pr_curve_cells", "recall_at", "pr_curve_queries", "PRCurve", "LoopClosureEvaluator"):
        assert getattr(dlc.evaluate, name) is getattr(dlc, name) and name in dlc.__all__


# ---- the CLI's new argument errors --------------------------------------------------------------------------------------------
def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_argument_errors(tmp_path):
    """Raised by argparse (exit status 2, usage on stderr) before an engine is created: they do not need a GPU."""
    frames = len([f for f in os.listdir(os.path.join(GOLDEN, "datasets_test")) if f.endswith(".ppm")])
    good, short, words, three = (str(tmp_path / name) for name in ("good.txt", "short.txt", "words.txt", "three.txt"))
    open(good, "w").write("".join("%d\n" % t for t in range(frames)))
    open(short, "w").write("".join("%d 0\n" % t for t in range(frames - 1)))
    open(words, "w").write("".join("here\n" for t in range(frames)))
    open(three, "w").write("".join("1 2 3\n" for t in range(frames)))
    seqslam = ("--network", "seqslam", "--metric", "sad")
    for args in (seqslam + ("--radius", "2"), seqslam + ("--pr-curve", str(tmp_path / "curve.tsv")),
                 seqslam + ("--positions", good), seqslam + ("--positions", good, "--radius", "-1"),
                 seqslam + ("--positions", short, "--radius", "2"), seqslam + ("--positions", words, "--radius", "2"),
                 seqslam + ("--positions", three, "--radius", "2"),
                 seqslam + ("--positions", str(tmp_path / "missing.txt"), "--radius", "2")):
        res = run_cli(*args)
        assert res.returncode == 2 and "error:" in res.stderr and "usage:" in res.stderr, (args, res.stderr)
        assert res.stdout == "" and not os.path.exists(str(tmp_path / "curve.tsv"))
