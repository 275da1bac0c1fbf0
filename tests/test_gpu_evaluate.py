"""GPU ground-truth evaluation (dlc_pr_cell_counts, dlc_positive_rank_rows, Engine.pr_cell_counts / positive_rank_rows,
evaluate.pr_curve_cells / recall_at / LoopClosureEvaluator, --positions on the CLI) against the NumPy restatement of the
definitions (tests/evaluate_oracle.py, pinned by test_evaluate_cpu.py).  Everything is integer counting: every comparison
is exact.  The matrices are built as tests/test_gpu_peaks.py builds them: eight values with -0.0 and 0.0 among them, NaN in
one cell in sixteen, infinities, rows that start at an odd element, a winning value in the columns past n."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import evaluate_oracle as eo
from test_gpu_peaks import ABSENT, KINDS, PEAKS, SENTINEL, SIZES, VALUES, data, np_dtype, on_device, winner

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 17)
TS = (1, 2, 7, 8, 63, 64, 65, 4096)
TRUTHS = ("none", "all", "quarter")


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def limit_cases(n):
    """(limit0, limit_step): every step of {-1, 0, 1}, limits that reach 0 and limits that reach n."""
    return [(None, 0), (-3, 1), (n - 8, 1), (n + 2, -1), (5, -1)]


def truth_mask(rng, kind, rows, n):
    if kind == "none":
        return np.zeros((rows, n), np.uint8)
    if kind == "all":
        return rng.randint(1, 256, size=(rows, n)).astype(np.uint8)               # any non-zero byte
    return (rng.randint(0, 4, size=(rows, n)) == 0).astype(np.uint8) * rng.randint(1, 256, size=(rows, n)).astype(np.uint8)


def truth_on_device(e, t, ldt):
    """t [rows, n] as the first n columns of a [rows, ldt] device view that starts at an odd byte; the rest is non-zero."""
    rows, n = t.shape
    flat = torch.full((rows * ldt + 1,), 255, dtype=torch.uint8, device=e.device)
    buf = flat[1:].view(rows, ldt)
    buf[:, :n] = torch.from_numpy(t).to(e.device)
    return buf


def threshold_table(rng, kind, count):
    """`count` distinct thresholds, shuffled, some given twice: the data's own values first (the tie side of the bin rule),
    then the planted peaks and the infinities, then others."""
    own = np.asarray(VALUES[kind], np_dtype(kind))[rng.permutation(8)]
    if kind == "i64":
        extra = np.array(list(PEAKS[kind]) + [np.iinfo(np.int64).min, np.iinfo(np.int64).max], np.int64)
        fill = rng.randint(-(1 << 62), 1 << 62, size=2 * count).astype(np.int64)
    else:
        extra = np.array(list(PEAKS[kind]) + [np.inf, -np.inf], np_dtype(kind))
        fill = (rng.standard_normal(2 * count) * 3).astype(np_dtype(kind))
    pool = np.concatenate([own, extra, fill]).astype(np.int64 if kind == "i64" else np.float64)
    _, first = np.unique(eo.order_keys(pool), return_index=True)
    table = pool[np.sort(first)][:count]                                          # the first `count` distinct ones, in pool order
    assert table.size == count
    return np.concatenate([table, table[:3]])[rng.permutation(count + min(3, count))]


def check_counts(e, buf, tbuf, m, t, table, **kw):
    pos, neg = e.pr_cell_counts(buf, tbuf, table, n=m.shape[1], **kw)
    want = eo.pr_cell_counts(m, t, eo.sort_thresholds(table, m.dtype == np.int64), **kw)
    assert pos.dtype == neg.dtype == torch.int64
    assert np.array_equal(pos.cpu().numpy(), want[0]) and np.array_equal(neg.cpu().numpy(), want[1]), (m.shape, table.size, kw)
    return want


# ---- counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_counts_exact_against_the_definition(dlc, kind, n):
    e = dlc.default_engine()
    rng = np.random.RandomState(4000 + 31 * KINDS.index(kind) + n)
    case = 0
    for rows in ROWS:
        m = data(rng, kind, rows, n)
        truths = {name: truth_mask(rng, name, rows, n) for name in TRUTHS}
        tbufs = {name: truth_on_device(e, t, n + 3) for name, t in truths.items()}
        for lower in (False, True):
            buf = on_device(e, m, n + 5, winner(kind, lower))                      # the tail columns would top every bin
            for limit0, step in limit_cases(n):
                for turn in range(2):                                              # every T and every truth comes round several times
                    count, name = TS[case % len(TS)], TRUTHS[case % len(TRUTHS)]
                    case += 1
                    kw = dict(limit0=limit0, limit_step=step, lower_is_better=lower)
                    if kind == "i64" and case % 2:
                        kw["absent"] = ABSENT
                    pos, neg = check_counts(e, buf, tbufs[name], m, truths[name], threshold_table(rng, kind, count), **kw)
                    offered = eo.offered_mask(m, n, limit0, step, kw.get("absent")).sum()
                    assert pos.sum() + neg.sum() == offered and (name != "none" or pos.sum() == 0) and (name != "all" or neg.sum() == 0)


@pytest.mark.parametrize("kind", KINDS)
def test_counts_every_cell_in_one_bin(dlc, kind):
    """The contention path: every lane of every wave adds to the same two words."""
    e = dlc.default_engine()
    rng = np.random.RandomState(77)
    m = np.full((64, 4097), VALUES[kind][3], np_dtype(kind))
    t = truth_mask(rng, "quarter", 64, 4097)
    buf, tbuf = on_device(e, m, 4097 + 5, winner(kind, False)), truth_on_device(e, t, 4097 + 3)
    for count in (1, 64, 4096):
        for lower in (False, True):
            pos, neg = check_counts(e, buf, tbuf, m, t, threshold_table(rng, kind, count), lower_is_better=lower)
            assert np.count_nonzero(pos) == 1 and np.count_nonzero(neg) == 1 and pos.sum() + neg.sum() == 64 * 4097


@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_counts_several_workgroups_a_row(dlc, kind):
    """300 x 5000: three chunks a row, 900 items -- one workgroup each at T = 65, a grid that strides at T = 4096."""
    e = dlc.default_engine()
    rng = np.random.RandomState(78)
    m, t = data(rng, kind, 300, 5000), truth_mask(rng, "quarter", 300, 5000)
    buf, tbuf = on_device(e, m, 5000 + 5, winner(kind, True)), truth_on_device(e, t, 5000 + 3)
    for count in (65, 4096):
        for kw in (dict(), dict(limit0=4000, limit_step=5, lower_is_better=True), dict(limit0=5100, limit_step=-20)):
            check_counts(e, buf, tbuf, m, t, threshold_table(rng, kind, count), **kw)


def test_counts_do_not_depend_on_the_batch(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(79)
    m, t = data(rng, "f64", 33, 2500), truth_mask(rng, "quarter", 33, 2500)
    buf, tbuf = on_device(e, m, 2505, np.inf), truth_on_device(e, t, 2503)
    table = threshold_table(rng, "f64", 100)
    whole = check_counts(e, buf, tbuf, m, t, table, limit0=2400, limit_step=7)
    for size in (1, 5):
        parts = [e.pr_cell_counts(buf[lo:lo + size], tbuf[lo:lo + size], table, n=2500, limit0=2400 + 7 * lo, limit_step=7)
                 for lo in range(0, 33, size)]
        assert np.array_equal(sum(p[0] for p in parts).cpu().numpy(), whole[0])
        assert np.array_equal(sum(p[1] for p in parts).cpu().numpy(), whole[1])


# ---- ranks ----------------------------------------------------------------------------------------------------------------
def check_ranks(e, buf, tbuf, m, t, **kw):
    got = e.positive_rank_rows(buf, tbuf, n=m.shape[1], **kw)
    want = eo.positive_rank_rows(m, t, **kw)
    for g, w, what in zip(got, want, ("rank", "idx", "npos")):
        assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w), (what, m.shape, kw)
    return got


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_ranks_exact_and_the_slot_of_the_topk_list(dlc, kind, n):
    e = dlc.default_engine()
    rng = np.random.RandomState(5000 + 31 * KINDS.index(kind) + n)
    case = 0
    for rows in ROWS:
        m = data(rng, kind, rows, n)
        truths = {name: truth_mask(rng, name, rows, n) for name in TRUTHS}
        truths["quarter"][rows // 2] = 0                                           # a row without a positive among the others
        tbufs = {name: truth_on_device(e, t, n + 3) for name, t in truths.items()}
        for lower in (False, True):
            buf = on_device(e, m, n + 5, winner(kind, lower))
            for limit0, step in limit_cases(n):
                name = TRUTHS[case % len(TRUTHS)]
                case += 1
                kw = dict(limit0=limit0, limit_step=step, lower_is_better=lower)
                if kind == "i64" and case % 2:
                    kw["absent"] = ABSENT
                rank, idx, npos = check_ranks(e, buf, tbufs[name], m, truths[name], **kw)
                if name == "none":
                    assert bool((rank == -1).all()) and bool((idx == -1).all()) and bool((npos == 0).all())
                # the consequence the header states: rank is the slot of idx in the row's top-k list
                _, lists = e.peak_topk_rows(buf, 128, 0, n=n, **kw)
                inside = (rank >= 0) & (rank < 128)
                assert bool((lists[inside, rank[inside]] == idx[inside]).all())
                assert bool(((rank >= 0) == (npos > 0)).all())


@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_ranks_slabs_and_whole_rows(dlc, kind):
    """300 x 5000 (five slabs a row: three launches), 2100 x 1100 (a workgroup per row: one launch) and 2 x 70 001."""
    e = dlc.default_engine()
    rng = np.random.RandomState(80)
    for rows, n in ((300, 5000), (2100, 1100), (2, 70_001)):
        m, t = data(rng, kind, rows, n), truth_mask(rng, "quarter", rows, n)
        t[::7] = 0
        t[1::7, 1:], t[1::7, 0] = 0, 9                                             # one positive, at column 0
        buf, tbuf = on_device(e, m, n + 5, winner(kind, False)), truth_on_device(e, t, n + 3)
        for kw in (dict(), dict(limit0=n - 900, limit_step=3, lower_is_better=True), dict(limit0=n + 100, limit_step=-20)):
            rank, idx, npos = check_ranks(e, buf, tbuf, m, t, **kw)
            assert bool((rank[::7] == -1).all())
    some = [e.positive_rank_rows(buf[lo:lo + 1], tbuf[lo:lo + 1], n=n, limit0=n + 100 - 20 * lo, limit_step=-20) for lo in (0, 1)]
    assert all(torch.equal(torch.cat([s[c] for s in some]), (rank, idx, npos)[c]) for c in range(3))   # a row alone


# ---- the C entry points: fully written outputs, errors that write nothing ---------------------------------------------------
def test_outputs_fully_written_and_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    lib, T = e.lib, 5
    m = torch.arange(8 * 50, dtype=torch.float64, device=e.device).view(8, 50)
    truth = torch.zeros((8, 50), dtype=torch.uint8, device=e.device)
    truth[:, 10] = 1
    table = torch.tensor([0.0, 10.0, 100.0, 200.0, 399.0], dtype=torch.float64, device=e.device)
    outs = [torch.full((T + 1,), SENTINEL, dtype=torch.int64, device=e.device) for _ in range(2)]
    outs += [torch.full((8,), SENTINEL, dtype=torch.int64, device=e.device) for _ in range(3)]
    need_c, need_r = lib.dlc_pr_cell_counts_workspace_bytes(8, 50, T), lib.dlc_positive_rank_rows_workspace_bytes(8, 50)
    assert need_c == 8 * 2 * (T + 1) * 8 and need_r == 256       # eight workgroups' partials; 32 bytes a row
    ws = torch.empty(need_c, dtype=torch.uint8, device=e.device)
    src, tr, tb, wp = (C.c_void_p(t.data_ptr()) for t in (m, truth, table, ws))
    op, on, o1, o2, o3 = (C.c_void_p(t.data_ptr()) for t in outs)
    F64 = _lib.DLC_F64
    names_c = ["ctx", "dtype", "scores", "rows", "n", "ld", "limit0", "step", "lower", "has_absent", "absent", "truth", "ldt",
               "thr", "T", "pos", "neg", "ws", "bytes", "stream"]
    ok_c = (e.ctx, F64, src, 8, 50, 50, 50, 0, 0, 0, 0, tr, 50, tb, T, op, on, wp, need_c, None)
    names_r = names_c[:13] + ["rank", "idx", "npos", "ws", "bytes", "stream"]
    ok_r = ok_c[:13] + (o1, o2, o3, wp, need_r, None)

    def but(names, ok, **change):
        return tuple(change.get(name, v) for name, v in zip(names, ok))

    # nothing offered: all zero / (-1, -1, 0), DLC_OK, every word written
    assert lib.dlc_pr_cell_counts(*but(names_c, ok_c, limit0=0)) == _lib.DLC_OK
    assert lib.dlc_positive_rank_rows(*but(names_r, ok_r, limit0=-7, step=1)) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert outs[0].tolist() == [0] * 6 and outs[1].tolist() == [0] * 6
    assert outs[2].tolist() == [-1] * 8 and outs[3].tolist() == [-1] * 8 and outs[4].tolist() == [0] * 8
    for o in outs:
        o.fill_(SENTINEL)
    assert lib.dlc_pr_cell_counts(*ok_c) == _lib.DLC_OK and lib.dlc_positive_rank_rows(*ok_r) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert outs[0].tolist() == [0, 0, 2, 2, 4, 0] and outs[1].tolist() == [0, 10, 88, 98, 195, 1]    # cell (r, j) holds 50 r + j; column 10 is true
    assert outs[2].tolist() == [39] * 8 and outs[3].tolist() == [10] * 8 and outs[4].tolist() == [1] * 8
    for o in outs:
        o.fill_(SENTINEL)
    both = {"dtype": dict(dtype=_lib.DLC_I8), "null scores": dict(scores=None), "null truth": dict(truth=None), "rows 0": dict(rows=0),
            "n 0": dict(n=0), "ld < n": dict(ld=49), "ld_truth < n": dict(ldt=49), "absent with fp64": dict(has_absent=1),
            "misaligned scores": dict(scores=C.c_void_p(m.data_ptr() + 4))}
    for f, names, ok, who, more in (
            (lib.dlc_pr_cell_counts, names_c, ok_c, b"pr_cell_counts",
             {"null thresholds": dict(thr=None), "null pos": dict(pos=None), "null neg": dict(neg=None), "T 0": dict(T=0),
              "T 4097": dict(T=4097), "misaligned thresholds": dict(thr=C.c_void_p(table.data_ptr() + 4))}),
            (lib.dlc_positive_rank_rows, names_r, ok_r, b"positive_rank_rows",
             {"null rank": dict(rank=None), "null idx": dict(idx=None), "null npos": dict(npos=None)})):
        for what, change in dict(both, **more).items():
            assert f(*but(names, ok, **change)) == _lib.DLC_ERR_BAD_ARG, what
            assert who in lib.dlc_last_error(e.ctx), what
        assert f(*but(names, ok, ctx=None)) == _lib.DLC_ERR_BAD_ARG
        assert f(*but(names, ok, n=1 << 31, ld=1 << 31, ldt=1 << 31)) == _lib.DLC_ERR_BAD_SHAPE
        for change in (dict(ws=None), dict(bytes=ok[names.index("bytes")] - 1)):
            assert f(*but(names, ok, **change)) == _lib.DLC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs), "an error wrote to the outputs"
    # the engine's own checks
    for call in (lambda: e.pr_cell_counts(m, truth, []), lambda: e.pr_cell_counts(m, truth, [1.0, float("nan")]),
                 lambda: e.pr_cell_counts(m, truth, np.arange(4097.0)), lambda: e.pr_cell_counts(m, truth[:7], [1.0]),
                 lambda: e.pr_cell_counts(m, truth.cpu(), [1.0]), lambda: e.pr_cell_counts(m, truth, [1.0], absent=3),
                 lambda: e.pr_cell_counts(m.to(torch.int64), truth, [1.5]), lambda: e.positive_rank_rows(m, truth[:, :49]),
                 lambda: e.positive_rank_rows(m, truth.to(torch.int32)), lambda: e.positive_rank_rows(m, truth, n=51)):
        with pytest.raises(ValueError):
            call()
    pos, neg = e.pr_cell_counts(m, truth != 0, [399.0, 0.0, 10.0, 200.0, 100.0, 10.0])                # a bool mask; any order
    assert pos.tolist() == [0, 0, 2, 2, 4, 0] and neg.tolist() == [0, 10, 88, 98, 195, 1]


# ---- the module's surface -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_module_functions(dlc, kind):
    e = dlc.default_engine()
    rng = np.random.RandomState(90)
    m, t = data(rng, kind, 40, 300), truth_mask(rng, "quarter", 40, 300)
    t[5] = 0
    absent = dict(absent=ABSENT) if kind == "i64" else {}
    for lower in (False, True):
        kw = dict(limit0=-3, limit_step=9, lower_is_better=lower, **absent)
        table = threshold_table(rng, kind, 30)
        for scores, truth in ((m, t), (torch.from_numpy(m).to(e.device), torch.from_numpy(t).to(e.device))):
            curve = dlc.pr_curve_cells(scores, truth, table, **kw)
            ascending = eo.sort_thresholds(table, kind == "i64")
            wt, tp, fp, positives = eo.curve_from_counts(*eo.pr_cell_counts(m, t, ascending, **kw), ascending, lower)
            assert np.array_equal(eo.order_keys(curve.thresholds), eo.order_keys(wt)) and curve.positives == positives
            assert np.array_equal(curve.tp, tp) and np.array_equal(curve.fp, fp)
            p, r = eo.precision_recall(tp, fp, positives)
            assert np.array_equal(curve.precision, p) and np.array_equal(curve.recall, r)
            assert curve.average_precision == eo.average_precision(tp, fp, positives)
            assert curve.recall_at_full_precision == eo.recall_at_full_precision(tp, fp, positives)
            assert curve.best_f1 == eo.best_f1(tp, fp, positives, wt)
            recalls, rank = dlc.recall_at(scores, truth, ks=(1, 5, 300), **kw)
            wrank, _, wnpos = eo.positive_rank_rows(m, t, **kw)
            assert isinstance(rank, torch.Tensor) and np.array_equal(rank.cpu().numpy(), wrank)
            assert recalls == {k: int(((wrank >= 0) & (wrank < k)).sum()) / int((wnpos > 0).sum()) for k in (1, 5, 300)}
            assert recalls[300] == 1.0
        # T evenly spaced thresholds over the finite offered range
        curve = dlc.pr_curve_cells(m, t, 12, **kw)
        off = eo.offered_mask(m, 300, -3, 9, absent.get("absent"))
        cells = m[off] if kind == "i64" else m[off & np.isfinite(m)]
        lo, hi = cells.min().item(), cells.max().item()
        want = sorted({lo + (i * (hi - lo)) // 11 for i in range(12)}) if kind == "i64" else np.linspace(float(lo), float(hi), 12).tolist()
        assert sorted(curve.thresholds.tolist()) == list(want)
    assert dlc.recall_at(m, np.zeros_like(t))[0] == {1: 0.0, 5: 0.0, 10: 0.0, 20: 0.0}


# ---- end to end: a detector, and the CLI ------------------------------------------------------------------------------------
FRAMES = sorted(glob.glob(os.path.join(GOLDEN, "datasets_test", "*.ppm")))
POSITIONS = [t % 6 for t in range(len(FRAMES))]                        # a route that passes the same six places again and again
RADIUS, EXCLUSION = 1, 2


def test_evaluator_on_the_seqslam_detector(dlc):
    from deeploopcloser_amd import pipeline
    from deeploopcloser_amd.input import read_ppm
    net = dlc.SeqSlam(size=(32, 64))
    desc = pipeline.seqslam_descriptors_from_frames(np.stack([read_ppm(f) for f in FRAMES]), net)
    for k, batch in ((1, 4), (3, 5)):
        det = dlc.SeqSlamLoopClosureDetector(desc.shape[1], k=k, exclusion=EXCLUSION, capacity=64)
        judge = dlc.LoopClosureEvaluator(np.array(POSITIONS), RADIUS, EXCLUSION, lower_is_better=True)
        lists = []
        for lo in range(0, len(FRAMES), batch):
            s, i = det.query_and_insert(desc[lo:lo + batch])
            judge.add(s, i, lo)
            lists.append((s.cpu().numpy(), i.cpu().numpy(), lo))
        curve, candidates_recall = judge.result()
        flags = [eo.detector_flags(POSITIONS, RADIUS, EXCLUSION, lo, i) for _, i, lo in lists]
        hit, any_hit, has = (np.concatenate([f[c] for f in flags]) for c in range(3))
        t, tp, fp, positives = eo.queries_curve(np.concatenate([s[:, 0] for s, _, _ in lists]),
                                                np.concatenate([i[:, 0] for _, i, _ in lists]), hit, has, True)
        assert judge.queries == len(FRAMES) and positives == has.sum() > 0 and len(t) > 1
        assert np.array_equal(curve.thresholds, t) and np.array_equal(curve.tp, tp) and np.array_equal(curve.fp, fp)
        assert curve.positives == positives and candidates_recall == any_hit.sum() / has.sum()
        assert curve.average_precision == eo.average_precision(tp, fp, positives)


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_positions(dlc, tmp_path):
    positions, out = str(tmp_path / "positions.txt"), str(tmp_path / "curve.tsv")
    open(positions, "w").write("".join("%d\n" % p for p in POSITIONS))
    base = ("--network", "seqslam", "--metric", "sad", "--k", "1", "--exclusion", str(EXCLUSION), "--batch", "4")
    res = run_cli(*base, "--positions", positions, "--radius", str(RADIUS), "--pr-curve", out)
    assert res.returncode == 0, res.stdout + res.stderr
    loops = [l.split("\t") for l in res.stdout.splitlines() if l.startswith("loop\t")]
    assert loops and len(loops) == len({l[1] for l in loops})                    # k = 1: at most one line a frame
    scores, ids = np.zeros(len(FRAMES), np.int64), np.full(len(FRAMES), -1, np.int64)
    for l in loops:
        ids[int(l[1])], scores[int(l[1])] = int(l[3]), int(l[5])
    hit, _, has = eo.detector_flags(POSITIONS, RADIUS, EXCLUSION, 0, ids[:, None])
    t, tp, fp, positives = eo.queries_curve(scores, ids, hit, has, True)
    lines = [l for l in res.stderr.splitlines() if l.startswith("pr\t")]
    assert lines == [eo.pr_line(len(FRAMES), tp, fp, positives, t)]
    assert res.stderr.splitlines()[-1] == lines[0] and "frames\t%d\t" % len(FRAMES) in res.stderr
    rows = [l.split("\t") for l in open(out).read().splitlines()]
    assert rows[0] == ["threshold", "tp", "fp", "precision", "recall"]
    assert [[int(v) for v in r[:3]] for r in rows[1:]] == [list(v) for v in zip(t.tolist(), tp.tolist(), fp.tolist())]
    plain = run_cli(*base)                                                       # without the flag: the same stdout, no pr line
    assert plain.returncode == 0 and plain.stdout == res.stdout and "pr\t" not in plain.stderr
