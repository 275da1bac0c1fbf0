"""GPU windowed peak top-k of score rows (dlc_peak_topk_rows, Engine.peak_topk_rows, sequence.peak_topk / sequence_peaks /
uniqueness_ratio, suppress=W on the three detectors and on the CLI) against the NumPy restatement of the definition
(tests/peaks_oracle.py, pinned by test_peaks_cpu.py).  Every comparison is exact: indices equal, scores by bit pattern
(sequence_oracle.same_bits)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import peaks_oracle as po
import sequence_oracle as so

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
KINDS = ["f64", "f32", "i64"]
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097]
SEAMS = (63, 64, 255, 256, 257, 1023, 1024)                        # columns on either side of a chunk's edge
# the eight values a matrix is drawn from (mass ties), and the pair planted at the seams: above and below all eight
VALUES = {"f64": [-2.5, -0.0, 0.0, 1.0, 1.5, 3.25, -1e-300, 1e300],
          "f32": [-2.5, -0.0, 0.0, 1.0, 1.5, 3.25, -1e-30, 1e30],
          "i64": [-5, -1, 0, 3, 7, 1 << 40, -(1 << 50), 9]}
PEAKS = {"f64": (1e305, -1e305), "f32": (3e38, -3e38), "i64": (1 << 60, -(1 << 60))}
ABSENT = 3                                                          # (one of the eight: many cells are absent)


def pairs(n):
    """(suppress, k): every suppress and every k of the issue's lists, a dozen of their sixty combinations."""
    return [(0, 5), (0, 128), (1, 64), (1, 128), (5, 2), (5, 65), (63, 5), (64, 128), (255, 2), (256, 5), (300, 65), (n, 2),
            (1 << 40, 1), (1 << 40, 5)]


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def np_dtype(kind):
    return {"f64": np.float64, "f32": np.float32, "i64": np.int64}[kind]


def winner(kind, lower):
    """A value that beats every other: what the cells a call must not read are filled with."""
    if kind == "i64":
        return np.iinfo(np.int64).min if lower else np.iinfo(np.int64).max
    return -np.inf if lower else np.inf


def data(rng, kind, rows, n):
    """[rows, n] drawn from eight values, peaks planted on both sides of every chunk seam (the best value in even rows,
    the worst in odd ones, and the reverse two columns on), and for the float kinds one cell in sixteen a NaN and two
    cells a row an infinity."""
    m = np.asarray(VALUES[kind], np_dtype(kind))[rng.randint(0, 8, size=(rows, n))]
    hi, lo = PEAKS[kind]
    for c in SEAMS:
        if c < n:
            m[0::2, c], m[1::2, c] = hi, lo
        if c + 2 < n:
            m[0::2, c + 2], m[1::2, c + 2] = lo, hi
    if kind != "i64":
        m[rng.randint(0, 16, size=(rows, n)) == 0] = np.nan
        m[np.arange(rows), rng.randint(0, n, size=rows)] = np.inf
        m[np.arange(rows), rng.randint(0, n, size=rows)] = -np.inf
    return m


def on_device(e, m, ld, beyond):
    """m [rows, n] as the first n columns of a [rows, ld] device view whose rows start at an ODD element of their
    allocation; the other columns hold `beyond`."""
    rows, n = m.shape
    flat = torch.empty(rows * ld + 1, dtype=torch.from_numpy(m[:1, :1]).dtype, device=e.device)
    buf = flat[1:].view(rows, ld)
    buf.fill_(int(beyond) if flat.dtype == torch.int64 else float(beyond))
    buf[:, :n] = torch.from_numpy(m).to(e.device)
    return buf


def same(got, want):
    gs, gi = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    return gs.dtype == want[0].dtype and so.same_bits(gs, want[0]) and np.array_equal(gi, want[1])


def check(e, buf, m, k, suppress, **kw):
    """One call on the device view buf of m against the oracle on m."""
    got = e.peak_topk_rows(buf, k, suppress, n=m.shape[1], **kw)
    want = po.peak_topk_rows(m, k, suppress, **kw)
    assert same(got, want), (m.shape, k, suppress, kw)
    return got


# ---- P1: shapes, suppress, k, kinds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_against_the_definition(dlc, kind, n):
    e = dlc.default_engine()
    rng = np.random.RandomState(2000 + 31 * KINDS.index(kind) + n)
    for rows in (1, 5):
        m = data(rng, kind, rows, n)
        for lower in (False, True):
            buf = on_device(e, m, n + 5, winner(kind, lower))         # the tail columns would win
            for suppress, k in pairs(n):
                check(e, buf, m, k, suppress, lower_is_better=lower)
                if kind == "i64":
                    check(e, buf, m, k, suppress, lower_is_better=lower, absent=ABSENT)


@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_several_slabs(dlc, kind):
    """2 x 70 001: 274 chunks a row, shared out among several slabs of the chunk pass."""
    e = dlc.default_engine()
    m = data(np.random.RandomState(5), kind, 2, 70_001)
    buf = on_device(e, m, 70_001 + 3, winner(kind, False))
    absent = dict(absent=ABSENT) if kind == "i64" else {}
    for suppress, k in ((0, 128), (32, 5), (300, 128), (20_000, 5), (70_001, 3)):
        check(e, buf, m, k, suppress, **absent)
    check(e, on_device(e, m, 70_001, winner(kind, True)), m, 65, 5, lower_is_better=True, **absent)


def test_more_picks_asked_for_than_fit(dlc):
    """k > n / (W + 1): the all-equal row gives 0, W + 1, 2 (W + 1), ... and then empty slots."""
    e = dlc.default_engine()
    for n, w, k in ((300, 63, 8), (1023, 255, 5), (257, 256, 3), (700, 5, 128)):
        for value in (np.full((2, n), 3.0), np.full((2, n), -0.0), np.full((2, n), 7, np.int64)):
            s, i = check(e, torch.from_numpy(value).to(e.device), value, k, w)
            fit = min(k, (n + w) // (w + 1))
            assert i[0, :fit].tolist() == [t * (w + 1) for t in range(fit)] and bool((i[:, fit:] == -1).all())


def test_hand_worked_row(dlc):
    row = po.hand_worked_row()[None, :]
    s, i = dlc.peak_topk(row, 5, 0)
    assert i.tolist() == [[100, 99, 101, 98, 102]] and s.tolist() == [[10.0, 9.0, 9.0, 8.0, 8.0]]
    s, i = dlc.peak_topk(row, 4, 5)
    assert i.tolist() == [[100, 300, 94, 106]] and s.tolist() == [[10.0, 8.0, 4.0, 4.0]]
    s, i = dlc.peak_topk(po.hand_worked_row(reach_b=7)[None, :], 3, 6)
    assert i.tolist() == [[100, 300, 293]] and s.tolist() == [[10.0, 8.0, 1.0]]


# ---- P2: limits, and what is never read ----------------------------------------------------------------------------------
LIMITS = [(-4, 1), (0, 1), (120, 1), (7, 0), (136, -2), (20, -2)]


@pytest.mark.parametrize("limit0,step", LIMITS + [(-300, 150), (650, -90)])
def test_limits_and_what_is_never_read(dlc, limit0, step):
    e = dlc.default_engine()
    rows, n = (33, 130) if (limit0, step) in LIMITS else (7, 700)
    rng = np.random.RandomState(1000 + limit0)
    lim = so.limits(rows, n, limit0, step)
    past = np.arange(n)[None, :] >= lim[:, None]
    for kind in KINDS:
        m = data(rng, kind, rows, n)
        for lower in (False, True):
            filled = m.copy()
            filled[past] = winner(kind, lower)                        # cells at or past lim(r) would win, as the tail would
            buf = on_device(e, filled, n + 5, winner(kind, lower))
            for suppress, k in ((0, 5), (5, 3), (64, 128), (1 << 40, 2)):
                kw = dict(limit0=limit0, limit_step=step, lower_is_better=lower)
                if kind == "i64":
                    kw["absent"] = ABSENT
                s, i = check(e, buf, m, k, suppress, **kw)
                assert bool((i < torch.from_numpy(lim).to(e.device)[:, None]).all())


@pytest.mark.parametrize("limit0,step", [(0, 0), (-32, 1), (0, -1)])
def test_nothing_offered_gives_the_empty_lists(dlc, limit0, step):
    e = dlc.default_engine()
    for kind in KINDS:
        m = data(np.random.RandomState(3), kind, 33, 130)
        for lower in (False, True):
            s, i = check(e, on_device(e, m, 135, winner(kind, lower)), m, 4, 5, limit0=limit0, limit_step=step, lower_is_better=lower)
            assert bool((i == -1).all()) and bool((s == (-1 if kind == "i64" else (np.inf if lower else -np.inf))).all())


def test_row_strided_view(dlc):
    e = dlc.default_engine()
    whole = torch.randn((30, 700), dtype=torch.float64, device=e.device)
    view = whole[:, 100:500]
    want = po.peak_topk_rows(view.cpu().numpy(), 6, 20)
    assert same(e.peak_topk_rows(view, 6, 20), want) and same(dlc.peak_topk(view, 6, 20), want)
    whole[:, :100] = float("inf")                                    # what lies around the view changes nothing
    whole[:, 500:] = float("inf")
    assert same(e.peak_topk_rows(view, 6, 20), want)
    assert same(e.peak_topk_rows(whole, 6, 20, n=400), po.peak_topk_rows(whole.cpu().numpy(), 6, 20, n=400))


# ---- P3: what the header promises ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit0,step", [(1023, 0), (100, 7), (-2, 1)])
def test_suppress_zero_equals_topk_rows_f64(dlc, limit0, step):
    e = dlc.default_engine()
    m = data(np.random.RandomState(8), "f64", 5, 1023)
    buf = torch.from_numpy(m).to(e.device)
    for k in (1, 5, 128):
        ts, ti = e.topk_rows_f64(buf, limit0, step, k)
        ps, pi = e.peak_topk_rows(buf, k, 0, limit0=limit0, limit_step=step)
        assert torch.equal(ts.view(torch.int64), ps.view(torch.int64)) and torch.equal(ti, pi)


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_does_not_depend_on_its_batch(dlc, kind):
    e = dlc.default_engine()
    m = data(np.random.RandomState(60), kind, 33, 700)
    buf = on_device(e, m, 705, winner(kind, False))
    for suppress, k, limit0 in ((5, 7, 690), (300, 3, -3), (0, 128, 40)):
        whole = check(e, buf, m, k, suppress, limit0=limit0, limit_step=20)
        for size in (1, 5):
            parts = [e.peak_topk_rows(buf[lo:lo + size], k, suppress, n=700, limit0=limit0 + 20 * lo, limit_step=20)
                     for lo in range(0, 33, size)]
            assert same((torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])),
                        tuple(t.cpu().numpy() for t in whole)), (suppress, k, size)


def test_poison_word(dlc):
    e = dlc.default_engine()
    for kind in ("f64", "f32"):
        m = data(np.random.RandomState(21), kind, 5, 300)
        buf = torch.from_numpy(m).to(e.device)
        word = torch.zeros(1, dtype=torch.int64, device=e.device)
        assert same(e.peak_topk_rows(buf, 4, 5, poison=word), po.peak_topk_rows(m, 4, 5))
        word.fill_(7)
        s, i = e.peak_topk_rows(buf, 4, 5, poison=word)
        assert bool(s.isnan().all()) and bool((i == -1).all())
        s, i = e.peak_topk_rows(buf, 4, 5, limit0=0, poison=word)       # nothing offered, and still "these scores mean nothing"
        assert bool(s.isnan().all()) and bool((i == -1).all())
    with pytest.raises(ValueError):
        e.peak_topk_rows(torch.zeros((2, 9), dtype=torch.int64, device=e.device), 2, 1, poison=word)


def test_definition_checked_directly(dlc):
    """Without the oracle: the picks are pairwise more than W apart, and each is the best offered cell that is not
    within W of the picks before it."""
    e = dlc.default_engine()
    rng = np.random.RandomState(33)
    m = rng.standard_normal((4, 3000))
    m[rng.randint(0, 20, size=m.shape) == 0] = np.nan
    w, k, lim = 37, 30, 2900                                       # (30 windows of 75 columns do not cover 2900)
    s, i = (t.cpu().numpy() for t in e.peak_topk_rows(torch.from_numpy(m).to(e.device), k, w, limit0=lim))
    cols = np.arange(3000)
    for r in range(4):
        assert (i[r] >= 0).all() and (np.abs(i[r][:, None] - i[r][None, :])[~np.eye(k, dtype=bool)] > w).all()
        for t in range(k):
            free = (cols < lim) & ~np.isnan(m[r]) & (np.abs(cols[:, None] - i[r, :t][None, :]) > w).all(axis=1)
            best = np.nanmax(np.where(free, m[r], -np.inf))
            assert s[r, t] == best == m[r, i[r, t]] and i[r, t] == np.flatnonzero(free & (m[r] == best))[0]


# ---- P4: bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    m = torch.zeros((8, 50), dtype=torch.float64, device=e.device)
    o_s = torch.full((8, 4), SENTINEL, dtype=torch.int64, device=e.device)
    o_i = torch.full((8, 4), SENTINEL, dtype=torch.int64, device=e.device)
    word = torch.zeros(1, dtype=torch.int64, device=e.device)
    need = e.lib.dlc_peak_topk_rows_workspace_bytes(8, 50, 4)
    assert need == 256 and e.lib.dlc_peak_topk_rows_workspace_bytes(3, 70_001, 4) == (3 * 274 * 16 + 255) // 256 * 256
    for rows, n, k in ((0, 50, 4), (8, 0, 4), (8, 1 << 31, 4), (8, 50, 0), (8, 50, 129)):
        assert e.lib.dlc_peak_topk_rows_workspace_bytes(rows, n, k) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=e.device)
    src, ds, di, wp, pw = (C.c_void_p(t.data_ptr()) for t in (m, o_s, o_i, ws, word))
    f = e.lib.dlc_peak_topk_rows
    F64, I64 = _lib.DLC_F64, _lib.DLC_I64
    #      ctx    dtype scores rows n   ld  limit0 step lower suppress has_absent absent k  out_s out_i poison ws  bytes stream
    ok = (e.ctx, F64, src, 8, 50, 50, 50, 0, 0, 5, 0, 0, 4, ds, di, None, wp, need, None)
    assert f(*ok) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert o_i[:, 0].tolist() == [0] * 8 and o_s.view(torch.float64)[:, 3].tolist() == [0.0] * 8
    o_s.fill_(SENTINEL)
    o_i.fill_(SENTINEL)

    def but(**change):
        names = ["ctx", "dtype", "scores", "rows", "n", "ld", "limit0", "step", "lower", "suppress", "has_absent", "absent", "k",
                 "out_s", "out_i", "poison", "ws", "bytes", "stream"]
        return tuple(change.get(name, v) for name, v in zip(names, ok))

    bad = {"dtype": but(dtype=_lib.DLC_I8), "null scores": but(scores=None), "null out_scores": but(out_s=None),
           "null out_idx": but(out_i=None), "rows 0": but(rows=0), "n 0": but(n=0), "ld < n": but(ld=49),
           "suppress < 0": but(suppress=-1), "k 0": but(k=0), "k 129": but(k=129),
           "absent with fp64": but(has_absent=1, absent=-1), "absent with fp32": but(dtype=_lib.DLC_F32, has_absent=1),
           "poison with int64": but(dtype=I64, poison=pw), "misaligned scores": but(scores=C.c_void_p(m.data_ptr() + 4))}
    for what, args in bad.items():
        assert f(*args) == _lib.DLC_ERR_BAD_ARG, what
        assert b"peak_topk_rows" in e.lib.dlc_last_error(e.ctx), what
    assert f(*but(ctx=None)) == _lib.DLC_ERR_BAD_ARG
    assert f(*but(n=1 << 31, ld=1 << 31)) == _lib.DLC_ERR_BAD_SHAPE
    for args in (but(ws=None), but(bytes=need - 1)):
        assert f(*args) == _lib.DLC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((o_s == SENTINEL).all()) and bool((o_i == SENTINEL).all()), "an error wrote to the outputs"
    # the engine's own checks
    for kw in (dict(k=0, suppress=1), dict(k=129, suppress=1), dict(k=2, suppress=-1), dict(k=2, suppress=1, n=51),
               dict(k=2, suppress=1, n=0), dict(k=2, suppress=1, absent=-1)):
        with pytest.raises(ValueError):
            e.peak_topk_rows(m, **kw)
    for scores in (m.to(torch.float16), m.cpu(), m[0]):
        with pytest.raises(ValueError):
            e.peak_topk_rows(scores, 2, 1)


# ---- P5: the detectors ---------------------------------------------------------------------------------------------------
L_SEQ, W_SUP, K_DET, EXCLUSION = 4, 5, 3, 10
REVISITS = [(t, 20 + t - 90, 55 + t - 90) for t in range(96, 120)]      # (frame, the place it revisits strongly, weakly)


def int8_scene(units):
    return po.two_place_scene(0, lambda rng, c: rng.randint(-128, 128, size=c).astype(np.int8), units)


def stream(det, x, batch):
    outs = [det.query_and_insert(x[lo:lo + batch]) for lo in range(0, x.shape[0], batch)]
    return torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy()


def same_lists(results, es, ei):
    for s, i in results:
        assert s.dtype == es.dtype and np.array_equal(i, ei) and so.same_bits(s, es)


def both_places_only_with_suppress(with_w, plain):
    for t, a, b in REVISITS:
        assert a in with_w[t] and b in with_w[t], (t, with_w[t])
        assert a in plain[t] and b not in plain[t], (t, plain[t])


def test_cnn_vtl_detector(dlc):
    x = int8_scene(64)

    def make(**kw):
        return dlc.CnnVtlLoopClosureDetector(64, k=K_DET, exclusion=EXCLUSION, capacity=64, **kw)

    results = [stream(make(sequence=L_SEQ, suppress=W_SUP), x, batch) for batch in (1, 7, 32)]
    d = dlc.DistanceCalculator.distance_matrix(x)                                  # the detector's own raw rows, as a matrix
    kw = dict(limit0=-EXCLUSION, limit_step=1, lower_is_better=True)
    dense = dlc.sequence_scores(d, L_SEQ, **kw)
    es, ei = po.peak_topk_rows(dense, K_DET, W_SUP, absent=-1, **kw)
    assert es.dtype == np.int64
    same_lists(results, es, ei)
    assert same(dlc.sequence_peaks(d, K_DET, L_SEQ, W_SUP, **kw), (es, ei))
    both_places_only_with_suppress(ei, stream(make(sequence=L_SEQ), x, 32)[1])
    assert (ei[:L_SEQ - 1 + EXCLUSION] == -1).all() and (es[:L_SEQ - 1 + EXCLUSION] == -1).all()
    # sequence = 1: the frame distances themselves; contrast in front of it: fp64 lists
    same_lists([stream(make(sequence=1, suppress=W_SUP), x, 7)], *po.peak_topk_rows(d, K_DET, W_SUP, **kw))
    cs, ci = dlc.sequence_peaks(d, K_DET, L_SEQ, W_SUP, contrast=5, **kw)
    assert cs.dtype == np.float64
    same_lists([stream(make(sequence=L_SEQ, contrast=5, suppress=W_SUP), x, 7)], cs, ci)
    u = dlc.uniqueness_ratio(es)
    assert u.dtype == np.float64 and np.isnan(u[:L_SEQ - 1 + EXCLUSION + W_SUP]).all() and (u[96:] < 1.0).all()
    for kw in (dict(suppress=W_SUP), dict(sequence=L_SEQ, suppress=-1)):
        with pytest.raises(ValueError):
            make(**kw)
    # suppress=None is the detector as it was
    a, b = stream(make(sequence=L_SEQ, suppress=None), x, 32), stream(make(sequence=L_SEQ), x, 7)
    assert a[0].dtype == np.int64 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_cosine_detector(dlc):
    x = int8_scene(256).astype(np.float32)

    def make(**kw):
        return dlc.LoopClosureDetector(256, k=K_DET, exclusion=EXCLUSION, capacity=16, **kw)

    results = []
    for batch in (1, 7, 32):
        det = make(sequence=L_SEQ, suppress=W_SUP)
        results.append(stream(det, x, batch))
    keys = det.db.score_keys(det.db.rows)                                          # the detector's own raw rows: int64 keys
    kw = dict(limit0=-EXCLUSION, limit_step=1)
    dense = dlc.sequence_scores(keys, L_SEQ, **kw).cpu().numpy()
    ks, ei = po.peak_topk_rows(dense, K_DET, W_SUP, absent=-1, **kw)
    es = np.where(ei >= 0, ks.astype(np.float64) * 2.0 ** -40, -np.inf)            # key sums -> scores, as the detector does
    same_lists(results, es, ei)
    both_places_only_with_suppress(ei, stream(make(sequence=L_SEQ), x, 32)[1])
    with pytest.raises(ValueError):
        make(suppress=W_SUP)
    a, b = stream(make(sequence=L_SEQ, suppress=None), x, 32), stream(make(sequence=L_SEQ), x, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sdav_detector(dlc):
    e = dlc.default_engine()
    scene = po.two_place_scene(0, lambda rng, c: 1.0 / (1.0 + np.exp(-4.0 * rng.standard_normal((c, 250)))), 30)
    scene = np.clip(scene + 0.01 * np.random.RandomState(100).rand(*scene.shape), 0.001, 0.999)   # no two patches alike
    ds = torch.from_numpy(scene).to(e.device)
    n = ds.shape[0]

    def make(**kw):
        return dlc.SdavLoopClosureDetector(ds, patches=30, width=250, k=K_DET, exclusion=EXCLUSION, capacity=8, **kw)

    results = [stream(make(sequence=L_SEQ, suppress=W_SUP), ds, batch) for batch in (1, 7, 32)]
    sim = dlc.SimilarityCalculator(scene).similarity_matrix(as_int64=False)        # the detector's own raw rows
    kw = dict(limit0=-EXCLUSION, limit_step=1)
    es, ei = po.peak_topk_rows(dlc.sequence_scores(sim, L_SEQ, **kw), K_DET, W_SUP, **kw)
    same_lists(results, es, ei)
    both_places_only_with_suppress(ei, stream(make(sequence=L_SEQ), ds, 32)[1])
    assert (ei[:L_SEQ - 1 + EXCLUSION] == -1).all() and np.isneginf(es[:L_SEQ - 1 + EXCLUSION]).all()
    det, outs, tickets = make(sequence=L_SEQ, suppress=W_SUP), [], []
    for lo in range(0, n, 16):                                                     # two batches in flight
        tickets.append(det.submit(ds[lo:lo + 16]))
        if len(tickets) > 1:
            outs.append(det.result(tickets[-2]))
    outs.append(det.result(tickets[-1]))
    same_lists([(torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy())], es, ei)
    with pytest.raises(ValueError):
        make(suppress=W_SUP)
    a, b = stream(make(sequence=L_SEQ, suppress=None), ds, 32), stream(make(sequence=L_SEQ), ds, 7)
    assert so.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a poisoned stream still answers (NaN, -1)
    det = make(sequence=3, suppress=2)
    det.query_and_insert(ds[:20])
    bad = ds[20].clone()
    bad[1, 1] = 1.5
    s, i = det.query_and_insert(bad)
    assert bool(s.isnan().all()) and bool((i == -1).all())


# ---- P6: the module's surface ----------------------------------------------------------------------------------------------
def test_module_functions_numpy_and_tensors(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(12)
    for kind in KINDS:
        m = data(rng, kind, 40, 300)
        absent = dict(absent=ABSENT) if kind == "i64" else {}
        for lower in (False, True):
            kw = dict(limit0=-3, limit_step=9, lower_is_better=lower, **absent)
            want = po.peak_topk_rows(m, 4, 6, **kw)
            got = dlc.peak_topk(m, 4, 6, **kw)
            assert all(isinstance(t, np.ndarray) for t in got) and same(got, want)
            got = dlc.peak_topk(torch.from_numpy(m).to(e.device), 4, 6, **kw)
            assert all(isinstance(t, torch.Tensor) and t.device == e.device for t in got) and same(got, want)
    for m in (rng.standard_normal((40, 70)), rng.randint(0, 4097, size=(40, 70)).astype(np.int64)):
        for lower in (False, True):
            kw = dict(limit0=-3, limit_step=1, lower_is_better=lower)
            dense = so.sequence_scores(m, 5, dlc.slope_offsets(5), **kw)[0]
            want = po.peak_topk_rows(dense, 3, 4, absent=-1 if m.dtype == np.int64 else None, **kw)
            got = dlc.sequence_peaks(m, 3, 5, 4, **kw)
            assert all(isinstance(t, np.ndarray) for t in got) and same(got, want)
            got = dlc.sequence_peaks(torch.from_numpy(m).to(e.device), 3, 5, 4, **kw)
            assert all(isinstance(t, torch.Tensor) for t in got) and same(got, want)
            plain = dlc.sequence_topk(m, 3, 5, **kw)                                 # suppress = 0: the sequence search's own lists
            assert same(dlc.sequence_peaks(m, 3, 5, 0, **kw), plain[:2])
    s, i = dlc.peak_topk(np.zeros((0, 5)), 2, 1)
    assert s.shape == (0, 2) and i.shape == (0, 2)
    s, i = dlc.peak_topk(np.zeros((3, 0), np.int64), 2, 1)
    assert (s == -1).all() and (i == -1).all() and s.shape == (3, 2)
    for name in ("peak_topk", "sequence_peaks", "uniqueness_ratio"):
        assert getattr(dlc.sequence, name) is getattr(dlc, name) and name in dlc.__all__
    with pytest.raises(ValueError):
        dlc.peak_topk(m, 0, 1)
    with pytest.raises(ValueError):
        dlc.peak_topk(m, 2, -1)


def test_uniqueness_ratio(dlc):
    e = dlc.default_engine()
    d = np.random.RandomState(2).randint(1, 4097, size=(20, 90)).astype(np.int64)
    s, i = dlc.peak_topk(d, 2, 5, limit0=-2, limit_step=1, lower_is_better=True)
    u = dlc.uniqueness_ratio(s)
    filled = i[:, 1] >= 0
    assert isinstance(u, np.ndarray) and u.dtype == np.float64 and np.isnan(u[~filled]).all()
    assert not filled[:9].any() and filled[14:].all()                 # row r offers r - 2 cells; a window covers up to 11
    assert np.array_equal(u[filled], s[filled, 0].astype(np.float64) / s[filled, 1].astype(np.float64)) and (u[filled] <= 1.0).all()
    # OpenSeqSLAM's quotient, written out for one row
    row = d[19, :17]
    at = int(np.argmin(row))
    outside = np.abs(np.arange(17) - at) > 5
    assert u[19] == row.min() / row[outside].min()
    t = dlc.uniqueness_ratio(torch.from_numpy(s).to(e.device))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == e.device and so.same_bits(t.cpu().numpy(), u)
    fp = np.where(s >= 0, s, np.inf).astype(np.float64)               # the fp64 lists' empty fill
    assert so.same_bits(dlc.uniqueness_ratio(fp), u)
    with pytest.raises(ValueError):
        dlc.uniqueness_ratio(s[:, :1])


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_suppress(dlc):
    res = run_cli("--network", "sdav", "--metric", "similarity", "--sequence", "3", "--suppress", "2", "--exclusion", "2", "--k", "2",
                  "--batch", "4")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    loops = [l.split("\t") for l in res.stdout.splitlines() if l.startswith("loop\t")]
    assert loops and all(len(l) == 6 and int(l[1]) - int(l[3]) > 2 for l in loops)                # the format, and old enough
    by_frame = {}
    for l in loops:
        by_frame.setdefault(int(l[1]), []).append(int(l[3]))
    assert any(len(v) == 2 for v in by_frame.values()) and all(len(v) == 1 or abs(v[0] - v[1]) > 2 for v in by_frame.values())
    for args in (("--network", "sdav", "--metric", "similarity", "--suppress", "2"),
                 ("--network", "sdav", "--metric", "similarity", "--sequence", "3", "--suppress", "-1")):
        res = run_cli(*args)
        assert res.returncode == 2 and "error:" in res.stderr and "usage:" in res.stderr
