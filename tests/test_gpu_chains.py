"""GPU chains of the sequence searches (dlc_sequence_elastic_chains / dlc_sequence_chains, Engine.sequence_elastic_chains /
sequence_chains, deeploopcloser_amd.sequence.sequence_chains and chains=True on sequence_topk, sequence_peaks, the three
detectors and the CLI) against the NumPy restatement (tests/chains_oracle.py) and against the searches themselves.  Every
comparison is exact: columns and slopes by value, cells by bit pattern, NaN slots by position."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import chains_oracle as ch
import contrast_oracle as cn
import elastic_oracle as eo
import peaks_oracle as po
import sequence_oracle as so

pytestmark = pytest.mark.gpu

MAX_K = 128
SENTINEL = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A
# eight numbers, sums of which are exact in fp64 in any order: ties between steps and between chains at every level
EIGHT_F = np.array([-2.0, -0.5, -0.0, 0.0, 0.25, 1.0, 1.5, 3.0])
EIGHT_I = np.array([-3, -2, -1, 0, 1, 2, 3, 5], dtype=np.int64)
N_COLS = 650                                                          # past the widest trapezoid, (64 - 1) * 8 + 1 = 505


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def data(rng, dtype, rows, n):
    if dtype == "i64":
        return EIGHT_I[rng.randint(0, 8, size=(rows, n))]
    m = EIGHT_F[rng.randint(0, 8, size=(rows, n))]
    return m.astype(np.float32) if dtype == "f32" else m


def winning(m, lower):
    if m.dtype == np.int64:
        return -(1 << 40) if lower else (1 << 40)
    return -1e30 if lower else 1e30


def padded(dlc, m, ld, fill):
    """m [rows, n] on the device inside a [rows, ld] buffer whose other columns hold a value that would win if it were read."""
    e = dlc.default_engine()
    buf = torch.full((m.shape[0], ld), fill, dtype=torch.from_numpy(m[:1, :1]).dtype, device=e.device)
    buf[:, :m.shape[1]] = torch.from_numpy(m).to(e.device)
    return buf


def beyond_limits_win(m, limit0, step, lower):
    """(in place) every cell at or past its row's limit holds a value that would win if it were read."""
    rows, n = m.shape
    lim = so.limits(rows, n, n if limit0 is None else limit0, step)
    m[np.arange(n)[None, :] >= lim[:, None]] = winning(m, lower)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def placed_columns(rows, row0, n, L, d_max, limit0, step):
    """int64 [rows - row0, 12]: candidate ends at 0, inside and just below (L-1) * d_max (the trapezoid is cut by column 0),
    at n - 1, at the row's limit - 1 (cut by the limits of the rows behind), AT the limit, and what is no column: -1, n,
    another negative, 2^40."""
    lim = so.limits(rows, n, n if limit0 is None else limit0, step)[row0:]
    halo = (L - 1) * d_max
    fixed = [0, 3, max(halo - 1, 0) % n, (halo // 2) % n, min(halo, n - 1), n - 1, -1, n, -7, 1 << 40]
    cols = np.empty((rows - row0, len(fixed) + 2), np.int64)
    cols[:, :len(fixed)] = fixed
    cols[:, -2], cols[:, -1] = lim - 1, lim
    return cols


def check_elastic(dlc, m, L, steps, row0=0, limit0=None, step=0, lower=False, k=5, pad=7):
    """The chains of m's k best cells per row (the search's own idx) and of placed_columns against the oracle, and against
    the search itself: the cells summed oldest first are its scores bit for bit, chain[0] == idx - span.  The buffer's
    padding holds values that would win.  Returns (chain, cells) of the search's candidates, NumPy."""
    e = dlc.default_engine()
    rows, n = m.shape
    buf = padded(dlc, m, n + pad, winning(m, lower))
    kw = dict(row0=row0, n=n, limit0=limit0, limit_step=step, lower_is_better=lower)
    s, i, span, _ = e.sequence_elastic_topk(buf, L, steps, k=k, **kw)
    idx = torch.cat([i, torch.from_numpy(placed_columns(rows, row0, n, L, steps[1], limit0, step)).to(e.device)], 1)
    chain, cells = e.sequence_elastic_chains(buf, L, steps, idx, cells=True, **kw)
    assert chain.dtype == torch.int32 and tuple(chain.shape) == (rows - row0, idx.shape[1], L) and cells.shape == chain.shape
    only, none = e.sequence_elastic_chains(buf, L, steps, idx, **kw)
    assert none is None and torch.equal(only, chain)
    chain, cells, s, i, span = (t.cpu().numpy() for t in (chain, cells, s, i, span))
    want, want_cells = ch.elastic_chains(m, idx.cpu().numpy(), L, steps[0], steps[1], n, limit0, step, lower, row0)
    assert np.array_equal(chain, want), "chains"
    assert cells.dtype == want_cells.dtype and so.same_bits(cells, want_cells), "cells"
    # no oracle: the search's own lists
    got = i >= 0
    assert np.array_equal(chain[:, :k, L - 1], i) and np.array_equal(chain[:, :k, 0], np.where(got, i - span, -1))
    assert np.array_equal(bits(ch.sum_oldest_first(cells[:, :k]))[got], bits(s)[got]), "the cells do not sum to the score"
    return chain[:, :k], cells[:, :k]


SHAPES = [(1, (0, 0)), (5, (1, 1)), (12, (0, 8)), (64, (0, 8)), (64, (8, 8)), (10, (0, 2)), (7, (2, 5))]


@pytest.mark.parametrize("L,steps", SHAPES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32", "i64"])
def test_elastic_sweep(dlc, dtype, lower, L, steps):
    """Every dtype in both orders at a trapezoid of one column (L = 1; steps (1, 1)), of 89 (more than one 64-lane chunk)
    and of 505 columns (the maximum), and at the largest fixed step; the whole matrix, the detectors' limits (limit_step 1
    from a negative limit0: the limits of the rows behind cut the trapezoid) behind context rows (row0 > 0), and limits
    that grow by 3; rows with r < L - 1 are among the output rows of the first and the last."""
    rng = np.random.RandomState(L * 100 + steps[0] * 10 + steps[1] + lower)
    rows = L + 6
    valid = 0
    for limit0, step, row0 in ((None, 0, 0), (-2, 1, L + 1), (N_COLS - 45, 3, max(L - 3, 0))):
        m = data(rng, dtype, rows, N_COLS)
        beyond_limits_win(m, limit0, step, lower)
        chain, _ = check_elastic(dlc, m, L, steps, row0, limit0, step, lower)
        valid += int((chain >= 0).sum())
        if row0 < L - 1:
            assert (chain[:L - 1 - row0] == -1).all()
    assert valid > 0


def test_ties_take_the_lowest_step(dlc):
    for dtype, val in ((np.int64, 3), (np.float64, 2.5), (np.float32, 2.5)):
        same = np.full((12, 300), val, dtype)
        for steps in ((0, 2), (1, 3), (8, 8), (0, 8)):
            for lower in (False, True):
                L = 6
                chain, cells = check_elastic(dlc, same, L, steps, 3, lower=lower, k=20)
                j = np.arange((L - 1) * steps[0], (L - 1) * steps[0] + 20)           # ties -> the lower column, too
                want = j[:, None] - (L - 1 - np.arange(L))[None, :] * steps[0]
                assert all(np.array_equal(c, want) for c in chain[2:]) and (chain[:2] == -1).all()
    zeros = np.zeros((5, 300))
    zeros[:, ::2] = -0.0                                               # -0.0 ranks below +0.0
    for lower in (False, True):
        check_elastic(dlc, zeros, 3, (0, 1), lower=lower, k=20)
        check_elastic(dlc, zeros.astype(np.float32), 4, (0, 3), lower=lower, k=20)


def test_non_finite_entries(dlc):
    rng = np.random.RandomState(8)
    for dtype in (np.float64, np.float32):
        m = rng.standard_normal((40, N_COLS)).astype(dtype)            # inexact sums: the order of the additions shows
        m[rng.rand(40, N_COLS) < 0.02] = np.nan
        m[rng.rand(40, N_COLS) < 0.02] = np.inf
        m[rng.rand(40, N_COLS) < 0.02] = -np.inf                       # +inf and -inf in one window: the recursion decides
        m[rng.rand(40, N_COLS) < 0.02] = 0.0
        m[rng.rand(40, N_COLS) < 0.02] = -0.0
        m[7] = np.nan
        m[20] = np.inf
        m[21, ::3] = -np.inf
        for lower in (False, True):
            chain, cells = check_elastic(dlc, m, 5, (0, 2), 4, None, 0, lower, k=20)
            check_elastic(dlc, m, 2, (1, 3), 1, 600, 1, lower, k=MAX_K - 12)   # (idx: k + the 12 placed columns)
            check_elastic(dlc, m, 1, (0, 8), 0, 600, 1, lower, k=20)
        assert (chain[7 - 4:7 + 1] == -1).all() and np.isnan(cells[7 - 4:7 + 1]).all()   # every chain through row 7 is NaN


def test_poison_word(dlc):
    e = dlc.default_engine()
    m = torch.randn((20, 300), dtype=torch.float64, device=e.device)
    word = torch.zeros(1, dtype=torch.int64, device=e.device)
    off = dlc.slope_offsets(3)
    _, i, _, _ = e.sequence_elastic_topk(m, 3, (0, 2), k=7)
    _, li, _, _ = e.sequence_topk(m, 3, off, k=7)
    clean = e.sequence_elastic_chains(m, 3, (0, 2), i, cells=True) + e.sequence_chains(m, 3, off, li, cells=True)
    same = e.sequence_elastic_chains(m, 3, (0, 2), i, cells=True, poison=word) + e.sequence_chains(m, 3, off, li, cells=True, poison=word)
    assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b) for a, b in zip(clean, same))
    assert bool((clean[0][2:] >= 0).all()) and bool((clean[2][2:] >= 0).all())
    for scores in (m, m.float()):
        c, x = e.sequence_elastic_chains(scores, 3, (0, 2), i, cells=True, poison=word + 5)
        assert bool((c == -1).all()) and bool(x.isnan().all())
        c, x, v = e.sequence_chains(scores, 3, off, li, cells=True, poison=word + 1)
        assert bool((c == -1).all()) and bool(x.isnan().all()) and bool((v == -1).all())
    with pytest.raises(ValueError):
        e.sequence_elastic_chains(m.long(), 3, (0, 2), i, poison=word)
    with pytest.raises(ValueError):
        e.sequence_chains(m.long(), 3, off, li, poison=word)


# ---- the lines ----------------------------------------------------------------------------------------------------------
def check_lines(dlc, m, L, off, row0=0, limit0=None, step=0, lower=False, k=5, pad=7):
    """As check_elastic for dlc_sequence_chains: the oracle, then the search itself -- the cells summed NEWEST first are its
    scores bit for bit, the slope is its slope."""
    e = dlc.default_engine()
    rows, n = m.shape
    buf = padded(dlc, m, n + pad, winning(m, lower))
    kw = dict(row0=row0, n=n, limit0=limit0, limit_step=step, lower_is_better=lower)
    s, i, slope, _ = e.sequence_topk(buf, L, off, k=k, **kw)
    idx = torch.cat([i, torch.from_numpy(placed_columns(rows, row0, n, L, int(np.max(off)) // max(L - 1, 1), limit0, step)).to(e.device)], 1)
    chain, cells, v = e.sequence_chains(buf, L, off, idx, cells=True, **kw)
    only, none, v2 = e.sequence_chains(buf, L, off, idx, **kw)
    assert none is None and torch.equal(only, chain) and torch.equal(v, v2) and v.dtype == torch.int32
    chain, cells, v, s, i, slope = (t.cpu().numpy() for t in (chain, cells, v, s, i, slope))
    want, want_cells, want_v = ch.line_chains(m, idx.cpu().numpy(), L, off, n, limit0, step, lower, row0)
    assert np.array_equal(chain, want) and np.array_equal(v, want_v), "chains"
    assert cells.dtype == want_cells.dtype and so.same_bits(cells, want_cells), "cells"
    got = i >= 0
    assert np.array_equal(v[:, :k], slope) and np.array_equal(chain[:, :k, L - 1], i)
    assert np.array_equal(bits(ch.sum_newest_first(cells[:, :k]))[got], bits(s)[got]), "the cells do not sum to the score"
    return chain[:, :k]


@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32", "i64"])
def test_lines_sweep(dlc, dtype, lower):
    rng = np.random.RandomState(50 + lower)
    valid = 0
    tables = [(1, np.zeros((1, 1), np.int32)), (5, dlc.slope_offsets(5)), (10, dlc.slope_offsets(10, 0.0, 1.5, 0.1)),
              (64, dlc.slope_offsets(64)), (64, dlc.slope_offsets(64, 0.0, 8.0, 8.0 / 15))]
    assert tables[2][1].shape[0] == 16 and tables[4][1].shape[0] == 16 and tables[4][1].max() == 504
    for L, off in tables:
        rows = L + 6
        for limit0, step, row0 in ((None, 0, 0), (-2, 1, L + 1), (N_COLS - 45, 3, max(L - 3, 0))):
            if dtype == "i64":
                m = data(rng, dtype, rows, N_COLS)                     # ties between slopes: the lowest wins
            else:
                m = rng.standard_normal((rows, N_COLS)).astype(np.float32 if dtype == "f32" else np.float64)
                m[rng.rand(rows, N_COLS) < 0.01] = np.nan
                m[rng.rand(rows, N_COLS) < 0.01] = np.inf
            beyond_limits_win(m, limit0, step, lower)
            valid += int((check_lines(dlc, m, L, off, row0, limit0, step, lower) >= 0).sum())
    assert valid > 0
    same = np.full((9, 100), 2, np.int64) if dtype == "i64" else np.full((9, 100), 0.5, np.float32 if dtype == "f32" else np.float64)
    chain = check_lines(dlc, same, 6, dlc.slope_offsets(6), lower=lower, k=20)     # every slope ties: slope 0
    off = dlc.slope_offsets(6)[0]                                       # the first column its line fits into
    assert np.array_equal(chain[5, 0], off.max() - off[::-1])


# ---- independence of the batching ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,steps,lower", [("f64", (0, 2), False), ("i64", (1, 3), True), ("f32", None, True)])
def test_rows_split_over_batches(dlc, dtype, steps, lower):
    """A chain is a function of the L rows behind its cell: batches of 1, 7 and 32 rows, each with its L - 1 context rows in
    front (row0), give the chains of the whole matrix (steps None: the lines)."""
    e = dlc.default_engine()
    rng = np.random.RandomState(40)
    rows, n, L, k, limit0 = 75, 300, 10, 5, -4
    m = data(rng, dtype, rows, n)
    dev = torch.from_numpy(m).to(e.device)
    off = dlc.slope_offsets(L)
    if steps is None:
        _, idx, _, _ = e.sequence_topk(dev, L, off, k=k, limit0=limit0, limit_step=1, lower_is_better=lower)
        whole = e.sequence_chains(dev, L, off, idx, limit0=limit0, limit_step=1, lower_is_better=lower, cells=True)
    else:
        _, idx, _, _ = e.sequence_elastic_topk(dev, L, steps, k=k, limit0=limit0, limit_step=1, lower_is_better=lower)
        whole = e.sequence_elastic_chains(dev, L, steps, idx, limit0=limit0, limit_step=1, lower_is_better=lower, cells=True)
    assert bool((whole[0][40:] >= 0).all())
    for batch in (1, 7, 32):
        outs = []
        for lo in range(0, rows, batch):
            base = max(0, lo - (L - 1))
            kw = dict(row0=lo - base, limit0=limit0 + base, limit_step=1, lower_is_better=lower, cells=True)
            if steps is None:
                outs.append(e.sequence_chains(dev[base:lo + batch], L, off, idx[lo:lo + batch], **kw))
            else:
                outs.append(e.sequence_elastic_chains(dev[base:lo + batch], L, steps, idx[lo:lo + batch], **kw))
        for t, w in enumerate(whole):
            assert so.same_bits(torch.cat([o[t] for o in outs]).cpu().numpy(), w.cpu().numpy()), (batch, t)


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    m = torch.zeros((8, 50), dtype=torch.float64, device=e.device)
    idx = torch.full((8, 4), 5, dtype=torch.int64, device=e.device)
    o_c = torch.full((8, 4, 3), SENTINEL32, dtype=torch.int32, device=e.device)
    o_x = torch.full((8, 4, 3), SENTINEL, dtype=torch.int64, device=e.device)
    o_v = torch.full((8, 4), SENTINEL32, dtype=torch.int32, device=e.device)
    word = torch.zeros(1, dtype=torch.int64, device=e.device)
    off = (C.c_int32 * 6)(0, 1, 2, 0, 1, 1)
    src, di, dc, dx, dv, pw = (C.c_void_p(t.data_ptr()) for t in (m, idx, o_c, o_x, o_v, word))

    def reset():
        o_c.fill_(SENTINEL32), o_x.fill_(SENTINEL), o_v.fill_(SENTINEL32)

    def untouched():
        torch.cuda.synchronize()
        return bool((o_c == SENTINEL32).all()) and bool((o_x == SENTINEL).all()) and bool((o_v == SENTINEL32).all())

    common = {"dtype": dict(dtype=_lib.DLC_I8), "null scores": dict(scores=None), "null idx": dict(idx=None),
              "null out_chain": dict(chain=None), "rows 0": dict(rows=0), "row0 = rows": dict(row0=8), "row0 < 0": dict(row0=-1),
              "n 0": dict(n=0), "ld < n": dict(ld=49), "n 2^31": dict(n=1 << 31, ld=1 << 31), "L 0": dict(L=0), "L 65": dict(L=65),
              "k 0": dict(k=0), "k 129": dict(k=129), "poison with int64": dict(dtype=_lib.DLC_I64, poison=pw)}
    # a scores pointer off its element's alignment, inside a buffer a row larger than the call describes
    big = torch.zeros(9 * 50, dtype=torch.float64, device=e.device)
    assert big.data_ptr() % 8 == 0
    for name, dt, shift in (("f64", _lib.DLC_F64, 4), ("f32", _lib.DLC_F32, 2), ("i64", _lib.DLC_I64, 4)):
        common["misaligned scores " + name] = dict(dtype=dt, scores=C.c_void_p(big.data_ptr() + shift))
    # elastic
    names = ["ctx", "dtype", "scores", "rows", "row0", "n", "ld", "limit0", "step", "L", "d_min", "d_max", "lower", "k", "idx",
             "chain", "cells", "poison", "stream"]
    ok = (e.ctx, _lib.DLC_F64, src, 8, 0, 50, 50, 50, 0, 3, 0, 2, 0, 4, di, dc, dx, None, None)
    f = e.lib.dlc_sequence_elastic_chains
    assert len(ok) == len(names) and f(*ok) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert o_c[2:].unique().tolist() == [5] and o_c[:2].unique().tolist() == [-1] and bool((o_v == SENTINEL32).all())
    assert o_x[2:].unique().tolist() == [0] and bool(o_x[:2].view(torch.float64).isnan().all())

    def but(**change):
        return tuple(change.get(name, v) for name, v in zip(names, ok))

    reset()
    bad = dict(common, **{"d_min > d_max": dict(d_min=3), "d_min < 0": dict(d_min=-1), "d_max 9": dict(d_max=9)})
    for what, change in bad.items():
        assert f(*but(**change)) == _lib.DLC_ERR_BAD_ARG, what
        assert b"sequence_elastic_chains" in e.lib.dlc_last_error(e.ctx), what
    assert f(*but(ctx=None)) == _lib.DLC_ERR_BAD_ARG
    assert f(*but(rows=(1 << 31) // 4 + 1, row0=1)) == _lib.DLC_ERR_BAD_SHAPE
    assert f(*but(cells=None)) == _lib.DLC_OK and untouched_cells(o_x)
    reset()
    # lines
    names = names[:10] + ["n_slopes", "offsets"] + names[12:17] + ["slope"] + names[17:]
    ok = (e.ctx, _lib.DLC_F64, src, 8, 0, 50, 50, 50, 0, 3, 2, off, 0, 4, di, dc, dx, dv, None, None)
    f = e.lib.dlc_sequence_chains
    assert len(ok) == len(names) and f(*ok) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert o_c[2:, :].reshape(-1, 3).unique(dim=0).tolist() == [[3, 4, 5]] and o_c[:2].unique().tolist() == [-1]   # both lines tie
    assert o_v[2:].unique().tolist() == [0] and o_v[:2].unique().tolist() == [-1]
    reset()
    bad = dict(common, **{"null offsets": dict(offsets=None), "n_slopes 0": dict(n_slopes=0), "n_slopes 17": dict(n_slopes=17),
                          "offsets[0][0] != 0": dict(offsets=(C.c_int32 * 6)(1, 1, 2, 0, 1, 1)),
                          "offsets decrease": dict(offsets=(C.c_int32 * 6)(0, 2, 1, 0, 1, 1)),
                          "offsets past 32767": dict(offsets=(C.c_int32 * 6)(0, 1, 40000, 0, 1, 1))})
    for what, change in bad.items():
        assert f(*but(**change)) == _lib.DLC_ERR_BAD_ARG, what
        assert b"sequence_chains" in e.lib.dlc_last_error(e.ctx), what
    assert f(*but(ctx=None)) == _lib.DLC_ERR_BAD_ARG
    assert untouched(), "an error wrote"
    # the engine's and the module's own checks
    e.sequence_elastic_chains(m, 3, (0, 2), idx)
    for steps in ((3, 2), (-1, 2), (0, 9), (0,), 2, None):
        with pytest.raises(ValueError):
            e.sequence_elastic_chains(m, 3, steps, idx)
    for kw in (dict(row0=8), dict(row0=-1), dict(n=51), dict(n=0), dict(row0=1)):     # (row0 = 1: idx has a row too many)
        with pytest.raises(ValueError):
            e.sequence_elastic_chains(m, 3, (0, 2), idx, **kw)
        with pytest.raises(ValueError):
            e.sequence_chains(m, 3, [[0, 1, 2]], idx, **kw)
    for bad_idx in (idx.int(), idx.cpu(), idx[0], idx[:, :0], torch.zeros((8, MAX_K + 1), dtype=torch.int64, device=e.device)):
        with pytest.raises(ValueError):
            e.sequence_elastic_chains(m, 3, (0, 2), bad_idx)
        with pytest.raises(ValueError):
            e.sequence_chains(m, 3, [[0, 1, 2]], bad_idx)
    for table in ([[0, 1]], [0, 1, 2], [[0, 0.5, 1]]):
        with pytest.raises(ValueError):
            e.sequence_chains(m, 3, table, idx)
    with pytest.raises(ValueError):
        e.sequence_elastic_chains(m, 65, (0, 2), idx)
    with pytest.raises(ValueError):
        dlc.sequence_chains(m, idx, 3, offsets=[[0, 1, 2]], steps=(0, 2))


def untouched_cells(o_x):
    torch.cuda.synchronize()
    return bool((o_x == SENTINEL).all())


# ---- the module functions -----------------------------------------------------------------------------------------------
def test_module_functions_numpy_and_tensors(dlc):
    """deeploopcloser_amd.sequence: NumPy in -> NumPy out, tensors in -> tensors out; the chains are those of the matrix the
    search saw (contrast in front), of the picks (suppress behind); without chains=True every tuple is as it was."""
    rng = np.random.RandomState(10)
    e = dlc.default_engine()
    x = rng.randint(-128, 128, size=(60, 33)).astype(np.int8)
    dist = dlc.DistanceCalculator.distance_matrix(x)
    kw = dict(limit0=-3, limit_step=1, lower_is_better=True)
    L = 6
    for steps in ((0, 2), None):
        def oracle(m, idx):
            if steps is None:
                return ch.line_chains(m, idx, L, dlc.slope_offsets(L), **kw)[:2]
            return ch.elastic_chains(m, idx, L, steps[0], steps[1], **kw)

        plain = dlc.sequence_topk(dist, 3, L, steps=steps, **kw)
        s, i, v, chain = dlc.sequence_topk(dist, 3, L, steps=steps, chains=True, **kw)
        assert len(plain) == 3 and all(np.array_equal(a, b) for a, b in zip(plain, (s, i, v)))
        want, want_cells = oracle(dist, i)
        assert isinstance(chain, np.ndarray) and chain.dtype == np.int32 and np.array_equal(chain, want) and (chain[20:] >= 0).all()
        c2, cells = dlc.sequence_chains(dist, i, L, steps=steps, cells=True, **kw)
        assert np.array_equal(c2, want) and np.array_equal(cells, want_cells) and cells.dtype == np.int64
        assert np.array_equal(dlc.sequence_chains(dist, i, L, steps=steps, **kw), want)
        t = torch.from_numpy(dist).to(e.device)
        ts, ti, tv, tc = dlc.sequence_topk(t, 3, L, steps=steps, chains=True, **kw)
        assert isinstance(tc, torch.Tensor) and tc.device == e.device and tc.dtype == torch.int32 and np.array_equal(tc.cpu().numpy(), want)
        tc = dlc.sequence_chains(t, ti, L, steps=steps, **kw)
        assert isinstance(tc, torch.Tensor) and np.array_equal(tc.cpu().numpy(), want)
        # contrast in front
        normal = cn.contrast_rows(dist, 5, limit0=-3, limit_step=1)
        cs, ci, cv, cc = dlc.sequence_topk(dist, 3, L, steps=steps, contrast=5, chains=True, **kw)
        plain = dlc.sequence_topk(dist, 3, L, steps=steps, contrast=5, **kw)
        assert so.same_bits(cs, plain[0]) and np.array_equal(ci, plain[1]) and np.array_equal(cv, plain[2])
        want, want_cells = oracle(normal, ci)
        assert np.array_equal(cc, want) and (cc[20:] >= 0).all()
        c2, cells = dlc.sequence_chains(dist, ci, L, steps=steps, contrast=5, cells=True, **kw)
        assert np.array_equal(c2, want) and so.same_bits(cells, want_cells)
        # suppress behind, with and without contrast
        for contrast, m in ((None, dist), (5, normal)):
            plain = dlc.sequence_peaks(dist, 3, L, 4, steps=steps, contrast=contrast, **kw)
            ps, pi, pc = dlc.sequence_peaks(dist, 3, L, 4, steps=steps, contrast=contrast, chains=True, **kw)
            assert len(plain) == 2 and so.same_bits(ps, plain[0]) and np.array_equal(pi, plain[1])
            assert np.array_equal(pc, oracle(m, pi)[0]) and (pc[20:, 0] >= 0).all()
            assert (np.abs(pi[20:, 0] - pi[20:, 1]) > 4).all()


# ---- the detectors ------------------------------------------------------------------------------------------------------
L_SEQ, STEPS, K_DET, EXCLUSION = 4, (0, 2), 3, 10
MIXED = [1, 2, 9, 1, 40, 3]                                              # shorter and longer than the context
VARIANTS = [dict(steps=STEPS), dict(), dict(steps=STEPS, contrast=5, suppress=5), dict(contrast=5, suppress=5)]


def int8_scene(units):
    return po.two_place_scene(0, lambda rng, c: rng.randint(-128, 128, size=c).astype(np.int8), units)


def stream(det, x, batch):
    """What det returns for x's frames in batches of `batch` (a list: those sizes in turn, then the rest at once),
    concatenated, NumPy."""
    sizes = batch if isinstance(batch, list) else [batch] * (x.shape[0] // batch + 1)
    outs, f = [], 0
    for b in sizes + [x.shape[0]]:
        take = min(b, x.shape[0] - f)
        if take > 0:
            outs.append(det.query_and_insert(x[f:f + take]))
            f += take
    assert len(set(len(o) for o in outs)) == 1
    return tuple(torch.cat([o[t] for o in outs]).cpu().numpy() for t in range(len(outs[0])))


def detector_chains(dlc, make, x, rows, lower, batches=(1, 7, MIXED)):
    """Every variant of the search, batched unevenly, against ONE sequence_chains call over the detector's own raw rows
    `rows` as a matrix; without chains the detector returns what it returned before."""
    kw = dict(limit0=-EXCLUSION, limit_step=1, lower_is_better=lower)
    for variant in VARIANTS:
        plain = stream(make(sequence=L_SEQ, **variant), x, 32)
        assert len(plain) == 2
        search = {k: v for k, v in variant.items() if k != "suppress"}
        for batch in batches:
            s, i, chain = stream(make(sequence=L_SEQ, chains=True, **variant), x, batch)
            assert so.same_bits(s, plain[0]) and np.array_equal(i, plain[1]), (variant, batch)
            want = dlc.sequence_chains(rows, i, L_SEQ, **search, **kw)
            assert chain.dtype == np.int32 and np.array_equal(chain, want), (variant, batch)
            assert np.array_equal(chain[..., L_SEQ - 1], i) and (chain[L_SEQ + EXCLUSION:, 0] >= 0).all()
            assert (chain[:L_SEQ - 1 + EXCLUSION] == -1).all()
    with pytest.raises(ValueError):
        make(chains=True)


def test_cnn_vtl_detector(dlc):
    x = int8_scene(64)
    make = lambda **kw: dlc.CnnVtlLoopClosureDetector(64, k=K_DET, exclusion=EXCLUSION, capacity=64, **kw)
    detector_chains(dlc, make, x, dlc.DistanceCalculator.distance_matrix(x), True)
    det = make(sequence=L_SEQ, steps=STEPS, chains=True)
    s, i, chain = det.query_and_insert(x[:0])
    assert tuple(chain.shape) == (0, K_DET, L_SEQ) and chain.dtype == torch.int32
    s, i, chain = det.query_and_insert(x)
    plain, listed = det.loops(s, i, 0), det.loops(s, i, 0, chain)
    assert plain and len(plain) == len(listed) and all(len(p) == 3 and q[:3] == p for p, q in zip(plain, listed))
    for frame, match, _, pairs in listed:
        assert len(pairs) == L_SEQ and pairs[-1] == (frame, match) and [p[0] for p in pairs] == list(range(frame - L_SEQ + 1, frame + 1))
        assert all(0 <= b[1] - a[1] <= 2 and a[0] >= 0 for a, b in zip(pairs, pairs[1:]))


def test_cosine_detector(dlc):
    x = int8_scene(256).astype(np.float32)
    make = lambda **kw: dlc.LoopClosureDetector(256, k=K_DET, exclusion=EXCLUSION, capacity=16, **kw)
    det = make()
    det.query_and_insert(x)
    keys = det.db.score_keys(det.db.rows).cpu().numpy()                            # the detector's own raw rows: int64 keys
    detector_chains(dlc, make, x, keys, False)


def test_sdav_detector(dlc):
    e = dlc.default_engine()
    scene = po.two_place_scene(0, lambda rng, c: 1.0 / (1.0 + np.exp(-4.0 * rng.standard_normal((c, 250)))), 30)
    scene = np.clip(scene + 0.01 * np.random.RandomState(100).rand(*scene.shape), 0.001, 0.999)   # no two patches alike
    ds = torch.from_numpy(scene).to(e.device)
    make = lambda **kw: dlc.SdavLoopClosureDetector(ds, patches=30, width=250, k=K_DET, exclusion=EXCLUSION, capacity=8, **kw)
    sim = dlc.SimilarityCalculator(scene).similarity_matrix(as_int64=False)        # the detector's own raw rows
    detector_chains(dlc, make, ds, sim, False, batches=(7, MIXED))
    whole = stream(make(sequence=L_SEQ, steps=STEPS, chains=True), ds, 32)
    det, outs, tickets = make(sequence=L_SEQ, steps=STEPS, chains=True), [], []
    for lo in range(0, ds.shape[0], 16):                                           # two batches in flight
        tickets.append(det.submit(ds[lo:lo + 16]))
        if len(tickets) > 1:
            outs.append(det.result(tickets[-2]))
    outs.append(det.result(tickets[-1]))
    assert all(len(o) == 3 for o in outs)
    assert all(so.same_bits(torch.cat([o[t] for o in outs]).cpu().numpy(), whole[t]) for t in range(3))
    # a poisoned stream answers (NaN, -1) and no chain
    det = make(sequence=3, steps=(0, 1), chains=True)
    det.query_and_insert(ds[:20])
    bad = ds[20].clone()
    bad[1, 1] = 1.5
    s, i, chain = det.query_and_insert(bad)
    assert bool(s.isnan().all()) and bool((i == -1).all()) and bool((chain == -1).all()) and tuple(chain.shape) == (1, K_DET, 3)


def test_planted_revisit_chains_through_the_detector(dlc):
    """tests/test_chains_cpu.py's planted case through CnnVtlLoopClosureDetector(steps=(0, 2), chains=True): at each of the
    51 frames whose chain lies inside the revisit the top candidate's chain is the true correspondence, frame by frame."""
    x, true, alias, first = eo.planted_elastic_revisit()
    det = dlc.CnnVtlLoopClosureDetector(64, k=1, exclusion=30, capacity=512, sequence=10, steps=(0, 2), chains=True)
    s, i, chain = stream(det, x, 32)
    for f in range(9, 60):
        assert np.array_equal(chain[first + f, 0], true[f - 9:f + 1]), f


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_chains(dlc):
    common = ("--network", "sdav", "--metric", "similarity", "--exclusion", "2", "--k", "2", "--batch", "4")
    res = run_cli(*common, "--sequence", "3", "--steps", "0:2", "--chains")
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    loops = [n for n, l in enumerate(lines) if l.startswith("loop\t")]
    assert loops and len([l for l in lines if l.startswith("chain\t")]) == len(loops)
    for n in loops:
        loop, chain = lines[n].split("\t"), lines[n + 1].split("\t")
        assert chain[0] == "chain" and len(chain) == 1 + 3
        pairs = [tuple(int(v) for v in p.split(":")) for p in chain[1:]]
        frame, match = int(loop[1]), int(loop[3])
        assert pairs[-1] == (frame, match) and [p[0] for p in pairs] == [frame - 2, frame - 1, frame]
        assert all(0 <= b[1] - a[1] <= 2 for a, b in zip(pairs, pairs[1:])) and pairs[0][1] >= 0
    res = run_cli(*common, "--chains")
    assert res.returncode == 2 and "error:" in res.stderr and "--chains" in res.stderr
