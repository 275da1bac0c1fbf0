"""GPU elastic sequence search (dlc_sequence_elastic_topk, Engine.sequence_elastic_topk, steps= on deeploopcloser_amd.sequence
and on the three detectors, the CLI) against the NumPy restatement of the recursion (tests/elastic_oracle.py).  Every
comparison is exact: indices and spans by value, fp64 scores by bit pattern, NaN slots by position."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import contrast_oracle as co
import elastic_oracle as eo
import peaks_oracle as po
import sequence_oracle as so

pytestmark = pytest.mark.gpu

MAX_K = 128
SENTINEL = 0x5A5A5A5A5A5A5A5A
# eight numbers, sums of which are exact in fp64 in any order: ties between cells, between steps and between chains
EIGHT_F = np.array([-2.0, -0.5, -0.0, 0.0, 0.25, 1.0, 1.5, 3.0])
EIGHT_I = np.array([-3, -2, -1, 0, 1, 2, 3, 5], dtype=np.int64)
# the scan's plan (csrc/sequence_elastic.hip, restated by plan() below): 64-column chunks, four output rows per workgroup,
# tiles of 512 columns (1024 once the halo (L-1) * d_max passes 256), halved down to 128 -- not below the padded halo --
# while the call has fewer than 256 workgroups; slabs of whole tiles, at most 1024 workgroups
CHUNK, WAVES, TILE, WIDE_TILE, WIDE_HALO, MIN_TILE, WANT_WG, MAX_WG = 64, 4, 512, 1024, 256, 128, 256, 1024


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


def cdiv(a, b):
    return -(-a // b)


def plan(rows, row0, L, steps, cols):
    """(columns per tile, columns per slab) of the scan of a call whose output rows offer `cols` columns: el_plan and
    dlc::split_slabs as csrc/sequence_elastic.hip applies them."""
    halo = (L - 1) * steps[1]
    lead = cdiv(halo, CHUNK) * CHUNK
    ct = WIDE_TILE if halo > WIDE_HALO else TILE
    while ct > MIN_TILE and ct // 2 >= lead and cdiv(rows - row0, WAVES) * cdiv(cols, ct) < WANT_WG:
        ct //= 2
    col_tiles = cdiv(cols, ct)
    slabs = min(col_tiles, cdiv(MAX_WG, cdiv(rows, WAVES)))
    return ct, ct * cdiv(col_tiles, slabs)


def seams_of(rows, row0, n, L, steps, limit0, step):
    """(every column at which a tile -- and with it a slab -- of the plan begins, the first chunk seams, the tile widths in
    use), over the two calls check() makes: with the dense output the scan covers the n columns, without it the columns
    up to the largest limit of an output row, and the two may get different plans."""
    lim = so.limits(rows, n, n if limit0 is None else limit0, step)
    seams, tiles = set(c for c in (CHUNK, 2 * CHUNK, 3 * CHUNK, 4 * CHUNK) if c < n), set()
    for cols in (n, int(max(lim[row0], lim[rows - 1]))):
        if cols > 0:
            ct, slab = plan(rows, row0, L, steps, cols)
            assert slab % ct == 0                                  # a slab seam is a tile seam
            tiles.add(ct)
            seams.update(range(ct, cols, ct))
    return sorted(seams), tiles


def plant(m, r, j, steps, L, rng, lower):
    """A chain that beats everything drawn from the eight numbers: it ends in cell (r, j) and steps back a random
    d_min .. d_max columns per row.  Returns its span (None where it does not fit into the matrix)."""
    if r - (L - 1) < 0:
        return None
    cols = [j]
    for _ in range(L - 1):
        cols.append(cols[-1] - int(rng.randint(steps[0], steps[1] + 1)))
    if cols[-1] < 0 or j >= m.shape[1]:
        return None
    for s, c in enumerate(cols):
        m[r - s, c] = -50 if lower else 50
    return j - cols[-1]


def padded(dlc, m, ld, fill):
    """m [rows, n] on the device inside a [rows, ld] buffer whose other columns hold a value that would win if it were read."""
    e = dlc.default_engine()
    buf = torch.full((m.shape[0], ld), fill, dtype=torch.from_numpy(m[:1, :1]).dtype, device=e.device)
    buf[:, :m.shape[1]] = torch.from_numpy(m).to(e.device)
    return buf


def winning(m, lower):
    if m.dtype == np.int64:
        return -(1 << 40) if lower else (1 << 40)
    return -1e30 if lower else 1e30


def check(dlc, m, L, steps, k, row0=0, limit0=None, step=0, lower=False, pad=5, only=None):
    """Lists, spans and the dense scores of m against the oracle; the buffer's padding, and (the caller's business) whatever
    lies past a row's limit, hold values that would win.  only: the rows of m to compare (a wave works a row out on its
    own and a cell depends on the L rows behind it alone; the call is made for all of them)."""
    e = dlc.default_engine()
    n = m.shape[1]
    buf = padded(dlc, m, n + pad, winning(m, lower))
    kw = dict(k=k, row0=row0, n=n, limit0=limit0, limit_step=step, lower_is_better=lower)
    s, i, v, d = e.sequence_elastic_topk(buf, L, steps, dense=True, **kw)
    sel = slice(None) if only is None else np.asarray(only) - row0
    ed, esp = eo.elastic_scores(m, L, steps[0], steps[1], n, limit0, step, lower, row0, only)
    es, ei, ev = eo.topk_of(ed[sel], esp[sel], k, lower)
    assert np.array_equal(i.cpu().numpy()[sel], ei), "indices"
    assert np.array_equal(v.cpu().numpy()[sel], ev), "spans"
    assert so.same_bits(s.cpu().numpy()[sel], es), "scores"
    assert so.same_bits(d.cpu().numpy()[sel], ed[sel]), "dense scores"
    # the lists alone (no dense output: the scan then stops at the columns the rows offer) are the same lists
    s2, i2, v2, d2 = e.sequence_elastic_topk(buf, L, steps, **kw)
    assert d2 is None and torch.equal(i2, i) and torch.equal(v2, v) and so.same_bits(s2.cpu().numpy(), s.cpu().numpy())
    return s, i, v


def beyond_limits_win(m, limit0, step, lower):
    """(in place) every cell at or past its row's limit holds a value that would win if it were read."""
    rows, n = m.shape
    lim = so.limits(rows, n, n if limit0 is None else limit0, step)
    m[np.arange(n)[None, :] >= lim[:, None]] = winning(m, lower)


# (dtype, L, steps, rows, row0, n, k, limit0, limit_step, lower).  Every dtype in both orders; n in 1, 63, 64, 65, 257, 300,
# 1031 and 70 001; L in 1, 2, 10, 64; steps (0,0), (0,2), (1,1), (1,3), (0,8), (8,8); k in 1, 5, 128; limit_step in
# -1, 0, 1, 3 with limit0 negative, zero, inside and past n; row0 > 0 -- each value at least twice.  L = 64 needs 64 rows
# before anything is offered, so those cases have 70 -- a call of two workgroups per tile, whose tile is halved to the
# padded halo's 512 columns; the case of 575 rows is large enough to keep the 1024-column tile (61.8 KB of LDS).
SWEEP = [
    ("f64", 1, (0, 0), 1, 0, 1, 1, None, 0, False),
    ("i64", 1, (0, 2), 7, 0, 63, 5, 0, 3, True),
    ("f32", 2, (0, 0), 2, 1, 1, 5, 1, 0, True),
    ("f64", 2, (1, 1), 9, 1, 64, MAX_K, 70, -1, False),
    ("i64", 2, (8, 8), 5, 0, 65, 1, -2, 3, False),
    ("f32", 2, (1, 3), 40, 0, 257, MAX_K, None, 0, False),
    ("f64", 10, (0, 2), 40, 9, 300, 5, -5, 1, True),
    ("i64", 10, (1, 1), 33, 0, 300, MAX_K, 310, -1, True),
    ("f32", 10, (1, 3), 25, 12, 1031, 5, 0, 0, False),                # limit 0: nothing is offered
    ("f64", 10, (0, 8), 40, 9, 1031, MAX_K, 990, 1, False),           # limits that grow past n
    ("i64", 10, (8, 8), 30, 9, 257, 5, None, 0, False),
    ("f32", 10, (0, 8), 12, 0, 63, 1, 60, 3, True),
    ("f64", 64, (0, 8), 70, 63, 1031, 5, None, 0, True),              # the halo of 504 columns: tiles of 512
    ("i64", 64, (0, 8), 575, 63, 1031, 5, None, 0, True),             # 128 workgroups per tile: tiles of 1024
    ("i64", 64, (0, 8), 70, 63, 1031, MAX_K, 900, 3, False),
    ("f32", 64, (1, 3), 70, 66, 300, 1, 150, 1, False),
    ("i64", 64, (0, 2), 70, 0, 65, 5, 66, -1, True),
    ("f64", 10, (0, 2), 12, 9, 70001, 5, 69990, 3, False),            # 274 slabs of one 256-column tile each
    ("i64", 1, (1, 3), 40, 3, 1031, MAX_K, -1, 1, False),
    ("f64", 2, (0, 0), 1, 0, 64, 1, None, 0, True),                   # rows = L - 1: nothing is offered
]


def planted_case(dtype, L, steps, rows, row0, n, limit0, step, lower, rng):
    """(matrix, the cells planted chains end in, the tile widths of the plan): values from the eight numbers, a best chain
    ending just left of, on, and half a halo right of EVERY tile seam (slab seams are among them) of both calls' plans and
    of the first chunk seams, dealt round the output rows; then winning values past every row's limit."""
    m = data(rng, dtype, rows, n)
    seams, tiles = seams_of(rows, row0, n, L, steps, limit0, step)
    out_rows = list(range(max(row0, L - 1), rows))
    planted = []
    for seam in seams:
        for j in (seam - 1, seam, seam + (L - 1) * steps[1] // 2):
            if out_rows:
                r = out_rows[-1 - len(planted) % len(out_rows)]
                if plant(m, r, j, steps, L, rng, lower) is not None:
                    planted.append((r, j))
    beyond_limits_win(m, limit0, step, lower)
    return m, planted, tiles


@pytest.mark.parametrize("dtype,L,steps,rows,row0,n,k,limit0,step,lower", SWEEP)
def test_sweep(dlc, dtype, L, steps, rows, row0, n, k, limit0, step, lower):
    rng = np.random.RandomState(L * 1000 + steps[0] * 100 + steps[1] * 10 + rows + n + k)
    m, planted, tiles = planted_case(dtype, L, steps, rows, row0, n, limit0, step, lower, rng)
    # many rows: the call is made for all of them, the rows chains were planted in and every 8th are compared
    only = None if rows - row0 <= 128 else sorted(set(r for r, _ in planted) | set(range(row0, rows, 8)))
    s, i, v = check(dlc, m, L, steps, k, row0, limit0, step, lower, only=only)
    assert planted or n < 2 * CHUNK or rows < L
    if L == 1:
        assert bool(((v == 0) | (i < 0)).all())


def test_sweep_meets_every_tile_width():
    """The plan as restated above: the sweep runs tiles of 128, 256, 512 and 1024 columns, and the 1024-column tile with
    the halo of L = 64, steps (0, 8) -- the largest LDS footprint -- is among them."""
    widths = {}
    for dtype, L, steps, rows, row0, n, k, limit0, step, lower in SWEEP:
        for ct in seams_of(rows, row0, n, L, steps, limit0, step)[1]:
            widths.setdefault(ct, set()).add((L, steps))
    assert sorted(widths) == [128, 256, 512, 1024] and (64, (0, 8)) in widths[1024] and (64, (0, 8)) in widths[512]


def test_ties_take_the_lowest_step_and_the_lower_column(dlc):
    for dtype, val in ((np.int64, 3), (np.float64, 2.5), (np.float32, 2.5)):
        same = np.full((12, 900), val, dtype)
        for steps in ((0, 2), (1, 3), (8, 8), (0, 8)):
            first = 3 * steps[0]
            s, i, v = check(dlc, same, 4, steps, 20, 3)
            assert (i.cpu().numpy() == np.arange(first, first + 20)).all() and bool((v == first).all()) and bool((s == 4 * val).all())
    zeros = np.zeros((3, 300))
    zeros[:, ::2] = -0.0                                               # -0.0 ranks below +0.0, as in dlc_topk_rows_f64
    check(dlc, zeros, 1, (0, 0), 20)
    check(dlc, zeros, 3, (0, 1), 20)
    check(dlc, zeros, 3, (0, 1), 20, lower=True)


def test_non_finite_entries(dlc):
    rng = np.random.RandomState(8)
    for dtype in (np.float64, np.float32):
        m = rng.standard_normal((40, 1031)).astype(dtype)
        m[rng.rand(40, 1031) < 0.02] = np.nan
        m[rng.rand(40, 1031) < 0.02] = np.inf
        m[rng.rand(40, 1031) < 0.02] = -np.inf                        # +inf and -inf in one window: the recursion decides
        m[rng.rand(40, 1031) < 0.02] = 0.0
        m[rng.rand(40, 1031) < 0.02] = -0.0
        m[7] = np.nan
        m[20] = np.inf
        m[21, ::3] = -np.inf
        for lower in (False, True):
            s, i, v = check(dlc, m, 5, (0, 2), 20, 4, None, 0, lower)
            check(dlc, m, 2, (1, 3), MAX_K, 1, 900, 1, lower)
            check(dlc, m, 1, (0, 8), MAX_K, 0, 900, 1, lower)
        assert not bool(s.isnan().any())
        assert bool((i[7 - 4:7 + 1] == -1).all())                     # every chain through row 7 is NaN


def test_poison_word(dlc):
    e = dlc.default_engine()
    m = torch.randn((20, 700), dtype=torch.float64, device=e.device)
    word = torch.zeros(1, dtype=torch.int64, device=e.device)

    def bits(t):
        return t.view(torch.int64) if t.dtype == torch.float64 else t

    clean = e.sequence_elastic_topk(m, 3, (0, 2), k=7, dense=True)
    same = e.sequence_elastic_topk(m, 3, (0, 2), k=7, dense=True, poison=word)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(clean, same))
    s, i, v, d = e.sequence_elastic_topk(m, 3, (0, 2), k=7, dense=True, poison=word + 5)
    assert bool(s.isnan().all()) and bool((i == -1).all()) and bool((v == -1).all()) and bool(d.isnan().all())
    s, i, v, d = e.sequence_elastic_topk(m.float(), 3, (0, 2), k=7, poison=word + 1)
    assert bool(s.isnan().all()) and bool((i == -1).all()) and bool((v == -1).all()) and d is None
    with pytest.raises(ValueError):
        e.sequence_elastic_topk(m.long(), 3, (0, 2), k=7, poison=word)


# ---- the stated consequences, on the device -----------------------------------------------------------------------------
def test_length_one_equals_topk_rows_f64(dlc):
    e = dlc.default_engine()
    g = torch.Generator(device=e.device)
    g.manual_seed(12)
    rows, ld, k = 37, 1500, 7
    sc = torch.randn((rows, ld), generator=g, device=e.device, dtype=torch.float64)
    sc[:, ::5] = sc[:, 1::5][:, :sc[:, ::5].shape[1]]
    sc[3, :] = 2.5
    sc[4, 10:900] = float("nan"); sc[5, :] = float("nan"); sc[6, 17] = float("inf"); sc[7, 3] = float("-inf")
    sc[8, ::2] = 0.0; sc[8, 1::2] = -0.0
    for limit0, step in ((ld, 0), (-3, 1), (4, 40), (0, 0), (ld + 9, -2)):
        for kk, steps in ((1, (0, 0)), (k, (0, 2)), (MAX_K, (8, 8))):
            ws, wi = e.topk_rows_f64(sc, limit0, step, kk)
            s, i, v, _ = e.sequence_elastic_topk(sc, 1, steps, k=kk, limit0=limit0, limit_step=step)
            assert torch.equal(i, wi) and torch.equal(s.view(torch.int64), ws.view(torch.int64)), (limit0, step, kk)
            assert torch.equal(v, torch.where(i >= 0, 0, -1).to(torch.int32))


@pytest.mark.parametrize("d", [0, 1, 2, 8])
def test_fixed_step_equals_the_linear_search_on_int64(dlc, d):
    e = dlc.default_engine()
    rng = np.random.RandomState(20 + d)
    L = 6
    m = torch.from_numpy(rng.randint(-1000, 1000, size=(40, 1031)).astype(np.int64)).to(e.device)
    line = np.array([[s * d for s in range(L)]], dtype=np.int32)
    for lower, limit0, step in ((False, None, 0), (True, -5, 3), (True, 1040, -1)):
        kw = dict(k=7, row0=2, limit0=limit0, limit_step=step, lower_is_better=lower, dense=True)
        s, i, v, dense = e.sequence_elastic_topk(m, L, (d, d), **kw)
        ls, li, _, ldense = e.sequence_topk(m, L, line, **kw)
        assert torch.equal(s, ls) and torch.equal(i, li) and torch.equal(dense, ldense)
        assert torch.equal(v, torch.where(li >= 0, (L - 1) * d, -1).to(torch.int32))


def test_dense_output_against_the_lists(dlc):
    """The lists are the k best cells of the dense output, and seq_out's columns n .. ld_out - 1 keep their bits (the
    raw entry point: the engine's own dense result has ld_out = n)."""
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    rng = np.random.RandomState(30)
    rows, n, ld_out, L, k = 23, 1031, 1040, 5, 9
    m = torch.from_numpy(data(rng, "f64", rows, n)).to(e.device)
    seq = torch.full((rows - 4, ld_out), SENTINEL, dtype=torch.int64, device=e.device)
    o_s = torch.empty((rows - 4, k), dtype=torch.float64, device=e.device)
    o_i = torch.empty((rows - 4, k), dtype=torch.int64, device=e.device)
    o_v = torch.empty((rows - 4, k), dtype=torch.int32, device=e.device)
    need = e.lib.dlc_sequence_elastic_topk_workspace_bytes(rows, n, L, 0, 2, k)
    ws = torch.empty(need, dtype=torch.uint8, device=e.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = e.lib.dlc_sequence_elastic_topk(e.ctx, _lib.DLC_F64, p(m), rows, 4, n, n, 1000, 1, L, 0, 2, 1, k, p(o_s), p(o_i), p(o_v),
                                         p(seq), ld_out, None, p(ws), need, None)
    assert rc == _lib.DLC_OK
    torch.cuda.synchronize()
    assert bool((seq[:, n:] == SENTINEL).all()), "seq_out past column n was written"
    dense = seq[:, :n].contiguous().view(torch.float64).cpu().numpy()
    ed, esp = eo.elastic_scores(m.cpu().numpy(), L, 0, 2, n, 1000, 1, True, 4)
    assert so.same_bits(dense, ed)
    ls, li, _ = eo.topk_of(dense, np.where(np.isnan(dense), -1, 0).astype(np.int32), k, True)
    assert np.array_equal(o_i.cpu().numpy(), li) and so.same_bits(o_s.cpu().numpy(), ls)
    assert np.array_equal(o_v.cpu().numpy(), eo.topk_of(ed, esp, k, True)[2])


@pytest.mark.parametrize("dtype,steps,lower", [("f64", (0, 2), False), ("i64", (1, 3), True)])
def test_rows_split_over_batches(dlc, dtype, steps, lower):
    """A cell is a function of the L rows behind it: batches of 1, 7 and 32 rows, each with its L - 1 context rows in
    front (row0), give the lists of the whole matrix."""
    e = dlc.default_engine()
    rng = np.random.RandomState(40)
    rows, n, L, k, limit0 = 75, 300, 10, 5, -4
    m = data(rng, dtype, rows, n)
    for r in range(L - 1, rows, 7):
        plant(m, r, int(rng.randint(0, n)), steps, L, rng, lower)
    es, ei, ev = eo.elastic_topk(m, k, L, steps[0], steps[1], n, limit0, 1, lower)
    dev = torch.from_numpy(m).to(e.device)
    for batch in (1, 7, 32):
        outs = []
        for lo in range(0, rows, batch):
            base = max(0, lo - (L - 1))
            outs.append(e.sequence_elastic_topk(dev[base:lo + batch], L, steps, k=k, row0=lo - base, limit0=limit0 + base,
                                                limit_step=1, lower_is_better=lower)[:3])
        s, i, v = (torch.cat([o[t] for o in outs]).cpu().numpy() for t in range(3))
        assert np.array_equal(i, ei) and np.array_equal(v, ev) and so.same_bits(s, es), batch


def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    m = torch.zeros((8, 50), dtype=torch.float64, device=e.device)
    o_s = torch.full((8, 4), SENTINEL, dtype=torch.int64, device=e.device)
    o_i = torch.full((8, 4), SENTINEL, dtype=torch.int64, device=e.device)
    o_v = torch.full((8, 4), 0x5A5A5A5A, dtype=torch.int32, device=e.device)
    seq = torch.full((8, 50), SENTINEL, dtype=torch.int64, device=e.device)
    word = torch.zeros(1, dtype=torch.int64, device=e.device)
    size = e.lib.dlc_sequence_elastic_topk_workspace_bytes
    need = size(8, 50, 3, 0, 2, 4)
    assert need == 8 * 1 * 4 * 16 and size(41, 100_000, 10, 0, 2, 5) == (41 * 94 * 5 * 16 + 255) // 256 * 256
    for args in ((0, 50, 3, 0, 2, 4), (8, 0, 3, 0, 2, 4), (8, 1 << 31, 3, 0, 2, 4), (8, 50, 0, 0, 2, 4), (8, 50, 65, 0, 2, 4),
                 (8, 50, 3, 3, 2, 4), (8, 50, 3, -1, 2, 4), (8, 50, 3, 0, 9, 4), (8, 50, 3, 0, 2, 0), (8, 50, 3, 0, 2, MAX_K + 1)):
        assert size(*args) == 0, args
    ws = torch.empty(need + 16, dtype=torch.uint8, device=e.device)
    src, ds, di, dv, dq, wp, pw = (C.c_void_p(t.data_ptr()) for t in (m, o_s, o_i, o_v, seq, ws, word))
    f = e.lib.dlc_sequence_elastic_topk
    names = ["ctx", "dtype", "scores", "rows", "row0", "n", "ld", "limit0", "step", "L", "d_min", "d_max", "lower", "k", "out_s",
             "out_i", "out_v", "seq", "ld_out", "poison", "ws", "bytes", "stream"]
    ok = (e.ctx, _lib.DLC_F64, src, 8, 0, 50, 50, 50, 0, 3, 0, 2, 0, 4, ds, di, dv, dq, 50, None, wp, need, None)
    assert len(ok) == len(names) and f(*ok) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert o_i[2:, 0].tolist() == [0] * 6 and o_i[:2, 0].tolist() == [-1] * 2 and o_v[2:].unique().tolist() == [0]
    for t in (o_s, o_i, seq):
        t.fill_(SENTINEL)
    o_v.fill_(0x5A5A5A5A)

    def but(**change):
        return tuple(change.get(name, v) for name, v in zip(names, ok))

    bad = {"dtype": but(dtype=_lib.DLC_I8), "null scores": but(scores=None), "null out_scores": but(out_s=None),
           "null out_idx": but(out_i=None), "no output": but(out_s=None, out_i=None, out_v=None, seq=None),
           "rows 0": but(rows=0), "row0 = rows": but(row0=8), "row0 < 0": but(row0=-1), "n 0": but(n=0), "ld < n": but(ld=49),
           "ld_out < n": but(ld_out=49), "n 2^31": but(n=1 << 31, ld=1 << 31), "L 0": but(L=0), "L 65": but(L=65),
           "d_min > d_max": but(d_min=3), "d_min < 0": but(d_min=-1), "d_max 9": but(d_max=9), "k 0": but(k=0),
           "k 129": but(k=129), "poison with int64": but(dtype=_lib.DLC_I64, poison=pw)}
    # a scores pointer off its element's alignment, inside a buffer a row larger than the call describes
    big = torch.zeros(9 * 50, dtype=torch.float64, device=e.device)
    assert big.data_ptr() % 8 == 0
    for name, dt, shift in (("f64", _lib.DLC_F64, 4), ("f32", _lib.DLC_F32, 2), ("i64", _lib.DLC_I64, 4)):
        bad["misaligned scores " + name] = but(dtype=dt, scores=C.c_void_p(big.data_ptr() + shift))
    for what, args in bad.items():
        assert f(*args) == _lib.DLC_ERR_BAD_ARG, what
        assert b"sequence_elastic_topk" in e.lib.dlc_last_error(e.ctx), what
    assert f(*but(ctx=None)) == _lib.DLC_ERR_BAD_ARG
    for what, args in {"no workspace": but(ws=None), "short": but(bytes=need - 1),
                       "misaligned": but(ws=C.c_void_p(ws.data_ptr() + 8))}.items():
        assert f(*args) == _lib.DLC_ERR_WORKSPACE, what
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (o_s, o_i, seq)) and bool((o_v == 0x5A5A5A5A).all()), "an error wrote"
    # the engine's and the module's own checks
    e.sequence_elastic_topk(m, 3, (0, 2), k=3)
    for steps in ((3, 2), (-1, 2), (0, 9), (0,), (0, 1, 2), 2, (0, 1.5), None):
        with pytest.raises(ValueError):
            e.sequence_elastic_topk(m, 3, steps, k=3)
    for kw in (dict(k=0), dict(k=MAX_K + 1), dict(k=3, row0=8), dict(k=3, row0=-1), dict(k=3, n=51), dict(k=3, n=0), dict()):
        with pytest.raises(ValueError):
            e.sequence_elastic_topk(m, 3, (0, 2), **kw)
    with pytest.raises(ValueError):
        e.sequence_elastic_topk(m, 65, (0, 2), k=3)
    for scores in (m.to(torch.float16), m.cpu(), m[0]):
        with pytest.raises(ValueError):
            e.sequence_elastic_topk(scores, 3, (0, 2), k=3)
    with pytest.raises(ValueError):
        dlc.sequence_topk(m, 3, 3, offsets=[[0, 1, 2]], steps=(0, 2))
    with pytest.raises(ValueError):
        dlc.sequence_scores(m, 3, steps=(2, 1))


def test_module_functions_numpy_and_tensors(dlc):
    """deeploopcloser_amd.sequence with steps=: NumPy in -> NumPy out, tensors in -> tensors out; contrast in front and
    suppress behind, each against the chain of oracles; steps=None is the linear search."""
    rng = np.random.RandomState(10)
    e = dlc.default_engine()
    x = rng.randint(-128, 128, size=(60, 33)).astype(np.int8)
    dist = dlc.DistanceCalculator.distance_matrix(x)
    kw = dict(limit0=-3, limit_step=1, lower_is_better=True)
    s, i, v = dlc.sequence_topk(dist, 3, 6, steps=(0, 2), **kw)
    es, ei, ev = eo.elastic_topk(dist, 3, 6, 0, 2, **kw)
    assert isinstance(s, np.ndarray) and s.dtype == np.int64 and np.array_equal(s, es) and np.array_equal(i, ei) and np.array_equal(v, ev)
    t = torch.from_numpy(dist).to(e.device)
    s, i, v = dlc.sequence_topk(t, 3, 6, steps=(0, 2), **kw)
    assert isinstance(s, torch.Tensor) and s.device == e.device and v.dtype == torch.int32
    assert np.array_equal(s.cpu().numpy(), es) and np.array_equal(i.cpu().numpy(), ei) and np.array_equal(v.cpu().numpy(), ev)
    d = dlc.sequence_scores(dist, 6, steps=(0, 2), **kw)
    assert np.array_equal(d, eo.elastic_scores(dist, 6, 0, 2, **kw)[0])
    normal = co.contrast_rows(dist, 5, limit0=-3, limit_step=1)
    cs, ci, cv = dlc.sequence_topk(dist, 3, 6, steps=(1, 3), contrast=5, **kw)
    es, ei, ev = eo.elastic_topk(normal, 3, 6, 1, 3, **kw)
    assert so.same_bits(cs, es) and np.array_equal(ci, ei) and np.array_equal(cv, ev)
    ps, pi = dlc.sequence_peaks(dist, 3, 6, 4, steps=(0, 2), **kw)
    es, ei = po.peak_topk_rows(eo.elastic_scores(dist, 6, 0, 2, **kw)[0], 3, 4, absent=-1, **kw)
    assert np.array_equal(ps, es) and np.array_equal(pi, ei)
    a, b = dlc.sequence_topk(dist, 3, 6, steps=None, **kw), dlc.sequence_topk(dist, 3, 6, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert np.array_equal(a[1], so.sequence_topk(dist, 3, 6, dlc.slope_offsets(6), **kw)[1])


# ---- the detectors ------------------------------------------------------------------------------------------------------
L_SEQ, STEPS, K_DET, EXCLUSION = 4, (0, 2), 3, 10


def int8_scene(units):
    return po.two_place_scene(0, lambda rng, c: rng.randint(-128, 128, size=c).astype(np.int8), units)


def stream(det, x, batch):
    """The lists of x's frames through det in batches of `batch` (a list: those sizes in turn, then the rest at once)."""
    sizes = batch if isinstance(batch, list) else [batch] * (x.shape[0] // batch + 1)
    outs, f = [], 0
    for b in sizes + [x.shape[0]]:
        take = min(b, x.shape[0] - f)
        if take > 0:
            outs.append(det.query_and_insert(x[f:f + take]))
            f += take
    return torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy()


MIXED = [1, 2, 9, 1, 40, 3]                                              # shorter and longer than the context


def same_lists(results, es, ei):
    for s, i in results:
        assert s.dtype == es.dtype and np.array_equal(i, ei) and so.same_bits(s, es)


def test_cnn_vtl_detector(dlc):
    x = int8_scene(64)

    def make(**kw):
        return dlc.CnnVtlLoopClosureDetector(64, k=K_DET, exclusion=EXCLUSION, capacity=64, **kw)

    d = dlc.DistanceCalculator.distance_matrix(x)                                  # the detector's own raw rows, as a matrix
    kw = dict(limit0=-EXCLUSION, limit_step=1, lower_is_better=True)
    es, ei, _ = eo.elastic_topk(d, K_DET, L_SEQ, STEPS[0], STEPS[1], **kw)
    assert es.dtype == np.int64 and (ei[:L_SEQ - 1 + EXCLUSION] == -1).all() and (ei[L_SEQ + EXCLUSION:, 0] >= 0).all()
    same_lists([stream(make(sequence=L_SEQ, steps=STEPS), x, batch) for batch in (1, 7, 32, MIXED)], es, ei)
    # contrast in front and suppress behind, composed: the chain of oracles
    normal = co.contrast_rows(d, 5, limit0=-EXCLUSION, limit_step=1)
    cs, ci = po.peak_topk_rows(eo.elastic_scores(normal, L_SEQ, STEPS[0], STEPS[1], **kw)[0], K_DET, 5, **kw)
    same_lists([stream(make(sequence=L_SEQ, steps=STEPS, contrast=5, suppress=5), x, batch) for batch in (7, 32)], cs, ci)
    # a fixed step of 1 is the line of velocity 1, index for index (int64 rows: the sums do not depend on the order)
    line = np.arange(L_SEQ, dtype=np.int32)[None, :]
    a, b = stream(make(sequence=L_SEQ, steps=(1, 1)), x, 7), stream(make(sequence=L_SEQ, slopes=line), x, 32)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    for bad in (dict(steps=STEPS), dict(sequence=L_SEQ, steps=STEPS, slopes=line), dict(sequence=L_SEQ, steps=(2, 1)),
                dict(sequence=L_SEQ, steps=(0, 9)), dict(sequence=L_SEQ, steps=(0, 1, 2))):
        with pytest.raises(ValueError):
            make(**bad)
    # steps=None is the detector as it was
    a, b = stream(make(sequence=L_SEQ, steps=None), x, 32), stream(make(sequence=L_SEQ), x, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_cosine_detector(dlc):
    x = int8_scene(256).astype(np.float32)

    def make(**kw):
        return dlc.LoopClosureDetector(256, k=K_DET, exclusion=EXCLUSION, capacity=16, **kw)

    results = []
    for batch in (1, 7, 32, MIXED):
        det = make(sequence=L_SEQ, steps=STEPS)
        results.append(stream(det, x, batch))
    keys = det.db.score_keys(det.db.rows).cpu().numpy()                            # the detector's own raw rows: int64 keys
    kw = dict(limit0=-EXCLUSION, limit_step=1)
    ks, ei, _ = eo.elastic_topk(keys, K_DET, L_SEQ, STEPS[0], STEPS[1], **kw)
    es = np.where(ei >= 0, ks.astype(np.float64) * 2.0 ** -40, -np.inf)            # key sums -> scores, as the detector does
    same_lists(results, es, ei)
    normal = co.contrast_rows(keys, 5, limit0=-EXCLUSION, limit_step=1)
    cs, ci = po.peak_topk_rows(eo.elastic_scores(normal, L_SEQ, STEPS[0], STEPS[1], **kw)[0], K_DET, 5, **kw)
    same_lists([stream(make(sequence=L_SEQ, steps=STEPS, contrast=5, suppress=5), x, batch) for batch in (7, 32)], cs, ci)
    line = np.arange(L_SEQ, dtype=np.int32)[None, :]
    a, b = stream(make(sequence=L_SEQ, steps=(1, 1)), x, 7), stream(make(sequence=L_SEQ, slopes=line), x, 32)
    assert np.array_equal(a[1], b[1]) and so.same_bits(a[0], b[0])
    for bad in (dict(steps=STEPS), dict(sequence=L_SEQ, steps=STEPS, slopes=line), dict(sequence=L_SEQ, steps=(0, 9))):
        with pytest.raises(ValueError):
            make(**bad)
    a, b = stream(make(sequence=L_SEQ, steps=None), x, 32), stream(make(sequence=L_SEQ), x, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sdav_detector(dlc):
    e = dlc.default_engine()
    scene = po.two_place_scene(0, lambda rng, c: 1.0 / (1.0 + np.exp(-4.0 * rng.standard_normal((c, 250)))), 30)
    scene = np.clip(scene + 0.01 * np.random.RandomState(100).rand(*scene.shape), 0.001, 0.999)   # no two patches alike
    ds = torch.from_numpy(scene).to(e.device)
    n = ds.shape[0]

    def make(**kw):
        return dlc.SdavLoopClosureDetector(ds, patches=30, width=250, k=K_DET, exclusion=EXCLUSION, capacity=8, **kw)

    sim = dlc.SimilarityCalculator(scene).similarity_matrix(as_int64=False)        # the detector's own raw rows
    kw = dict(limit0=-EXCLUSION, limit_step=1)
    es, ei, _ = eo.elastic_topk(sim, K_DET, L_SEQ, STEPS[0], STEPS[1], **kw)
    assert (ei[:L_SEQ - 1 + EXCLUSION] == -1).all() and np.isneginf(es[:L_SEQ - 1 + EXCLUSION]).all()
    same_lists([stream(make(sequence=L_SEQ, steps=STEPS), ds, batch) for batch in (1, 7, 32, MIXED)], es, ei)
    det, outs, tickets = make(sequence=L_SEQ, steps=STEPS), [], []
    for lo in range(0, n, 16):                                                     # two batches in flight
        tickets.append(det.submit(ds[lo:lo + 16]))
        if len(tickets) > 1:
            outs.append(det.result(tickets[-2]))
    outs.append(det.result(tickets[-1]))
    same_lists([(torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy())], es, ei)
    normal = co.contrast_rows(sim, 5, limit0=-EXCLUSION, limit_step=1)
    cs, ci = po.peak_topk_rows(eo.elastic_scores(normal, L_SEQ, STEPS[0], STEPS[1], **kw)[0], K_DET, 5, **kw)
    same_lists([stream(make(sequence=L_SEQ, steps=STEPS, contrast=5, suppress=5), ds, batch) for batch in (7, 32)], cs, ci)
    for bad in (dict(steps=STEPS), dict(sequence=L_SEQ, steps=STEPS, slopes=[[0, 1, 2, 3]]), dict(sequence=L_SEQ, steps=(3, 1))):
        with pytest.raises(ValueError):
            make(**bad)
    a, b = stream(make(sequence=L_SEQ, steps=None), ds, 32), stream(make(sequence=L_SEQ), ds, 7)
    assert so.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a poisoned stream still answers (NaN, -1)
    det = make(sequence=3, steps=(0, 1))
    det.query_and_insert(ds[:20])
    bad = ds[20].clone()
    bad[1, 1] = 1.5
    s, i = det.query_and_insert(bad)
    assert bool(s.isnan().all()) and bool((i == -1).all())


def test_planted_revisit_at_a_changing_speed_through_the_detector(dlc):
    """tests/test_elastic_cpu.py's planted case through CnnVtlLoopClosureDetector: of the 51 frames whose chain lies inside
    the revisit, sequence=10 with the default lines finds the true place for 26 (at most 30), steps=(0, 2) for all 51."""
    x, true, alias, first = eo.planted_elastic_revisit()

    def found(**kw):
        det = dlc.CnnVtlLoopClosureDetector(64, k=1, exclusion=30, capacity=512, sequence=10, **kw)
        ids = stream(det, x, 32)[1][:, 0]
        return int((ids[first + 9:first + 60] == true[9:]).sum())

    linear, elastic = found(), found(steps=(0, 2))
    print("true place found of 51: linear %d, elastic %d" % (linear, elastic))
    assert elastic == 51
    assert linear <= 30 and linear == 26
    single = stream(dlc.CnnVtlLoopClosureDetector(64, k=1, exclusion=30, capacity=512), x, 32)[1][:, 0]
    assert np.array_equal(single[first:first + 60], alias)


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_steps(dlc):
    common = ("--network", "sdav", "--metric", "similarity", "--exclusion", "2", "--k", "2", "--batch", "4")
    res = run_cli(*common, "--sequence", "3", "--steps", "0:2")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    loops = [l.split("\t") for l in res.stdout.splitlines() if l.startswith("loop\t")]
    assert loops and all(int(l[1]) - int(l[3]) > 2 and int(l[1]) >= 2 + 2 + 1 for l in loops)   # old enough, a full chain behind it
    for args in (common + ("--steps", "0:2"), common + ("--sequence", "3", "--steps", "0:9")):
        res = run_cli(*args)
        assert res.returncode == 2 and "error:" in res.stderr and "--steps" in res.stderr
