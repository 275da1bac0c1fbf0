"""GPU sequence search (dlc_sequence_topk, Engine.sequence_topk, deeploopcloser_amd.sequence, SdavLoopClosureDetector with
sequence=L, the CLI) against the NumPy restatement of the definition (tests/sequence_oracle.py).  Every comparison is
exact: integers by value, fp64 by bit pattern, NaN slots by position."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import sequence_oracle as so

pytestmark = pytest.mark.gpu

MAX_K = 128
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def table(rng, slopes, L, top):
    """A random valid offset table: rows start at 0 and never decrease."""
    t = np.sort(rng.randint(0, top + 1, size=(slopes, L)), axis=1).astype(np.int32)
    t[:, 0] = 0
    return t


def padded(dlc, m, ld, fill):
    """m [rows, n] on the device inside a [rows, ld] buffer whose other columns hold a value that would win if it were read."""
    e = dlc.default_engine()
    buf = torch.full((m.shape[0], ld), fill, dtype=torch.from_numpy(m[:1, :1]).dtype, device=e.device)
    buf[:, :m.shape[1]] = torch.from_numpy(m).to(e.device)
    return buf


def check(dlc, m, L, offsets, k, row0=0, limit0=None, step=0, lower=False, pad=5):
    e = dlc.default_engine()
    n = m.shape[1]
    if m.dtype == np.int64:
        fill = -(1 << 40) if lower else (1 << 40)
    else:
        fill = -1e30 if lower else 1e30
    buf = padded(dlc, m, n + pad, fill)
    s, i, v, d = e.sequence_topk(buf, L, offsets, k=k, row0=row0, n=n, limit0=limit0, limit_step=step, lower_is_better=lower,
                                 dense=True)
    es, ei, ev = so.sequence_topk(m, k, L, offsets, n, limit0, step, lower, row0)
    ed, _ = so.sequence_scores(m, L, offsets, n, limit0, step, lower, row0)
    assert np.array_equal(i.cpu().numpy(), ei), "indices"
    assert np.array_equal(v.cpu().numpy(), ev), "slopes"
    assert so.same_bits(s.cpu().numpy(), es), "scores"
    assert so.same_bits(d.cpu().numpy(), ed), "dense scores"
    # the lists alone (no dense output: the scan then stops at the columns the rows offer) are the same lists
    s2, i2, v2, d2 = e.sequence_topk(buf, L, offsets, k=k, row0=row0, n=n, limit0=limit0, limit_step=step, lower_is_better=lower)
    assert d2 is None and torch.equal(i2, i) and torch.equal(v2, v) and so.same_bits(s2.cpu().numpy(), s.cpu().numpy())
    return s, i, v


def data(rng, dtype, rows, n):
    if dtype == "i64":
        return rng.randint(-1000, 1000, size=(rows, n)).astype(np.int64)
    m = rng.standard_normal((rows, n))
    return m.astype(np.float32) if dtype == "f32" else m


# (dtype, L, slopes, rows, row0, n, k, limit0, limit_step, lower): every value of each axis at least once -- dtype, L (1, 2,
# 10, 33, 64), slopes (1, 5, 16), rows (1, L-1, L, 300), row0 (0, L-1), n (1, 7, 1000, 70 001), k (1, 20, 128), limit_step
# (0, 1) with negative and over-large limit0, both senses; then k = 63, 64, 65, where a list's last entry moves from a
# lane's first register to its second
SWEEP = [
    ("f64", 1, 1, 1, 0, 1, 1, None, 0, False),
    ("f32", 2, 5, 1, 0, 7, 20, -3, 1, True),                      # rows = L - 1: nothing is offered
    ("i64", 10, 5, 10, 9, 1000, MAX_K, 1050, 0, True),            # rows = L, row0 = L - 1, limit0 past n
    ("f64", 10, 5, 300, 0, 1000, 20, -40, 1, False),
    ("f64", 33, 16, 300, 32, 1000, MAX_K, 700, 1, False),         # limits that grow past n
    ("i64", 64, 16, 300, 63, 1000, 20, None, 0, True),
    ("f32", 64, 5, 64, 0, 7, 1, 100, 0, False),
    ("f64", 2, 1, 300, 1, 70001, 20, 70011, 0, True),
    ("i64", 10, 5, 9, 0, 70001, MAX_K, 60000, 1, False),          # rows = L - 1
    ("f32", 33, 1, 32, 0, 1, 20, None, 0, False),
    ("f64", 1, 1, 300, 0, 70001, MAX_K, 100, 250, False),
    ("f32", 10, 16, 300, 9, 1000, 20, -100, 5, True),
    ("i64", 2, 5, 2, 1, 7, 1, -1, 1, False),
    ("f64", 33, 5, 33, 32, 70001, 1, 69000, 1, False),
    ("i64", 1, 1, 1, 0, 1000, MAX_K, -5, 1, True),
    ("f32", 64, 16, 63, 0, 1000, MAX_K, None, 0, True),           # rows = L - 1
    ("f64", 2, 5, 40, 1, 1000, 63, None, 0, False),
    ("f64", 2, 5, 40, 1, 1000, 64, None, 0, False),
    ("f64", 2, 5, 40, 1, 1000, 65, None, 0, False),
    ("i64", 2, 5, 40, 1, 1000, 63, -3, 1, True),
    ("i64", 2, 5, 40, 1, 1000, 64, -3, 1, True),
    ("i64", 2, 5, 40, 1, 1000, 65, -3, 1, True),
    ("i64", 2, 5, 40, 1, 1000, 63, None, 0, True),                # (the limits above keep those lists short of k: these fill)
    ("i64", 2, 5, 40, 1, 1000, 64, None, 0, True),
    ("i64", 2, 5, 40, 1, 1000, 65, None, 0, True),
]


@pytest.mark.parametrize("dtype,L,slopes,rows,row0,n,k,limit0,step,lower", SWEEP)
def test_sweep(dlc, dtype, L, slopes, rows, row0, n, k, limit0, step, lower):
    rng = np.random.RandomState(L * 1000 + slopes * 100 + rows + n + k)
    offsets = table(rng, slopes, L, max(1, 2 * (L - 1)))
    check(dlc, data(rng, dtype, rows, n), L, offsets, k, row0, limit0, step, lower)


def test_default_slopes_at_every_length(dlc):
    """The tables slope_offsets gives, among them L = 64 (a window of 127 rows: the narrow tile) -- and a table whose
    offsets reach thousands of columns, which no window holds (the matrix is read through the caches)."""
    rng = np.random.RandomState(5)
    for L in (1, 2, 10, 33, 64):
        check(dlc, data(rng, "f64", 130, 3000), L, dlc.slope_offsets(L), 20, L - 1, -10, 1, False)
        check(dlc, data(rng, "i64", 130, 3000), L, dlc.slope_offsets(L), 20, 0, None, 0, True)
    far = np.array([[0, 5, 32767], [0, 0, 0], [0, 20000, 20000]], dtype=np.int32)
    for dtype in ("f64", "f32", "i64"):
        check(dlc, data(rng, dtype, 40, 70001), 3, far, 20, 2, None, 0, dtype == "i64")
        check(dlc, data(rng, dtype, 40, 70001), 3, far, MAX_K, 0, 40000, 500, dtype != "i64")


def test_ties(dlc):
    """Small-integer matrices: ties between cells (the lower column first) and between slopes (the lowest slope)."""
    rng = np.random.RandomState(6)
    for dtype in (np.int64, np.float64, np.float32):
        for L, slopes in ((1, 1), (3, 5), (10, 16)):
            m = rng.randint(-2, 3, size=(70, 2500)).astype(dtype)
            offsets = table(rng, slopes, L, 6)
            offsets[-1] = offsets[0]                                   # the same line twice: the first wins
            for lower in (False, True):
                s, i, v = check(dlc, m, L, offsets, MAX_K, 0, None, 0, lower)
                assert int(v.max()) < slopes - 1 or slopes == 1
    same = np.full((12, 900), 2.5)
    s, i, v = check(dlc, same, 4, dlc.slope_offsets(4), 20, 3, None, 0, False)
    assert (i.cpu().numpy() == np.arange(2, 22)).all() and (v == 0).all() and (s == 10.0).all()   # columns 0, 1: no line fits
    zeros = np.zeros((3, 300))
    zeros[:, ::2] = -0.0                                               # -0.0 ranks below +0.0, as in dlc_topk_rows_f64
    check(dlc, zeros, 1, [[0]], 20)
    check(dlc, zeros, 2, [[0, 1], [0, 0]], 20, lower=True)


def test_non_finite_entries(dlc):
    rng = np.random.RandomState(8)
    for dtype in (np.float64, np.float32):
        m = rng.standard_normal((60, 1200)).astype(dtype)
        m[rng.rand(60, 1200) < 0.02] = np.nan
        m[rng.rand(60, 1200) < 0.02] = np.inf
        m[rng.rand(60, 1200) < 0.02] = -np.inf                        # +inf + -inf on a line: a NaN sum, never taken
        m[7] = np.nan
        m[20] = np.inf
        m[21, ::3] = -np.inf
        for lower in (False, True):
            s, i, v = check(dlc, m, 5, dlc.slope_offsets(5), 20, 4, None, 0, lower)
            check(dlc, m, 1, [[0]], MAX_K, 0, 900, 1, lower)
        assert not bool(s.isnan().any())
        assert bool((i[7 - 4:7 + 1] == -1).all())                     # every line through row 7 is NaN


def test_poison_word(dlc):
    e = dlc.default_engine()
    m = torch.randn((20, 500), dtype=torch.float64, device=e.device)
    word = torch.zeros(1, dtype=torch.int64, device=e.device)
    off = dlc.slope_offsets(3)
    clean = e.sequence_topk(m, 3, off, k=7, dense=True)
    same = e.sequence_topk(m, 3, off, k=7, dense=True, poison=word)
    assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
               for a, b in zip(clean, same))
    s, i, v, d = e.sequence_topk(m, 3, off, k=7, dense=True, poison=word + 5)
    assert bool(s.isnan().all()) and bool((i == -1).all()) and bool((v == -1).all()) and bool(d.isnan().all())
    s, i, v, d = e.sequence_topk(m.float(), 3, off, k=7, poison=word + 1)
    assert bool(s.isnan().all()) and bool((i == -1).all()) and d is None
    with pytest.raises(ValueError):
        e.sequence_topk(m.long(), 3, off, k=7, poison=word)


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
        for kk in (1, k, MAX_K):
            ws, wi = e.topk_rows_f64(sc, limit0, step, kk)
            s, i, v, _ = e.sequence_topk(sc, 1, [[0]], k=kk, limit0=limit0, limit_step=step)
            assert torch.equal(i, wi) and torch.equal(s.view(torch.int64), ws.view(torch.int64)), (limit0, step, kk)
            assert torch.equal(v, torch.where(i >= 0, 0, -1).to(torch.int32))


def test_bad_arguments(dlc):
    e = dlc.default_engine()
    m = torch.zeros((8, 50), dtype=torch.float64, device=e.device)
    ok = np.array([[0, 1, 2]], dtype=np.int32)
    e.sequence_topk(m, 3, ok, k=3)
    for bad in ([[1, 1, 2]], [[0, 2, 1]], [[0, 1, 32768]], [[0, -1, 0]], [[0, 1]], [0, 1, 2], [[0, 1.5, 2]]):
        with pytest.raises(ValueError):
            e.sequence_topk(m, 3, bad, k=3)
    with pytest.raises(ValueError):
        e.sequence_topk(m, 3, np.zeros((17, 3), np.int32), k=3)        # too many slopes
    with pytest.raises(ValueError):
        e.sequence_topk(m, 65, np.zeros((1, 65), np.int32), k=3)       # too long
    with pytest.raises(ValueError):
        e.sequence_topk(m, 65, np.zeros((1, 65), np.int32), dense=True)
    for kw in (dict(k=0), dict(k=MAX_K + 1), dict(k=3, row0=8), dict(k=3, row0=-1), dict(k=3, n=51), dict(k=3, n=0), dict()):
        with pytest.raises(ValueError):
            e.sequence_topk(m, 3, ok, **kw)
    with pytest.raises(ValueError):
        e.sequence_topk(m.to(torch.float16), 3, ok, k=3)
    with pytest.raises(ValueError):
        e.sequence_topk(m.cpu(), 3, ok, k=3)
    with pytest.raises(ValueError):
        e.sequence_topk(m[0], 3, ok, k=3)
    assert e.lib.dlc_sequence_topk_workspace_bytes(8, 50, 3, 1, 3) > 0
    for args in ((0, 50, 3, 1, 3), (8, 0, 3, 1, 3), (8, 1 << 31, 3, 1, 3), (8, 50, 0, 1, 3), (8, 50, 65, 1, 3), (8, 50, 3, 0, 3),
                 (8, 50, 3, 17, 3), (8, 50, 3, 1, 0), (8, 50, 3, 1, MAX_K + 1)):
        assert e.lib.dlc_sequence_topk_workspace_bytes(*args) == 0
    # the library's own checks of the pointers the engine never gets wrong; no call here reaches a launch
    from deeploopcloser_amd import _lib
    need = e.lib.dlc_sequence_topk_workspace_bytes(8, 50, 3, 1, 4)
    o_s = torch.full((8, 4), SENTINEL, dtype=torch.int64, device=e.device)
    o_i = torch.full((8, 4), SENTINEL, dtype=torch.int64, device=e.device)
    o_v = torch.full((8, 4), 0x5A5A5A5A, dtype=torch.int32, device=e.device)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=e.device)
    assert ws.data_ptr() % 16 == 0
    off = (C.c_int32 * 3)(0, 1, 2)
    names = ["ctx", "dtype", "scores", "rows", "row0", "n", "ld", "limit0", "step", "L", "n_slopes", "offsets", "lower", "k",
             "out_s", "out_i", "out_v", "seq", "ld_out", "poison", "ws", "bytes", "stream"]
    good = (e.ctx, _lib.DLC_F64, C.c_void_p(m.data_ptr()), 8, 0, 50, 50, 50, 0, 3, 1, off, 0, 4, C.c_void_p(o_s.data_ptr()),
            C.c_void_p(o_i.data_ptr()), C.c_void_p(o_v.data_ptr()), None, 50, None, C.c_void_p(ws.data_ptr()), need, None)
    assert len(good) == len(names)

    def but(**change):
        return tuple(change.get(name, v) for name, v in zip(names, good))

    f = e.lib.dlc_sequence_topk
    assert f(*good) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert o_i[2:, 0].tolist() == [2] * 6 and o_i[:2, 0].tolist() == [-1] * 2      # (column 2 is the first with a whole line)
    o_s.fill_(SENTINEL), o_i.fill_(SENTINEL), o_v.fill_(0x5A5A5A5A)
    # a scores pointer off its element's alignment, inside a buffer a row larger than the call describes
    big = torch.zeros(9 * 50, dtype=torch.float64, device=e.device)
    assert big.data_ptr() % 8 == 0
    for name, dt, shift in (("f64", _lib.DLC_F64, 4), ("f32", _lib.DLC_F32, 2), ("i64", _lib.DLC_I64, 4)):
        assert f(*but(dtype=dt, scores=C.c_void_p(big.data_ptr() + shift))) == _lib.DLC_ERR_BAD_ARG, name
        assert b"sequence_topk" in e.lib.dlc_last_error(e.ctx), name
    assert f(*but(n=1 << 31, ld=1 << 31)) == _lib.DLC_ERR_BAD_ARG
    assert f(*but(ws=C.c_void_p(ws.data_ptr() + 8))) == _lib.DLC_ERR_WORKSPACE
    assert b"sequence_topk" in e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (o_s, o_i)) and bool((o_v == 0x5A5A5A5A).all()), "an error wrote"


def test_module_functions_numpy_and_tensors(dlc):
    """deeploopcloser_amd.sequence: NumPy in -> NumPy out, tensors in -> tensors out, on the reference's two matrices as
    they come (the similarity as int64 and as fp64, the distance as int64)."""
    rng = np.random.RandomState(10)
    e = dlc.default_engine()
    ds = 1.0 / (1.0 + np.exp(-4.0 * rng.standard_normal((50, 6, 40))))
    calc = dlc.SimilarityCalculator(ds)
    for m in (calc.similarity_matrix(), calc.similarity_matrix(as_int64=False)):
        s, i, v = dlc.sequence_topk(m, 5, 4, limit0=-3, limit_step=1)
        es, ei, ev = so.sequence_topk(m, 5, 4, dlc.slope_offsets(4), limit0=-3, limit_step=1)
        assert isinstance(s, np.ndarray) and so.same_bits(s, es) and np.array_equal(i, ei) and np.array_equal(v, ev)
        d = dlc.sequence_scores(m, 4, limit0=-3, limit_step=1)
        assert so.same_bits(d, so.sequence_scores(m, 4, dlc.slope_offsets(4), limit0=-3, limit_step=1)[0])
    x = rng.randint(-128, 128, size=(60, 33)).astype(np.int8)
    dist = dlc.DistanceCalculator.distance_matrix(x)
    t = torch.from_numpy(dist).to(e.device)
    s, i, v = dlc.sequence_topk(t, 3, 6, lower_is_better=True)
    es, ei, ev = so.sequence_topk(dist, 3, 6, dlc.slope_offsets(6), lower_is_better=True)
    assert isinstance(s, torch.Tensor) and s.dtype == torch.int64 and s.device == e.device
    assert np.array_equal(s.cpu().numpy(), es) and np.array_equal(i.cpu().numpy(), ei) and np.array_equal(v.cpu().numpy(), ev)
    d = dlc.sequence_scores(t, 6, lower_is_better=True)
    assert np.array_equal(d.cpu().numpy(), so.sequence_scores(dist, 6, dlc.slope_offsets(6), lower_is_better=True)[0])
    view = torch.randn((30, 700), dtype=torch.float64, device=e.device)[:, 100:500]      # a row-strided view, taken as it is
    s, i, v = dlc.sequence_topk(view, 4, 3)
    es, ei, ev = so.sequence_topk(view.cpu().numpy(), 4, 3, dlc.slope_offsets(3))
    assert so.same_bits(s.cpu().numpy(), es) and np.array_equal(i.cpu().numpy(), ei)


def test_planted_revisit_on_the_gpu(dlc):
    """tests/test_sequence_cpu.py's planted revisit through DistanceCalculator.distance_matrix and sequence_topk: the
    single-frame arg-min is right for 0 of 60 frames, the sequence arg-min for 51 of 51."""
    x, true, alias = so.planted_revisit()
    dist = dlc.DistanceCalculator.distance_matrix(x)
    _, i1, _ = dlc.sequence_topk(dist, 1, 1, limit0=-30, limit_step=1, lower_is_better=True)
    assert int((i1[200:260, 0] == true).sum()) == 0 and np.array_equal(i1[200:260, 0], alias)
    _, i10, v10 = dlc.sequence_topk(dist, 1, 10, limit0=-30, limit_step=1, lower_is_better=True)
    assert i10[209:260, 0].size == 51 and int((i10[209:260, 0] == true[9:]).sum()) == 51
    e_s, e_i, e_v = so.sequence_topk(dist, 1, 10, dlc.slope_offsets(10), limit0=-30, limit_step=1, lower_is_better=True)
    assert np.array_equal(i10, e_i) and np.array_equal(v10, e_v)


@pytest.mark.parametrize("L,slopes", [(4, None), (1, None), (6, "wide")])
def test_detector_with_sequence(dlc, L, slopes):
    """SdavLoopClosureDetector(sequence=L): the lists do not depend on the batching (1, 7, 32, mixed, submit / result),
    equal the oracle applied to SimilarityCalculator's fp64 matrix of the same frames, and stay equal across a growth of
    the stream (capacity 8 -> 140 frames)."""
    e = dlc.default_engine()
    g = torch.Generator(device=e.device)
    g.manual_seed(31 + L)
    n, p, h, k, exclusion = 140, 6, 48, 4, 5
    ds = torch.sigmoid(4.0 * torch.randn((n, p, h), generator=g, device=e.device, dtype=torch.float64))
    ds[100:130] = (ds[20:50] + 0.01 * torch.rand((30, p, h), generator=g, device=e.device, dtype=torch.float64)).clamp(0.001, 0.999)
    table_ = None if slopes is None else np.array([[0, 0, 1, 1, 2, 2], [0, 1, 2, 3, 4, 5], [0, 2, 4, 6, 8, 10]], dtype=np.int32)
    offsets = dlc.slope_offsets(L) if table_ is None else table_
    sim = dlc.SimilarityCalculator(ds.cpu().numpy()).similarity_matrix(as_int64=False)
    es, ei, _ = so.sequence_topk(sim, k, L, offsets, limit0=-exclusion, limit_step=1)

    def make():
        return dlc.SdavLoopClosureDetector(ds, patches=p, width=h, k=k, exclusion=exclusion, capacity=8, sequence=L, slopes=table_)

    def same(outs, what):
        s = torch.cat([o[0] for o in outs]).cpu().numpy()
        i = torch.cat([o[1] for o in outs]).cpu().numpy()
        assert np.array_equal(i, ei), what
        assert so.same_bits(s, es), what

    for batch in (1, 7, 32):
        det = make()
        same([det.query_and_insert(ds[lo:lo + batch]) for lo in range(0, n, batch)], batch)
        assert len(det) == n and det.stream.capacity >= n
    det, outs, f = make(), [], 0
    for b in (1, 2, 9, 1, 40, 3, n):                                   # mixed, shorter and longer than the context
        take = min(b, n - f)
        if take > 0:
            outs.append(det.query_and_insert(ds[f:f + take]))
            f += take
    same(outs, "mixed")
    det, outs, tickets = make(), [], []
    for lo in range(0, n, 16):                                         # two batches in flight
        tickets.append(det.submit(ds[lo:lo + 16]))
        if len(tickets) > 1:
            outs.append(det.result(tickets[-2]))
    outs.append(det.result(tickets[-1]))
    same(outs, "submit / result")
    if L == 4:
        assert int((ei[103:130, 0] == np.arange(23, 50)).sum()) == 27   # the revisit is found where its line fits
        assert (ei[:L - 1 + exclusion] == -1).all()
    # sequence=None is the detector as it was
    plain = dlc.SdavLoopClosureDetector(ds, patches=p, width=h, k=k, exclusion=exclusion, capacity=8)
    s0, i0 = plain.query_and_insert(ds)
    if L == 1:
        assert np.array_equal(i0.cpu().numpy(), ei) and so.same_bits(s0.cpu().numpy(), es)
    with pytest.raises(ValueError):
        dlc.SdavLoopClosureDetector(ds, patches=p, width=h, sequence=65)
    with pytest.raises(ValueError):
        dlc.SdavLoopClosureDetector(ds, patches=p, width=h, slopes=[[0]])


def test_detector_sequence_passes_the_poison_word(dlc):
    e = dlc.default_engine()
    g = torch.Generator(device=e.device)
    g.manual_seed(40)
    ds = torch.sigmoid(torch.randn((30, 6, 48), generator=g, device=e.device, dtype=torch.float64))
    det = dlc.SdavLoopClosureDetector(ds, patches=6, width=48, k=3, exclusion=2, sequence=3)
    s, i = det.query_and_insert(ds[:20])
    assert not bool(s.isnan().any()) and int(i.max()) >= 0
    bad = ds[20].clone()
    bad[1, 1] = 1.5
    s, i = det.query_and_insert(bad)
    assert bool(s.isnan().all()) and bool((i == -1).all())
    s, i = det.query_and_insert(ds[21:25])
    assert bool(s.isnan().all()) and bool((i == -1).all()) and int(det.poisoned) == 1
    with pytest.raises(RuntimeError):
        det.loops(s, i, 21)


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_similarity_metric_with_sequence(dlc):
    res = run_cli("--network", "sdav", "--metric", "similarity", "--sequence", "3", "--exclusion", "2", "--k", "2", "--batch", "4")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    loops = [l.split("\t") for l in res.stdout.splitlines() if l.startswith("loop\t")]
    assert loops and all(int(l[1]) - int(l[3]) > 2 and int(l[1]) >= 2 + 2 + 1 for l in loops)   # old enough, and a full line behind it
    for args in (("--network", "sdav", "--metric", "cosine", "--sequence", "3"),
                 ("--network", "cnn_vtl", "--metric", "distance", "--sequence", "3"),
                 ("--network", "cnn_vtl", "--metric", "similarity")):
        res = run_cli(*args)
        assert res.returncode == 2 and "error:" in res.stderr and "usage:" in res.stderr
