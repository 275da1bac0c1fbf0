"""GPU cosine score rows (dlc_cosine_score_rows, Engine.cosine_score_rows, KeyframeDatabase.scores_f64 / score_keys) and
LoopClosureDetector(sequence=L) on top of them.  The reference: the NumPy restatement of the cosine path's score and key
(tests/cosine_rows_oracle.py, pinned by test_cosine_rows_cpu.py), the fp64 scores the top-k itself hands out, and for the
detector tests/sequence_oracle.py over the key matrix of the rows as stored.  Every comparison is exact (bit patterns)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cosine_rows_oracle as cro
import sequence_oracle as so

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def operand(e, values, dt, pad):
    """values [rows, d] as a stored [rows, d] view of a device tensor whose rows lie d + pad apart (pad a multiple of 8;
    the padding holds 3.0: read by nobody)."""
    rows, d = values.shape
    full = torch.full((rows, d + pad), 3.0, dtype=dt, device=e.device)
    full[:, :d] = torch.from_numpy(values).to(dt)
    return full[:, :d]


def sentinels(e, rows, ld):
    """(scores, keys) buffers [rows, ld] holding the sentinel word everywhere."""
    k = torch.full((rows, ld), SENTINEL, dtype=torch.int64, device=e.device)
    return k.clone().view(torch.float64), k


def words(t):
    return t.contiguous().view(torch.int64).cpu().numpy()


def with_specials(x):
    """+-0, subnormals of both stored types, one inf and one NaN element, in rows of their own where x has the rows."""
    x = x.copy()
    n = x.shape[0]
    if n > 0:
        x[0, 0], x[0, 1] = -0.0, 0.0
    if n > 1:
        x[1, 2], x[1, 3], x[1, 4] = 1e-40, 3e-6, -3e-6              # subnormal in bf16 (1e-40) and in fp16 (3e-6)
    if n > 4:
        x[3, 5] = np.inf
        x[4, 6] = np.nan
    return x


# ---- 1. bits ------------------------------------------------------------------------------------------------------------
# d: one piece; one 64-element step of the top-k's; 65 and 129 pieces (lanes without a piece in the last step); 8 full
# steps; 8 steps and 8 pieces.  (Q, n): the single-query kernel; one partial tile; several workgroups with ragged edges.
SHAPES = [(1, 1), (5, 7), (33, 130), (70, 300)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", [8, 64, 520, 1032, 4096, 4160])
def test_scores_and_keys_equal_the_restatement(dlc, d, dt):
    e = dlc.default_engine()
    rng = np.random.RandomState(d)
    for nq, n in SHAPES:
        db = operand(e, with_specials(0.1 * rng.standard_normal((n, d))), dt, 24)
        if (nq, n) == (33, 130):
            qs = db[60:93]                                           # queries that are db rows (and ldq = lddb)
        else:
            qs = operand(e, with_specials(0.1 * rng.standard_normal((nq, d))), dt, 8)
        s, k = sentinels(e, nq, n + 5)
        got = e.cosine_score_rows(qs, db, out=s[:, :n], out_keys=k[:, :n])
        assert got[0].data_ptr() == s.data_ptr() and got[1].data_ptr() == k.data_ptr()
        ref = cro.chain_scores(cro.as_f64(qs), cro.as_f64(db))
        assert so.same_bits(s[:, :n].cpu().numpy(), ref), (nq, n)
        assert np.array_equal(k[:, :n].cpu().numpy(), cro.f64_key(ref)), (nq, n)
        assert (words(s[:, n:]) == SENTINEL).all() and (words(k[:, n:]) == SENTINEL).all()
        if n > 4:
            assert np.isnan(ref[:, 4]).all() and (k[:, 4] == cro.INT64_MIN + 1).all()      # the NaN score maps to its key
            assert np.isinf(ref[:, 3]).any() or np.isnan(ref[:, 3]).all()
        # each output alone is the same output
        assert so.same_bits(e.cosine_score_rows(qs, db).cpu().numpy(), ref)
        assert np.array_equal(e.cosine_score_rows(qs, db, keys=True).cpu().numpy(), cro.f64_key(ref))


# ---- 2. the same number as the top-k ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_rows_are_the_topks_numbers(dlc, dt):
    rng = np.random.RandomState(11)
    x = rng.standard_normal((300, 200))
    x[150:160] = x[20:30] + 0.05 * rng.standard_normal((10, 200))
    xq = np.concatenate([x[25:30] + 0.02 * rng.standard_normal((5, 200)), rng.standard_normal((4, 200))])
    # n <= 128: the top-k with k = n hands out every row's fp64 score
    db = dlc.KeyframeDatabase(x[:100], dtype=dt)
    q = db.prepare_queries(xq)
    t = db.match_topk(q, 100, details=True)
    rows = db.scores_f64(q)
    assert bool((t.idx >= 0).all())
    assert torch.equal(rows.gather(1, t.idx).view(torch.int64), t.scores_f64.view(torch.int64))
    assert np.array_equal(t.idx.cpu().numpy(), cro.rank_by_key(db.score_keys(q).cpu().numpy(), 100))
    # n = 300, k = 20: the top-k's ids are the key rows' own ranking (key descending, then the lower index)
    db = dlc.KeyframeDatabase(x, dtype=dt)
    q = db.prepare_queries(xq)
    t = db.match_topk(q, 20, details=True)
    keys = db.score_keys(q)
    assert np.array_equal(t.idx.cpu().numpy(), cro.rank_by_key(keys.cpu().numpy(), 20))
    assert torch.equal(db.scores_f64(q).gather(1, t.idx).view(torch.int64), t.scores_f64.view(torch.int64))
    assert so.same_bits(db.scores_f64(q).cpu().numpy(), cro.chain_scores(cro.as_f64(q), cro.as_f64(db.rows)))


# ---- 3. a call writes only what it offers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def limited(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(2)
    nq, n, d = 33, 130, 72
    db = operand(e, 0.1 * rng.standard_normal((n, d)), torch.bfloat16, 8)
    qs = operand(e, 0.1 * rng.standard_normal((nq, d)), torch.bfloat16, 16)
    ref = cro.chain_scores(cro.as_f64(qs), cro.as_f64(db))
    return qs, db, ref.view(np.int64), cro.f64_key(ref)


@pytest.mark.parametrize("limit0,step", [(-4, 1), (0, 1), (120, 1), (7, 0), (133, 0), (136, -2), (20, -2), (130, -2)])
def test_limits_and_what_is_left_alone(dlc, limited, limit0, step):
    e = dlc.default_engine()
    qs, db, ref_words, ref_keys = limited
    nq, n = ref_keys.shape
    offered = np.pad(cro.offered(nq, n, limit0, step), ((0, 0), (0, 9)))
    assert offered.any() and not offered.all()
    s, k = sentinels(e, nq, n + 9)
    e.cosine_score_rows(qs, db, limit0=limit0, limit_step=step, out=s[:, :n], out_keys=k[:, :n])
    assert np.array_equal(words(s), np.where(offered, np.pad(ref_words, ((0, 0), (0, 9))), SENTINEL))
    assert np.array_equal(k.cpu().numpy(), np.where(offered, np.pad(ref_keys, ((0, 0), (0, 9))), SENTINEL))
    # where the engine allocates, the cells not offered are NaN / INT64_MIN
    got = e.cosine_score_rows(qs, db, limit0=limit0, limit_step=step, keys=True)
    assert np.array_equal(got.cpu().numpy(), np.where(offered[:, :n], ref_keys, cro.INT64_MIN))
    got = e.cosine_score_rows(qs, db, limit0=limit0, limit_step=step).cpu().numpy()
    assert np.isnan(got[~offered[:, :n]]).all() and np.array_equal(got.view(np.int64)[offered[:, :n]], ref_words[offered[:, :n]])


@pytest.mark.parametrize("limit0,step", [(0, 0), (-5, 0), (-32, 1), (0, -1), (0, -2 ** 40), (-2 ** 40, 2 ** 30)])
def test_a_call_that_offers_nothing_touches_nothing(dlc, limited, limit0, step):
    e = dlc.default_engine()
    qs, db, _, ref_keys = limited
    nq, n = ref_keys.shape
    assert not cro.offered(nq, n, limit0, step).any()
    s, k = sentinels(e, nq, n)
    rc = e.lib.dlc_cosine_score_rows(e.ctx, 0, C.c_void_p(qs.data_ptr()), nq, qs.stride(0), C.c_void_p(db.data_ptr()), n,
                                     db.stride(0), qs.shape[1], limit0, step, C.c_void_p(s.data_ptr()),
                                     C.c_void_p(k.data_ptr()), n, e._stream())
    assert rc == 0
    assert (words(s) == SENTINEL).all() and (words(k) == SENTINEL).all()


# ---- 4. batching --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_a_row_does_not_depend_on_its_batch(dlc, dt):
    e = dlc.default_engine()
    rng = np.random.RandomState(8)
    db = operand(e, 0.1 * rng.standard_normal((150, 520)), dt, 8)
    qs = operand(e, 0.1 * rng.standard_normal((70, 520)), dt, 8)
    s70, k70 = e.cosine_score_rows(qs, db, out=torch.empty((70, 150), dtype=torch.float64, device=e.device), keys=True)
    for at in (3, 6):                                                # a batch of 7: both of its query tiles
        s7, k7 = e.cosine_score_rows(qs[:7], db, out=torch.empty((7, 150), dtype=torch.float64, device=e.device), keys=True)
        s1, k1 = e.cosine_score_rows(qs[at:at + 1], db, out=torch.empty((1, 150), dtype=torch.float64, device=e.device),
                                     keys=True)
        assert torch.equal(s1.view(torch.int64), s7[at:at + 1].view(torch.int64))
        assert torch.equal(s1.view(torch.int64), s70[at:at + 1].view(torch.int64))
        assert torch.equal(k1, k7[at:at + 1]) and torch.equal(k1, k70[at:at + 1])
    s1 = e.cosine_score_rows(qs[69:70], db)
    assert torch.equal(s1.view(torch.int64), s70[69:70].view(torch.int64))
    # ... nor on the limits of the call
    lim = e.cosine_score_rows(qs, db, limit0=100, limit_step=-1)
    seen = torch.arange(150, device=e.device)[None, :] < (100 - torch.arange(70, device=e.device))[:, None]
    assert torch.equal(lim.view(torch.int64)[seen], s70.view(torch.int64)[seen]) and bool(lim[~seen].isnan().all())


# ---- 5. bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    db = torch.zeros((50, 32), dtype=torch.bfloat16, device=e.device)
    qs = torch.zeros((4, 32), dtype=torch.bfloat16, device=e.device)
    s, k = sentinels(e, 4, 50)
    vp = lambda t, off=0: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + off)

    def c_call(dtype=_lib.DLC_BF16, qp=vp(qs), ldq=32, dbp=vp(db), ldd=32, d=32, o_s=s, o_k=k, ld_out=50, nq=4, n=50):
        return e.lib.dlc_cosine_score_rows(e.ctx, dtype, qp, nq, ldq, dbp, n, ldd, d, 50, 0, vp(o_s), vp(o_k), ld_out,
                                           e._stream())
    for kw in (dict(o_s=None, o_k=None), dict(dtype=_lib.DLC_F32), dict(dtype=_lib.DLC_I8), dict(d=12), dict(d=4),
               dict(ld_out=49), dict(qp=vp(qs, 2), d=16), dict(dbp=vp(db, 8), d=16), dict(ldq=20, d=16), dict(ldd=36),
               dict(ldq=24), dict(d=0), dict(nq=0), dict(n=0), dict(qp=vp(None)), dict(dbp=vp(None))):
        rc = c_call(**kw)
        assert rc == _lib.DLC_ERR_BAD_ARG, kw
        with pytest.raises(ValueError):
            e._check(rc)
    torch.cuda.synchronize()
    assert (words(s) == SENTINEL).all() and (words(k) == SENTINEL).all()      # the refused calls wrote nothing
    assert c_call() == _lib.DLC_OK and c_call(o_s=None) == _lib.DLC_OK and c_call(o_k=None) == _lib.DLC_OK
    assert not bool(s.any()) and not bool(k.any())                            # zeros . zeros
    # the Python entry
    good = e.cosine_score_rows(qs, db)
    assert good.shape == (4, 50) and good.dtype == torch.float64
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=e.device)
    bad = [lambda: e.cosine_score_rows(qs.float(), db.float()),
           lambda: e.cosine_score_rows(qs.to(torch.float16), db),                            # two dtypes
           lambda: e.cosine_score_rows(qs[:, :16], db),                                      # widths differ
           lambda: e.cosine_score_rows(qs[0], db),
           lambda: e.cosine_score_rows(qs.cpu(), db),
           lambda: e.cosine_score_rows(qs[:, ::2], db[:, ::2]),
           lambda: e.cosine_score_rows(qs[:, :12], db[:, :12]),                              # d not a multiple of 8
           lambda: e.cosine_score_rows(qs, db, out=f64(5, 50)),
           lambda: e.cosine_score_rows(qs, db, out=f64(4, 50).float()),
           lambda: e.cosine_score_rows(qs, db, out=f64(4, 49)),                              # narrower than n
           lambda: e.cosine_score_rows(qs, db, out=f64(4, 100)[:, ::2]),
           lambda: e.cosine_score_rows(qs, db, out=f64(4, 50).cpu()),
           lambda: e.cosine_score_rows(qs, db, out_keys=f64(4, 50)),                         # keys are int64
           lambda: e.cosine_score_rows(qs, db, out=f64(4, 60)[:, :50], out_keys=k)]          # two row strides
    for call in bad:
        with pytest.raises((ValueError, RuntimeError)):
            call()


# ---- 6. the database's entry points -------------------------------------------------------------------------------------
def test_database_rows(dlc):
    rng = np.random.RandomState(9)
    x, xq = rng.standard_normal((40, 100)), rng.standard_normal((6, 100))
    db = dlc.KeyframeDatabase.empty(100, capacity=16, dtype="f16")
    db.append(x[:10])
    db.append(x[10:])                                                  # grown from 16
    q = db.prepare_queries(xq)
    ref = cro.chain_scores(cro.as_f64(q), cro.as_f64(db.rows))
    s = db.scores_f64(xq)                                              # floats in: normalised as the rows were
    assert s.dtype == torch.float64 and s.device == db.engine.device and so.same_bits(s.cpu().numpy(), ref)
    k = db.score_keys(q, limit0=36, limit_step=2)
    assert k.dtype == torch.int64
    assert np.array_equal(k.cpu().numpy(), np.where(cro.offered(6, 40, 36, 2), cro.f64_key(ref), cro.INT64_MIN))
    own = db.scores_f64(db.rows[5:9])                                  # stored rows as queries
    assert so.same_bits(own.cpu().numpy(), cro.chain_scores(cro.as_f64(db.rows[5:9]), cro.as_f64(db.rows)))
    keep = torch.full((6, 48), -3, dtype=torch.int64, device=db.engine.device)
    assert db.score_keys(q, limit0=0, limit_step=9, out=keep[:, :40]).data_ptr() == keep.data_ptr()
    assert np.array_equal(keep[:, :40].cpu().numpy(), np.where(cro.offered(6, 40, 0, 9), cro.f64_key(ref), -3))
    assert bool((keep[:, 40:] == -3).all())


# ---- 7. the detector with sequence=L ------------------------------------------------------------------------------------
def stream(det, x, batches):
    """The frames of x through det in batches of the given sizes (the last size repeats); the lists of all frames."""
    outs, f = [], 0
    sizes = list(batches)
    while f < x.shape[0]:
        b = sizes.pop(0) if len(sizes) > 1 else sizes[0]
        outs.append(det.query_and_insert(x[f:f + b]))
        f += min(b, x.shape[0] - f)
    return torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_detector_with_sequence(dlc, dt):
    rng = np.random.RandomState(5)
    n, dim, K, EXCLUSION, L = 90, 64, 5, 3, 4
    x = rng.standard_normal((n, dim))
    x[60:80] = x[10:30] + 0.5 * rng.standard_normal((20, dim))       # a revisit, so that the lists are not all noise
    results = []
    for batches in ([1], [7], [32], [1, 2, 9, 1, 40, 3, n]):             # mixed: shorter and longer than the context
        det = dlc.LoopClosureDetector(dim, k=K, exclusion=EXCLUSION, sequence=L, capacity=16, dtype=dt)
        s, i = stream(det, x, batches)
        assert len(det) == n and det.db.capacity >= n                  # grew from 16
        assert s.dtype == np.float64 and i.dtype == np.int64
        results.append((s, i))
    # the oracle over the key matrix of the rows as stored
    rows = cro.as_f64(det.db.rows)
    keys = cro.f64_key(cro.chain_scores(rows, rows))
    es, ei, _ = so.sequence_topk(keys, K, L, dlc.slope_offsets(L), limit0=-EXCLUSION, limit_step=1)
    es = np.where(ei >= 0, es.astype(np.float64) * 2.0 ** -40, -np.inf)
    assert (ei[:L - 1 + EXCLUSION] == -1).all() and (ei[L - 1 + EXCLUSION + K:] >= 0).all()
    for s, i in results:
        assert np.array_equal(i, ei) and np.array_equal(s, es)
    assert int((ei[63:80, 0] == np.arange(13, 30)).sum()) == 17       # the revisit is found


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_sequence_of_one_is_the_detector_without(dlc, dt):
    rng = np.random.RandomState(6)
    n, dim = 90, 64
    x = rng.standard_normal((n, dim))
    x[70:75] = x[40:45]                                                # exact ties between distinct frames
    x[50:60] = x[5:15] + 0.3 * rng.standard_normal((10, dim))
    s0, i0 = stream(dlc.LoopClosureDetector(dim, k=5, exclusion=3, capacity=16, dtype=dt), x, [7])
    s1, i1 = stream(dlc.LoopClosureDetector(dim, k=5, exclusion=3, capacity=16, dtype=dt, sequence=1), x, [7])
    assert s0.dtype == np.float32 and s1.dtype == np.float64
    assert np.array_equal(i1, i0)
    assert np.array_equal(s1.astype(np.float32), s0)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_planted_revisit_on_the_detector(dlc, dt):
    x, true, alias = cro.planted_revisit_float(dim=64)
    _, i0 = stream(dlc.LoopClosureDetector(64, k=1, exclusion=30, capacity=64, dtype=dt), x, [32])
    assert int((i0[200:260, 0] == alias).sum()) == 60
    det = dlc.LoopClosureDetector(64, k=1, exclusion=30, capacity=64, dtype=dt, sequence=10)
    s, i = stream(det, x, [32])
    assert i[209:260, 0].size == 51 and int((i[209:260, 0] == true[9:]).sum()) == 51
    # loops(): the threshold is compared with the SUM of the L scores -- a mean of 0.5 is threshold = 0.5 * 10
    det.threshold = 0.5 * 10
    found = det.loops(torch.from_numpy(s), torch.from_numpy(i), 0)
    assert found == [(f, int(i[f, 0]), float(s[f, 0])) for f in range(260) if i[f, 0] >= 0 and s[f, 0] >= 5.0]
    assert {f for f, _, _ in found} >= set(range(209, 260))
