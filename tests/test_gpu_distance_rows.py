"""GPU rectangular cnn_vtl distance (dlc_cnnvtl_distance_rows, Engine.cnnvtl_distance_rows, CnnVtlKeyframeDatabase.distances,
DistanceCalculator.distance_rows) and CnnVtlLoopClosureDetector(sequence=L) on top of it.  The reference: oracle/distance.py
summed per pair (tests/distance_rows_oracle.py), the reference-made matrices of tests/golden/distance.npz and, for the
detector, tests/sequence_oracle.py over oracle.distance.distance_matrix.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import distance_rows_oracle as dro
import sequence_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def run(dlc, q, db, **kw):
    e = dlc.default_engine()
    return e.cnnvtl_distance_rows(torch.as_tensor(q).to(e.device), torch.as_tensor(db).to(e.device), **kw).cpu().numpy()


# ---- 1. the reference's own matrices ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n7_d2243", "n9_d37", "n3_d1"])
def test_rows_equal_the_reference_matrix(dlc, golden, name):
    z = golden("distance.npz")
    desc, matrix = z[name + "/desc"], z[name + "/matrix"]          # matrix: computed by the reference module itself
    got = run(dlc, desc, desc)
    assert got.dtype == np.int64 and np.array_equal(got, matrix)
    assert np.array_equal(run(dlc, desc[[2, 0]], desc), matrix[[2, 0]])


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------
# every value of each axis at least once: D (below, at and above the 16-byte load and the 64-byte step), N (both db tile
# widths +- 1, several tiles), Q (each tile plan -- 1 x 256 up to 4, 16 x 256, 64 x 64 -- and its edges)
SWEEP = [(1, 1, 1), (15, 63, 4), (16, 64, 5), (17, 65, 16), (63, 255, 17), (64, 256, 64), (65, 257, 65), (130, 1000, 130),
         (2243, 1000, 17), (2243, 257, 1), (64, 1000, 4), (1, 1000, 64), (130, 63, 65), (17, 256, 130)]


def test_sweep_covers_every_axis_value():
    assert {s[0] for s in SWEEP} == {1, 15, 16, 17, 63, 64, 65, 130, 2243}
    assert {s[1] for s in SWEEP} == {1, 63, 64, 65, 255, 256, 257, 1000}
    assert {s[2] for s in SWEEP} == {1, 4, 5, 16, 17, 64, 65, 130}


@pytest.mark.parametrize("d,n,q", SWEEP)
def test_shape_sweep(dlc, d, n, q):
    rng = np.random.RandomState(d * 7 + n * 3 + q)
    db, qs = dro.random_bytes(rng, (n, d)), dro.random_bytes(rng, (q, d))
    qs[0] = db[rng.randint(0, n)]                                      # an exact match (distance 0) among the queries
    got = run(dlc, qs, db)
    assert got.shape == (q, n) and np.array_equal(got, dro.distance_rows(qs, db))


def test_more_db_tiles_than_one_grid_row(dlc):
    """Past 65 536 db tiles a workgroup walks several of them (the grid's x extent is capped): 256-row tiles at Q = 1
    against the oracle, 64-row tiles at Q = 64 against the same call on slices of the db that stay below the cap."""
    e = dlc.default_engine()
    rng = np.random.RandomState(21)
    n = 256 * 65536 + 300
    db = dro.random_bytes(rng, (n, 1))
    q = np.array([[-128]], dtype=np.int8)
    got = run(dlc, q, db, limit0=n - 7)
    exp = dro.distance_rows(q, db)
    exp[0, n - 7:] = -1
    assert np.array_equal(got, exp)
    n = 64 * 65536 + 100
    dev = e._rows16(torch.from_numpy(db[:n]).to(e.device), 1)
    qs = dev[rng.randint(0, n, size=64)].clone()
    whole = e.cnnvtl_distance_rows(qs, dev, d=1)
    for lo in range(0, n, 1 << 21):
        assert torch.equal(whole[:, lo:lo + (1 << 21)], e.cnnvtl_distance_rows(qs, dev[lo:lo + (1 << 21)], d=1)), lo
    assert np.array_equal(whole[:2].cpu().numpy(), dro.distance_rows(qs[:2, :1].cpu().numpy(), db[:n]))


# ---- 3. limits, and what is left alone ----------------------------------------------------------------------------------
LIMIT_N, LIMIT_D, LIMIT_PAD = 300, 37, 5


@pytest.fixture(scope="module")
def limit_case():
    rng = np.random.RandomState(11)
    db, qs = dro.random_bytes(rng, (LIMIT_N, LIMIT_D)), dro.random_bytes(rng, (70, LIMIT_D))
    return db, qs, dro.distance_rows(qs, db)


@pytest.mark.parametrize("q", [70, 3])
@pytest.mark.parametrize("limit0,step", [(LIMIT_N, 0), (0, 1), (-30, 1), (5, 3), (LIMIT_N + 10, -7), (-5, 0)])
def test_limits_and_untouched_words(dlc, limit_case, q, limit0, step):
    e = dlc.default_engine()
    db, qs, dist = limit_case
    qs, dist, n = qs[:q], dist[:q], LIMIT_N
    # a sentinel no distance can equal, different in every word
    sentinel = -(np.arange(q * (n + LIMIT_PAD), dtype=np.int64).reshape(q, n + LIMIT_PAD) * 2654435761 + 12345)
    buf = torch.from_numpy(sentinel.copy()).to(e.device)
    out = e.cnnvtl_distance_rows(torch.from_numpy(qs).to(e.device), torch.from_numpy(db).to(e.device),
                                 limit0=limit0, limit_step=step, out=buf[:, :n])
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    offered = np.zeros((q, n + LIMIT_PAD), bool)
    offered[:, :n] = dro.offered(q, n, limit0, step)
    assert np.array_equal(got[offered], dist[offered[:, :n]])
    assert np.array_equal(got[~offered], sentinel[~offered])
    if limit0 == -5:
        assert not offered.any()                                       # the all-empty case: returned normally, nothing written
    # allocated by the engine: -1 where a cell is not offered
    fresh = run(dlc, qs, db, limit0=limit0, limit_step=step)
    assert np.array_equal(fresh, np.where(offered[:, :n], dist, -1))


# ---- 4. padding and aliasing --------------------------------------------------------------------------------------------
def test_padding_bytes_change_nothing_and_queries_may_be_db_rows(dlc):
    rng = np.random.RandomState(2)
    e = dlc.default_engine()
    for dd in (1, 13, 2243):
        ld = (dd + 15) // 16 * 16 + 16
        db, qs = dro.random_bytes(rng, (300, dd)), dro.random_bytes(rng, (33, dd))
        pdb = rng.randint(-128, 128, size=(300, ld)).astype(np.int8)     # garbage past dd
        pq = rng.randint(-128, 128, size=(33, ld)).astype(np.int8)
        pdb[:, :dd], pq[:, :dd] = db, qs
        got = e.cnnvtl_distance_rows(torch.from_numpy(pq).to(e.device), torch.from_numpy(pdb).to(e.device), d=dd)
        assert np.array_equal(got.cpu().numpy(), dro.distance_rows(qs, db))
        # queries that ARE rows of db (a row slice of the same tensor)
        dev = torch.from_numpy(pdb).to(e.device)
        own = e.cnnvtl_distance_rows(dev[100:133], dev, d=dd)
        assert own.data_ptr() != dev.data_ptr()
        assert np.array_equal(own.cpu().numpy(), dro.distance_rows(db[100:133], db))
        assert torch.equal(own, e.cnnvtl_distance_rows(dev[100:133].clone(), dev, d=dd))


# ---- 5. the existing kernels --------------------------------------------------------------------------------------------
def test_agreement_with_the_matrix_and_the_topk_kernels(dlc):
    q, n, d, k = 33, 700, 2243, 20
    e = dlc.default_engine()
    g = torch.Generator(device=e.device).manual_seed(5)
    db = torch.randint(-128, 128, (n, d), dtype=torch.int8, device=e.device, generator=g)
    qs = db[torch.randint(0, n, (q,), device=e.device, generator=g)].clone()
    qs[q // 2:] ^= torch.randint(0, 2, (q - q // 2, d), dtype=torch.int8, device=e.device, generator=g)   # near, not equal
    rows = e.cnnvtl_distance_rows(qs, db)
    m = e.cnnvtl_distance_matrix(torch.cat([db, qs]))
    assert torch.equal(rows, m[n:, :n])
    sd, si = torch.sort(rows, dim=1, stable=True)
    td, ti = e.cnnvtl_distance_topk(qs, db, k)
    assert torch.equal(sd[:, :k], td) and torch.equal(si[:, :k], ti)
    # a streamed batch's limits: the cells not offered sort last and become (-1, -1)
    lim = e.cnnvtl_distance_rows(qs, db, limit0=-30, limit_step=1)
    big = torch.iinfo(torch.int64).max
    sd, si = torch.sort(torch.where(lim < 0, big, lim), dim=1, stable=True)
    sd, si = sd[:, :k], si[:, :k]
    empty = sd == big
    td, ti = e.cnnvtl_distance_topk(qs, db, k, limit0=-30, limit_step=1)
    assert torch.equal(torch.where(empty, -1, sd), td) and torch.equal(torch.where(empty, -1, si), ti)
    assert bool(empty[:31].all()) and int((~empty[32]).sum()) == 2


# ---- 6. stream and bad arguments ----------------------------------------------------------------------------------------
def test_non_default_stream(dlc):
    rng = np.random.RandomState(4)
    e = dlc.default_engine()
    db = torch.from_numpy(dro.random_bytes(rng, (2000, 203))).to(e.device)
    qs = db[rng.randint(0, 2000, size=50)].clone()
    exp = e.cnnvtl_distance_rows(qs, db)
    s = torch.cuda.Stream(e.device)
    s.wait_stream(torch.cuda.current_stream(e.device))
    with torch.cuda.stream(s):
        for _ in range(3):
            got = e.cnnvtl_distance_rows(qs, db)
    torch.cuda.current_stream(e.device).wait_stream(s)
    assert torch.equal(got, exp)
    assert np.array_equal(exp.cpu().numpy(), dro.distance_rows(qs.cpu().numpy(), db.cpu().numpy()))


def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    db = torch.zeros((50, 32), dtype=torch.int8, device=e.device)
    qs = torch.zeros((4, 32), dtype=torch.int8, device=e.device)
    e.cnnvtl_distance_rows(qs, db)
    bad = [lambda: e.cnnvtl_distance_rows(qs.float(), db),                                  # dtype
           lambda: e.cnnvtl_distance_rows(qs, db.to(torch.uint8)),
           lambda: e.cnnvtl_distance_rows(qs[:, :16], db),                                  # widths differ
           lambda: e.cnnvtl_distance_rows(qs, db, d=33),                                    # d wider than the rows
           lambda: e.cnnvtl_distance_rows(qs[0], db),
           lambda: e.cnnvtl_distance_rows(qs.cpu(), db),
           lambda: e.cnnvtl_distance_rows(qs, db, out=torch.zeros((5, 50), dtype=torch.int64, device=e.device)),
           lambda: e.cnnvtl_distance_rows(qs, db, out=torch.zeros((4, 50), dtype=torch.int32, device=e.device)),
           lambda: e.cnnvtl_distance_rows(qs, db, out=torch.zeros((4, 49), dtype=torch.int64, device=e.device)),   # narrower than N
           lambda: e.cnnvtl_distance_rows(qs, db, out=torch.zeros((4, 100), dtype=torch.int64, device=e.device)[:, ::2]),
           lambda: e.cnnvtl_distance_rows(qs, db, out=torch.zeros((4, 50), dtype=torch.int64))]
    for call in bad:
        with pytest.raises((ValueError, RuntimeError)):
            call()
    # the C level: a misaligned base, a misaligned stride, ld_out < N -- refused before any launch
    out = torch.full((4, 50), -7, dtype=torch.int64, device=e.device)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def c_call(qp=vp(qs), ldq=32, dbp=vp(db), ldd=32, d=32, ld_out=50):
        return e.lib.dlc_cnnvtl_distance_rows(e.ctx, qp, 4, ldq, dbp, 50, ldd, d, 50, 0, vp(out), ld_out, e._stream())
    assert c_call() == _lib.DLC_OK
    for kw in (dict(qp=vp(qs, 1), d=16), dict(dbp=vp(db, 8), d=16), dict(ldq=24, d=16), dict(ldd=40), dict(ld_out=49),
               dict(d=0), dict(d=33)):
        rc = c_call(**kw)
        assert rc == _lib.DLC_ERR_BAD_ARG, kw
        with pytest.raises(ValueError):
            e._check(rc)
    for rows in ((1 << 20) + 1, 1 << 22):                             # Q > 2^20, as the header states it (refused before any read)
        assert e.lib.dlc_cnnvtl_distance_rows(e.ctx, vp(qs), rows, 32, vp(db), 50, 32, 32, 50, 0, vp(out), 50,
                                              e._stream()) == _lib.DLC_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert not bool(out.any())                                       # the one good call wrote zeros; the refused ones nothing


# ---- 7. the Python entry points -----------------------------------------------------------------------------------------
def test_database_distances_and_calculator_rows(dlc):
    rng = np.random.RandomState(9)
    x, q = dro.random_bytes(rng, (400, 37)), dro.random_bytes(rng, (9, 37))
    dist = dro.distance_rows(q, x)
    got = dlc.DistanceCalculator.distance_rows(q, x)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, dist)
    assert np.array_equal(dlc.DistanceCalculator.distance_rows(q.tolist(), x.tolist()), dist)
    with pytest.raises(ValueError):
        dlc.DistanceCalculator.distance_rows(q[:, :30], x)
    db = dlc.CnnVtlKeyframeDatabase.empty(37, capacity=16)
    db.append(x[:10])
    db.append(x[10:])                                                  # grown from 16
    rows = db.distances(q)                                             # NumPy in, rows on the device
    assert rows.dtype == torch.int64 and rows.device == db.engine.device and np.array_equal(rows.cpu().numpy(), dist)
    assert np.array_equal(db.distances(q[0]).cpu().numpy(), dist[:1])
    lim = db.distances(q, limit0=395, limit_step=2).cpu().numpy()      # -1 where a cell is not offered
    assert np.array_equal(lim, np.where(dro.offered(9, 400, 395, 2), dist, -1)) and (lim == -1).any()
    own = db.distances(db.rows[100:120])                               # stored rows, padding included, as queries
    assert np.array_equal(own.cpu().numpy(), dro.distance_rows(x[100:120], x))
    keep = torch.full((9, 410), -3, dtype=torch.int64, device=db.engine.device)
    assert db.distances(q, limit0=0, limit_step=50, out=keep[:, :400]).data_ptr() == keep.data_ptr()
    assert np.array_equal(keep[:, :400].cpu().numpy(), np.where(dro.offered(9, 400, 0, 50), dist, -3))
    assert bool((keep[:, 400:] == -3).all())
    with pytest.raises(ValueError):
        db.distances(np.zeros((2, 38), np.int8))


# ---- 8. the detector with sequence=L ------------------------------------------------------------------------------------
K, EXCLUSION = 4, 30
WIDE = np.array([[0, 0, 1, 1, 2, 2], [0, 1, 2, 3, 4, 5], [0, 2, 4, 6, 8, 10]], dtype=np.int32)


@pytest.fixture(scope="module")
def revisit():
    from oracle import distance as od
    x, true, alias = so.planted_revisit()
    assert x.shape == (260, 64)
    return x, true, alias, od.distance_matrix(x)


def stream(det, x, batches):
    """The frames of x through det in batches of the given sizes (the last size repeats); the lists of all frames."""
    outs, f = [], 0
    sizes = list(batches)
    while f < x.shape[0]:
        b = sizes.pop(0) if len(sizes) > 1 else sizes[0]
        outs.append(det.query_and_insert(x[f:f + b]))
        f += min(b, x.shape[0] - f)
    return torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy()


@pytest.mark.parametrize("L,slopes", [(1, None), (10, None), (6, WIDE)])
def test_detector_with_sequence(dlc, revisit, L, slopes):
    x, true, alias, dist = revisit
    n = x.shape[0]
    offsets = dlc.slope_offsets(L) if slopes is None else slopes
    es, ei, _ = so.sequence_topk(dist, K, L, offsets, limit0=-EXCLUSION, limit_step=1, lower_is_better=True)

    def make(**kw):
        return dlc.CnnVtlLoopClosureDetector(64, k=K, exclusion=EXCLUSION, capacity=8, **kw)

    # the lists do not depend on the batching and equal the oracle's over the matrix of all frames
    for batches in ([1], [7], [32], [1, 2, 9, 1, 40, 3, n]):                # mixed: shorter and longer than the context
        det = make(sequence=L, slopes=slopes)
        s, i = stream(det, x, batches)
        assert len(det) == n and det.db.capacity >= n                      # grew from 8
        assert s.dtype == np.int64 and np.array_equal(i, ei) and np.array_equal(s, es), batches
    assert (ei[:L - 1 + EXCLUSION] == -1).all() and (es[:L - 1 + EXCLUSION] == -1).all()
    # sequence=None is the detector as it was: the fused top-k, and what a single frame's nearest neighbour says
    d0, i0 = stream(make(), x, [32])
    assert int((i0[200:260, 0] == true).sum()) == 0 and np.array_equal(i0[200:260, 0], alias)
    if L == 1:
        assert np.array_equal(i0, ei) and np.array_equal(d0, es)
    if L == 10:
        assert ei[209:260, 0].size == 51 and int((ei[209:260, 0] == true[9:]).sum()) == 51
        # loops(): a max_distance between the true matches' sums and the best of everything else keeps the true matches only
        is_true = np.zeros(es.shape, bool)
        is_true[209:260, 0] = True
        top, rest = int(es[is_true].max()), int(es[(ei >= 0) & ~is_true].min())
        assert top < rest
        det = make(sequence=L, max_distance=(top + rest) // 2)
        found = []
        for lo in range(0, n, 32):
            found += det.loops(*det.query_and_insert(x[lo:lo + 32]), lo)
        assert found == [(f, int(true[f - 200]), int(es[f, 0])) for f in range(209, 260)]
        det.max_distance = None
        assert len(det.loops(torch.from_numpy(es), torch.from_numpy(ei), 0)) == int((ei >= 0).sum())
