"""GPU k-nearest search by the cnn_vtl distance (dlc_cnnvtl_distance_topk), the key-frame database and the streaming
detector on top of it.  The reference: a stable argsort of oracle/distance.py distances (distance ascending, ties -> the
lower row), (-1, -1) past the rows a query sees.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def oracle_dist(q, db):
    """[Q, N] int64 distances through oracle.distance.bitwise_diff, a query at a time."""
    from oracle import distance as od
    q, db = np.asarray(q, np.int8), np.asarray(db, np.int8)
    out = np.empty((q.shape[0], db.shape[0]), dtype=np.int64)
    step = max(1, (1 << 24) // max(1, db.shape[1]))
    for r in range(q.shape[0]):
        for lo in range(0, db.shape[0], step):
            out[r, lo:lo + step] = od.bitwise_diff(q[r][None, :], db[lo:lo + step]).sum(axis=1)
    return out


def rank(dist, k, limits=None):
    """(dist [Q, k], idx [Q, k]) of a stable argsort per row over the first limits[r] columns; (-1, -1) padding."""
    q, n = dist.shape
    od, oi = np.full((q, k), -1, np.int64), np.full((q, k), -1, np.int64)
    for r in range(q):
        lr = n if limits is None else int(min(n, max(0, limits[r])))
        order = np.argsort(dist[r, :lr], kind="stable")[:k]
        od[r, :order.size], oi[r, :order.size] = dist[r, order], order
    return od, oi


def run(dlc, q, db, k, **kw):
    e = dlc.default_engine()
    d, i = e.cnnvtl_distance_topk(torch.as_tensor(q).to(e.device), torch.as_tensor(db).to(e.device), k, **kw)
    return d.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("name", ["n7_d2243", "n9_d37", "n3_d1"])
def test_topk_equals_the_reference_matrix(dlc, golden, name):
    z = golden("distance.npz")
    desc, matrix = z[name + "/desc"], z[name + "/matrix"]          # matrix: computed by the reference module itself
    n = desc.shape[0]
    for k in (1, 3, n, n + 2):
        d, i = run(dlc, desc, desc, k)
        ed, ei = rank(matrix, k)
        assert np.array_equal(d, ed) and np.array_equal(i, ei), (name, k)


# every value of each axis at least once: D, N (1, k - 1, k, 1 000, 70 001), Q (1, 7, 256, 300), k (1, 20, 128); then
# k = 63, 64, 65, where a list's last entry moves from a lane's first register to its second (the 16 x 256 tile, four
# slabs: the merge sees several lists)
SWEEP = [(1, 70001, 7, 20), (3, 1, 300, 128), (4, 19, 256, 20), (15, 128, 7, 128), (16, 1000, 300, 1), (63, 1000, 1, 128),
         (64, 70001, 1, 20), (65, 127, 300, 128), (2243, 1000, 256, 20), (2463, 20, 300, 20), (2463, 1000, 7, 1),
         (15, 70001, 256, 128), (2243, 127, 1, 128), (64, 1, 1, 1), (3, 1000, 256, 1),
         (17, 1000, 7, 63), (17, 1000, 7, 64), (17, 1000, 7, 65)]


@pytest.mark.parametrize("d,n,q,k", SWEEP)
def test_shape_sweep(dlc, d, n, q, k):
    rng = np.random.RandomState(d * 7 + n + q + k)
    db = rng.randint(-128, 128, size=(n, d)).astype(np.int8)
    qs = rng.randint(-128, 128, size=(q, d)).astype(np.int8)
    if n > 1:
        qs[: min(q, 3)] = db[rng.randint(0, n, size=min(q, 3))]      # exact matches (distance 0) among the queries
    got = run(dlc, qs, db, k)
    exp = rank(oracle_dist(qs, db), k)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_extremes_duplicates_and_ties(dlc):
    rng = np.random.RandomState(1)
    vals = np.array([-128, 127, -1, 0], dtype=np.int8)
    db = vals[rng.randint(0, 4, size=(3000, 77))]
    db[2000:2010] = db[5]                                              # duplicates of row 5: distance 0 to it, lower id first
    qs = np.concatenate([db[[5, 2003, 17]], vals[rng.randint(0, 4, size=(40, 77))]])
    for k in (1, 11, 128):
        got = run(dlc, qs, db, k)
        exp = rank(oracle_dist(qs, db), k)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    d, i = run(dlc, qs[:2], db, 11)
    assert list(i[0]) == [5] + list(range(2000, 2010)) and list(i[1]) == list(i[0]) and not d[:, :11].any()
    # every row equal: all distances tie, the ids are 0 .. k-1
    same = np.tile(vals[rng.randint(0, 4, size=(1, 2243))], (5000, 1))
    for q in (1, 7, 100):
        d, i = run(dlc, same[:q], same, 128)
        assert (i == np.arange(128)).all() and not d.any()


def test_padding_bytes_change_nothing(dlc):
    rng = np.random.RandomState(2)
    e = dlc.default_engine()
    for dd in (1, 13, 2243):
        ld = (dd + 15) // 16 * 16 + 16
        db = rng.randint(-128, 128, size=(4000, dd)).astype(np.int8)
        qs = rng.randint(-128, 128, size=(33, dd)).astype(np.int8)
        exp = rank(oracle_dist(qs, db), 20)
        pdb = rng.randint(-128, 128, size=(4000, ld)).astype(np.int8)     # garbage past dd
        pq = rng.randint(-128, 128, size=(33, ld)).astype(np.int8)
        pdb[:, :dd], pq[:, :dd] = db, qs
        d, i = e.cnnvtl_distance_topk(torch.from_numpy(pq).to(e.device), torch.from_numpy(pdb).to(e.device), 20, d=dd)
        assert np.array_equal(d.cpu().numpy(), exp[0]) and np.array_equal(i.cpu().numpy(), exp[1])


@pytest.mark.parametrize("limit0,step", [(0, 1), (-40, 1), (5, 1), (1500, 1), (2999, 0), (100, 3), (2000, -7), (-5, 0)])
def test_limits(dlc, limit0, step):
    rng = np.random.RandomState(3)
    db = rng.randint(-128, 128, size=(3000, 100)).astype(np.int8)
    qs = rng.randint(-128, 128, size=(300, 100)).astype(np.int8)
    lim = [limit0 + r * step for r in range(300)]
    dist = oracle_dist(qs, db)
    for k in (1, 20, 128):
        got = run(dlc, qs, db, k, limit0=limit0, limit_step=step)
        exp = rank(dist, k, lim)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (limit0, step, k)
    if limit0 == -40:                                                    # rows that see nothing, then fewer than k
        assert (got[1][:41] == -1).all() and (got[0][:41] == -1).all() and (got[1][41] >= 0).sum() == 1


def test_non_default_stream(dlc):
    rng = np.random.RandomState(4)
    e = dlc.default_engine()
    db = torch.from_numpy(rng.randint(-128, 128, size=(20000, 2243)).astype(np.int8)).to(e.device)
    qs = db[rng.randint(0, 20000, size=50)].clone()
    exp = run(dlc, qs, db, 20)
    s = torch.cuda.Stream(e.device)
    s.wait_stream(torch.cuda.current_stream(e.device))
    with torch.cuda.stream(s):
        for _ in range(3):
            d, i = e.cnnvtl_distance_topk(qs, db, 20)
    torch.cuda.current_stream(e.device).wait_stream(s)
    assert np.array_equal(d.cpu().numpy(), exp[0]) and np.array_equal(i.cpu().numpy(), exp[1])


def swar_dist(q, db):
    """[Q, N] distances by the word form (|x| = (x ^ m) + s per byte, then popcount), for the 1 M-row check."""
    d = q.shape[1]
    pad = (-d) % 8
    qw = np.pad(q, ((0, 0), (0, pad))).view(np.uint64)
    out = np.empty((q.shape[0], db.shape[0]), np.int64)
    ones = np.uint64(0x0101010101010101)
    for lo in range(0, db.shape[0], 50000):
        dw = np.pad(db[lo:lo + 50000], ((0, 0), (0, pad))).view(np.uint64)
        for r in range(q.shape[0]):
            w = qw[r][None, :] ^ dw
            s = (w >> np.uint64(7)) & ones
            a = (w ^ ((s << np.uint64(8)) - s)) + s
            out[r, lo:lo + 50000] = np.bitwise_count(a).sum(axis=1, dtype=np.int64)
    return out


def test_large_n_against_the_matrix_kernel_and_the_oracle(dlc):
    n, d, q, k = 1_000_000, 2243, 32, 20
    e = dlc.default_engine()
    g = torch.Generator(device=e.device).manual_seed(5)
    db = torch.randint(-128, 128, (n, d), dtype=torch.int8, device=e.device, generator=g)
    sel = torch.randint(0, n, (q,), device=e.device, generator=g)
    qs = db[sel].clone()
    qs[q // 2:] ^= torch.randint(0, 2, (q - q // 2, d), dtype=torch.int8, device=e.device, generator=g)  # near, not equal
    got_d, got_i = e.cnnvtl_distance_topk(qs, db, k)
    # the fixture-pinned matrix kernel over [queries; db chunk], ranked with a stable sort
    full = torch.empty((q, n), dtype=torch.int64, device=e.device)
    chunk = 16384
    for lo in range(0, n, chunk):
        m = e.cnnvtl_distance_matrix(torch.cat([qs, db[lo:lo + chunk]]))
        full[:, lo:lo + chunk] = m[:q, q:]
        del m
    sd, si = torch.sort(full, dim=1, stable=True)
    assert torch.equal(got_d, sd[:, :k]) and torch.equal(got_i, si[:, :k])
    # two queries in full against numpy: the word form, itself checked against oracle.distance on a sample first
    hq, hdb = qs[[0, q - 1]].cpu().numpy(), db.cpu().numpy()
    assert np.array_equal(swar_dist(hq, hdb[:3000]), oracle_dist(hq, hdb[:3000]))
    od, oi = rank(swar_dist(hq, hdb), k)
    assert np.array_equal(got_d[[0, q - 1]].cpu().numpy(), od) and np.array_equal(got_i[[0, q - 1]].cpu().numpy(), oi)


# ---- key-frame database and detector ----------------------------------------------------------------------------------
def revisiting_sequence(t, d, period, seed, flips=10):
    """int8 frames that return to each place every `period` frames, a few bytes changed per visit."""
    rng = np.random.RandomState(seed)
    places = rng.randint(-128, 128, size=(period, d)).astype(np.int8)
    x = places[np.arange(t) % period].copy()
    for f in range(t):
        x[f, rng.randint(0, d, size=flips)] = rng.randint(-128, 128, size=flips)
    return x


def stream_oracle(x, k, exclusion):
    """Per-frame loop: frame f against frames < f - exclusion."""
    dist = oracle_dist(x, x)
    return rank(dist, k, [f - exclusion for f in range(x.shape[0])])


@pytest.mark.parametrize("batch", [1, 7, 64, 300])
def test_detector_batching_invariance(dlc, batch):
    t, d, k, exclusion = 330, 203, 5, 10
    x = revisiting_sequence(t, d, 97, seed=7)
    det = dlc.CnnVtlLoopClosureDetector(d, k=k, exclusion=exclusion, capacity=16)
    outs = [det.query_and_insert(x[lo:lo + batch]) for lo in range(0, t, batch)]
    dd = torch.cat([o[0] for o in outs]).cpu().numpy()
    ii = torch.cat([o[1] for o in outs]).cpu().numpy()
    assert len(det) == t and det.db.capacity >= t             # grew from 16
    ed, ei = stream_oracle(x, k, exclusion)
    assert np.array_equal(dd, ed) and np.array_equal(ii, ei)
    # exclusion: nothing within `exclusion` frames, and the first frames see nothing at all
    f = np.arange(t)[:, None]
    assert ((ii < 0) | (ii < f - exclusion)).all() and (ii[:exclusion + 1] == -1).all()
    # a revisit finds its earlier visit first
    for g in range(97 + exclusion + 1, t):
        assert ii[g, 0] % 97 == g % 97


def test_detector_loops_filter(dlc):
    t, d = 200, 64
    x = revisiting_sequence(t, d, 50, seed=8, flips=4)
    det = dlc.CnnVtlLoopClosureDetector(d, k=3, max_distance=None, exclusion=5)
    dist, ids = det.query_and_insert(x)
    every = det.loops(dist, ids, 0)
    hd, hi = dist.cpu().numpy(), ids.cpu().numpy()
    assert len(every) == int((hi >= 0).sum())
    lim = int(np.median(hd[hi >= 0]))
    det.max_distance = lim
    some = det.loops(dist, ids, 0)
    assert some == [(f, m, dd) for f, m, dd in every if dd <= lim] and 0 < len(some) < len(every)
    assert all(isinstance(v, int) for e_ in some for v in e_)


def test_database_save_load_and_growth(dlc, tmp_path):
    rng = np.random.RandomState(9)
    x = rng.randint(-128, 128, size=(1000, 37)).astype(np.int8)
    db = dlc.CnnVtlKeyframeDatabase.empty(37, capacity=16)
    assert db.append(x[:10]) == (0, 10) and db.append(x[10:]) == (10, 1000)
    assert len(db) == 1000 and db.capacity >= 1000 and db.rows.shape == (1000, 48)
    assert np.array_equal(db.rows[:, :37].cpu().numpy(), x) and not db.rows[:, 37:].any()
    with pytest.raises(ValueError):
        db.append(np.zeros((2, 38), np.int8))
    q = rng.randint(-128, 128, size=(9, 37)).astype(np.int8)
    d0, i0 = db.nearest(q, 20)
    exp = rank(oracle_dist(q, x), 20)
    assert np.array_equal(d0.cpu().numpy(), exp[0]) and np.array_equal(i0.cpu().numpy(), exp[1])
    path = str(tmp_path / "kf.npz")
    db.save(path)
    assert str(np.load(path)["format"]) == "dlc-cnnvtl-keyframes-v1"
    back = dlc.CnnVtlKeyframeDatabase.load(path)
    assert len(back) == 1000 and back.dim == 37 and torch.equal(back.rows, db.rows)
    d1, i1 = back.nearest(q, 20)
    assert torch.equal(d0, d1) and torch.equal(i0, i1)
    pre = db.prefix(100)
    d2, i2 = pre.nearest(q, 20)
    exp = rank(oracle_dist(q, x[:100]), 20)
    assert np.array_equal(d2.cpu().numpy(), exp[0]) and np.array_equal(i2.cpu().numpy(), exp[1])
    from deeploopcloser_amd.distance import distance_topk
    dn, inn = distance_topk(q, x, 20)
    assert np.array_equal(dn, d0.cpu().numpy()) and np.array_equal(inn, i0.cpu().numpy())


def test_cli_distance_metric(dlc, capsys):
    import glob
    from deeploopcloser_amd import loop_closure
    from deeploopcloser_amd.distance import DistanceCalculator
    files = sorted(glob.glob(os.path.join(GOLDEN, "frames", "*.ppm")))
    rc = loop_closure.main([os.path.join(GOLDEN, "frames"), "--network", "cnn_vtl", "--metric", "distance", "--k", "2",
                            "--exclusion", "0", "--batch", "2"])
    out = capsys.readouterr().out.strip().splitlines()
    assert rc == 0 and all(l.startswith("loop\t") for l in out)
    got = [(int(l.split("\t")[1]), int(l.split("\t")[3]), int(l.split("\t")[5])) for l in out]
    # the same descriptors (one chunk: a frame's descriptor does not depend on its chunk), the reference's matrix
    desc = loop_closure.describe_cnn_vtl(files, as_int8=True)
    assert desc.dtype == torch.int8 and loop_closure.describe_cnn_vtl(files).dtype == torch.float32
    m = DistanceCalculator.distance_matrix(desc.cpu().numpy())
    ed, ei = rank(m, 2, [f for f in range(len(files))])
    exp = [(f, int(ei[f, c]), int(ed[f, c])) for f in range(len(files)) for c in range(2) if ei[f, c] >= 0]
    assert got == exp and len(exp) == 3
    rc = loop_closure.main([os.path.join(GOLDEN, "frames"), "--network", "cnn_vtl", "--metric", "distance", "--k", "2",
                            "--exclusion", "0", "--batch", "3", "--max-distance", str(min(d for _, _, d in exp))])
    out = capsys.readouterr().out.strip().splitlines()
    assert rc == 0 and len(out) == sum(1 for _, _, d in exp if d <= min(d for _, _, d in exp))
