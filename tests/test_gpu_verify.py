"""GPU geometric verification (dlc_verify_pairs through the raw C ABI; Engine.verify_pairs, GeometricVerifier and the CLI on
top) against the NumPy / Python-int restatement of the definition (tests/verify_oracle.py, pinned by test_verify_cpu.py).
The definition fixes every rounding and the geometry is integer, so every comparison is `==` on integers or on the int64
views of the doubles: zero tolerance.  Inputs carry NaN-filled padding columns that would poison every distance if they
were read; outputs sit in sentinel-filled buffers wider than what may be written; candidate tables have a pitch larger
than k."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import real_frames
import verify_oracle as vfo

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A
SIM, TRANS = vfo.SIMILARITY, vfo.TRANSLATION


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def e(dlc):
    return dlc.default_engine()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def padded(e, m, pad):
    """m [frames, P, H] as the first H columns of a [frames * P, H + pad] device matrix whose other columns are NaN."""
    m = np.ascontiguousarray(m).reshape(-1, m.shape[-1])
    buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=torch.float64, device=e.device)
    buf[:, :m.shape[1]] = torch.from_numpy(m).to(e.device)
    return buf


def raw_verify(e, qd, qp, dd, dp, cand, model=SIM, tol=3, S=32, mutual=1, full=True, pads=(3, 1), cand_pad=2):
    """dlc_verify_pairs over qd [Q, P, H], qp [Q, P, 2], dd [N, P, H], dp [N, P, 2], cand [Q, k] into sentinel-framed
    outputs -> dict of host arrays: inliers, n_matches [Q, k]; with full: hyp [Q, k, 2], mask [Q, k] (uint64), match
    [Q, k, P], dist words int64 [Q, k, P, P] (the sentinel where a pair's slot was left alone)."""
    Q, P, H = qd.shape
    N, k = dd.shape[0], cand.shape[1]
    qb, db = padded(e, qd, pads[0]), padded(e, dd, pads[1])
    qpt = torch.from_numpy(np.ascontiguousarray(qp, dtype=np.int32)).to(e.device)
    dpt = torch.from_numpy(np.ascontiguousarray(dp, dtype=np.int32)).to(e.device)
    ct = torch.full((Q, k + cand_pad), 99, dtype=torch.int64, device=e.device)
    ct[:, :k] = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int64)).to(e.device)
    pairs = Q * k
    i32 = lambda n: torch.full((n + 2,), SENTINEL32, dtype=torch.int32, device=e.device)
    inl, nm, hyp, match = i32(pairs), i32(pairs), i32(2 * pairs + 3), i32(pairs * P)
    mask = torch.full((pairs + 2,), SENTINEL, dtype=torch.int64, device=e.device)
    dist = torch.full((pairs * P * P + 2,), SENTINEL, dtype=torch.int64, device=e.device)
    need = e.lib.dlc_verify_pairs_workspace_bytes(Q, k, P)
    assert need >= pairs * P * P * 8
    ws = torch.empty(need, dtype=torch.uint8, device=e.device)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n) if full else None
    rc = e.lib.dlc_verify_pairs(e.ctx, p(qb), qb.stride(0), p(qpt), Q, p(db), db.stride(0), p(dpt), N, P, H, p(ct), ct.stride(0), k,
                                model, tol, S, mutual, C.c_void_p(inl.data_ptr() + 4), C.c_void_p(nm.data_ptr() + 4),
                                off(hyp, 16), off(mask, 8), off(match, 4), off(dist, 8), p(ws), need, None)
    assert rc == 0, e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    inl, nm, hyp, match, mask, dist = (t.cpu().numpy() for t in (inl, nm, hyp, match, mask, dist))
    assert inl[0] == inl[-1] == nm[0] == nm[-1] == SENTINEL32
    out = dict(inliers=inl[1:-1].reshape(Q, k), n_matches=nm[1:-1].reshape(Q, k))
    if not full:
        assert (hyp == SENTINEL32).all() and (match == SENTINEL32).all() and (mask == SENTINEL).all() and (dist == SENTINEL).all()
        return out
    assert (hyp[:4] == SENTINEL32).all() and hyp[-1] == SENTINEL32 and match[0] == match[-1] == SENTINEL32
    assert mask[0] == mask[-1] == SENTINEL and dist[0] == dist[-1] == SENTINEL
    out.update(hyp=hyp[4:-1].reshape(Q, k, 2), mask=mask[1:-1].view(np.uint64).reshape(Q, k), match=match[1:-1].reshape(Q, k, P),
               dist=dist[1:-1].reshape(Q, k, P, P))
    return out


def same(got, want, where=""):
    """Every pair of a raw_verify result equals the oracle's verify_pairs."""
    Q, k = got["inliers"].shape
    for r in range(Q):
        for s in range(k):
            w, at = want[r][s], (where, r, s)
            assert (int(got["inliers"][r, s]), int(got["n_matches"][r, s])) == (w["inliers"], w["n_matches"]), at
            if "hyp" not in got:
                continue
            assert tuple(int(v) for v in got["hyp"][r, s]) == w["hyp"] and int(got["mask"][r, s]) == w["mask"], at
            assert np.array_equal(got["match"][r, s], w["match"]), at
            if w["dist"] is None:
                assert (got["dist"][r, s] == SENTINEL).all(), at
            else:
                nan = np.isnan(w["dist"])                              # (a NaN's payload is not part of the definition)
                assert np.array_equal(got["dist"][r, s][~nan], bits(w["dist"])[~nan]), at
                assert np.isnan(got["dist"][r, s].view(np.float64)[nan]).all(), at


def scene(rng, Q, N, P, H, R=10, dyadic=False):
    """Descriptors whose key-frame patches are, half of them, copies of a query frame's patches at other indices (real
    matches; with dyadic values also ties), points on a small grid (coincident points, accidental agreement), some absent."""
    val = (lambda *s: rng.randint(-4, 5, size=s) / 4.0) if dyadic else (lambda *s: rng.standard_normal(s))
    qd, dd = val(Q, P, H), val(N, P, H)
    for c in range(N):
        perm = rng.permutation(P)
        take = rng.rand(P) < 0.5
        dd[c][take] = qd[c % Q][perm][take]
    qp, dp = rng.randint(0, R, size=(Q, P, 2)), rng.randint(0, R, size=(N, P, 2))
    for pts in (qp, dp):
        gone = rng.rand(*pts.shape[:2]) < 0.08
        pts[gone] = (-1, -1)
        far = rng.rand(*pts.shape[:2]) < 0.04
        pts[far, rng.randint(2)] = 8192
    return qd, qp, dd, dp


# ---- the grid: P crosses the cell tiles of 8, 16 and 32 a side, H the 32 columns of the shortest LDS chunk ------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 30, 33, 64])
@pytest.mark.parametrize("H", [1, 31, 32, 33, 100])
def test_pairs_equal_the_oracle(e, P, H):
    rng = np.random.RandomState(P * 1000 + H)
    Q, k, N = (2, 3, 4) if P <= 30 else (1, 2, 3)
    qd, qp, dd, dp = scene(rng, Q, N, P, H, dyadic=H <= 31)
    cand = rng.randint(-1, N + 1, size=(Q, k))                             # ids of -1 and N among them
    cand[0, 0] = 0
    if k > 2:
        cand[1, 1] = cand[1, 0] = N - 1                                    # the same key-frame twice in a row
    model, mutual = (SIM, TRANS)[(P + H) % 2], (P + H // 2) % 2
    tol, S = (0, 1, 3, 255)[(P + H) % 4], (0, 16, 32)[(P * 7 + H) % 3]
    want = vfo.verify_pairs(qd, qp, dd, dp, cand, model=model, tol=tol, S=S, mutual=mutual)
    same(raw_verify(e, qd, qp, dd, dp, cand, model, tol, S, mutual), want, "every output")
    same(raw_verify(e, qd, qp, dd, dp, cand, model, tol, S, mutual, full=False), want, "no optional output")


@pytest.mark.parametrize("Q,k,N", [(1, 1, 1), (8, 5, 50), (3, 13, 17)])
def test_one_pair_to_forty_pairs_over_one_to_fifty_key_frames(e, Q, k, N):
    rng = np.random.RandomState(Q * 100 + N)
    qd, qp, dd, dp = scene(rng, Q, N, 7, 9, R=8, dyadic=True)
    cand = rng.randint(-1, N + 1, size=(Q, k))
    cand[0, 0] = N - 1
    for model in (SIM, TRANS):
        same(raw_verify(e, qd, qp, dd, dp, cand, model, 1, 32, 1, cand_pad=5),
             vfo.verify_pairs(qd, qp, dd, dp, cand, model=model, tol=1, S=32, mutual=1))


@pytest.mark.parametrize("H", [64, 65, 127, 128, 129, 257])
def test_columns_either_side_of_the_chunks(e, H):
    """Few pairs take one cell per thread and chunks of 128 columns, 130 pairs of 30 patches two cells and 64 columns."""
    rng = np.random.RandomState(H)
    qd, qp, dd, dp = scene(rng, 2, 4, 30, H, R=12)
    cand = rng.randint(0, 4, size=(2, 2))
    same(raw_verify(e, qd, qp, dd, dp, cand), vfo.verify_pairs(qd, qp, dd, dp, cand), "few")
    many = np.tile(cand, (13, 5))                                          # 26 x 10 = 260 pairs x 4 tiles of 16 x 16
    got = raw_verify(e, np.tile(qd, (13, 1, 1)), np.tile(qp, (13, 1, 1)), dd, dp, many)
    few = raw_verify(e, qd, qp, dd, dp, cand)
    for key in got:
        for r in range(26):
            for s in range(10):
                assert np.array_equal(got[key][r, s], few[key][r % 2, s % 2]), (key, r, s)


def test_full_width_descriptors(e):
    """H = 2500, the CLI's SDAV: 20 chunks of 128 columns, the last one short."""
    rng = np.random.RandomState(25)
    qd, qp, dd, dp = scene(rng, 1, 6, 30, 2500, R=40)
    cand = np.array([[0, 3, 5, -1, 2]])
    same(raw_verify(e, qd, qp, dd, dp, cand, SIM, 3, 32, 1), vfo.verify_pairs(qd, qp, dd, dp, cand, model=SIM, tol=3, S=32, mutual=1))


def test_ties_nan_and_infinity(e):
    # duplicate patch rows on both sides: every tie goes to the lower index, down the rows and down the columns
    q = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 0.0], [5.0, 5.0]])
    d = np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0], [1.0, 0.0]])
    pts = np.array([[1, 1], [2, 5], [7, 3], [4, 4]])
    for mutual in (0, 1):
        got = raw_verify(e, q[None], pts[None], d[None], pts[None], np.array([[0]]), TRANS, 0, 0, mutual)
        same(got, vfo.verify_pairs(q[None], pts[None], d[None], pts[None], np.array([[0]]), model=TRANS, tol=0, S=0, mutual=mutual))
        assert got["match"][0, 0].tolist() == ([1, 1, 0, 0] if not mutual else [1, -1, 0, -1])
    # a NaN row, a NaN column, an all-NaN table and +inf distances
    rng = np.random.RandomState(3)
    qd, qp, dd, dp = scene(rng, 2, 3, 5, 4, R=6)
    qp[:], dp[:] = rng.randint(0, 6, size=qp.shape), rng.randint(0, 6, size=dp.shape)
    qd[0, 1, 2] = np.nan                                                   # row 1 of every table of query 0
    dd[1, 3, 0] = np.nan                                                   # column 3 of every table against key-frame 1
    dd[2, :, 1] = np.nan                                                   # key-frame 2: all NaN
    dd[0, 2, 3] = np.inf                                                   # column 2 against key-frame 0: +inf
    qd[1, :, 0] = np.inf                                                   # query 1: every distance +inf (or NaN)
    cand = np.array([[0, 1, 2], [0, 1, 2]])
    for mutual in (0, 1):
        want = vfo.verify_pairs(qd, qp, dd, dp, cand, model=SIM, tol=1, S=0, mutual=mutual)
        got = raw_verify(e, qd, qp, dd, dp, cand, SIM, 1, 0, mutual)
        same(got, want)
        assert (got["n_matches"][:, 2] == 0).all() and (got["match"][:, 2] == -1).all() and (got["mask"][:, 2] == 0).all()
        assert got["match"][0, 0, 1] == -1 and (got["hyp"][:, 2] == -1).all()
    assert np.isinf(got["dist"][1, 0].view(np.float64)).all()
    assert (raw_verify(e, qd, qp, dd, dp, cand, SIM, 1, 0, 0)["n_matches"][1, 0] == 5)        # +inf can win: all five match patch 0


def test_planted_scenes_scale_bound_and_models(e):
    for g, model in (((0, 1), SIM), ((2, 0), SIM), ((1, 1), SIM), ((1, 0), TRANS)):
        q, qp, d, dp, planted = vfo.planted_scene(seed=5, g=g, outliers=10)
        args = (q[None], qp[None], d[None], dp[None], np.array([[0]]))
        for tol in (0, 1, 255):
            for S in (0, 16, 32):
                for mutual in (0, 1):
                    got = raw_verify(e, *args, model, tol, S, mutual)
                    same(got, vfo.verify_pairs(*args, model=model, tol=tol, S=S, mutual=mutual), (g, tol, S, mutual))
                    refused = S == 16 and g in ((2, 0), (1, 1))            # S = 16 is scale 1 alone: 2 and sqrt(2) are refused
                    if tol == 0 and not refused:
                        assert got["inliers"][0, 0] == 20 and int(got["mask"][0, 0]) == sum(1 << i for i in planted)
                    if tol == 0 and refused:
                        assert got["inliers"][0, 0] <= 2


def test_first_hypothesis_wins_and_coincident_points(e):
    # two disjoint groups of three matches, each consistent within itself under another shift: counts are equal, (0, 1) wins
    P = 6
    q = np.arange(P, dtype=np.float64)[:, None] * np.ones((1, 3))
    qp = np.array([[0, 0], [10, 0], [0, 10], [50, 50], [60, 50], [50, 60]])
    dp = qp + np.array([[5, 5]] * 3 + [[200, 90]] * 3)
    for model, hyp in ((SIM, [0, 1]), (TRANS, [0, -1])):
        got = raw_verify(e, q[None], qp[None], q[None], dp[None], np.array([[0]]), model, 0, 32, 1)
        same(got, vfo.verify_pairs(q[None], qp[None], q[None], dp[None], np.array([[0]]), model=model, tol=0, S=32, mutual=1))
        assert got["inliers"][0, 0] == 3 and got["hyp"][0, 0].tolist() == hyp and int(got["mask"][0, 0]) == 0b000111
    # every query point the same: |u|^2 = 0 for every pair, no valid similarity; the translation still counts
    qp2 = np.array([[7, 7]] * P)
    got = raw_verify(e, q[None], qp2[None], q[None], dp[None], np.array([[0]]), SIM, 3, 0, 1)
    assert got["inliers"][0, 0] == 0 and got["n_matches"][0, 0] == P and got["hyp"][0, 0].tolist() == [-1, -1] and got["mask"][0, 0] == 0
    got = raw_verify(e, q[None], qp2[None], q[None], qp2[None] + 3, np.array([[0]]), TRANS, 0, 0, 1)
    assert got["inliers"][0, 0] == P and int(got["mask"][0, 0]) == (1 << P) - 1


def test_a_pair_does_not_depend_on_its_call(e):
    """Alone, in a batch, with the pairs reversed, at another k and other pitches: the same words."""
    rng = np.random.RandomState(11)
    Q, k, N, P, H = 4, 3, 5, 30, 40
    qd, qp, dd, dp = scene(rng, Q, N, P, H, R=12)
    cand = rng.randint(0, N, size=(Q, k))
    whole = raw_verify(e, qd, qp, dd, dp, cand)
    flipped = raw_verify(e, qd[::-1], qp[::-1], dd, dp, cand[::-1, ::-1], pads=(0, 5), cand_pad=0)
    for key in whole:
        assert np.array_equal(flipped[key][::-1, ::-1], whole[key]), key
    for r in range(Q):
        for s in range(k):
            c = int(cand[r, s])
            one = raw_verify(e, qd[r:r + 1], qp[r:r + 1], dd[c:c + 1], dp[c:c + 1], np.array([[0]]), pads=(1, 0), cand_pad=7)
            for key in whole:
                assert np.array_equal(one[key][0, 0], whole[key][r, s]), (key, r, s)


def test_few_pairs_and_many_pairs_give_the_same_bits(e):
    """One pair alone takes the one-cell-per-thread tiles, 130 pairs the 16 x 16 tiles and 520 pairs the 32 x 32 tiles: a
    cell's chain is never cut, so the tables are the same words."""
    rng = np.random.RandomState(12)
    N, P, H = 3, 30, 100
    qd, qp, dd, dp = scene(rng, 2, N, P, H, R=12)
    ref = {}
    for r in range(2):
        for c in range(N):
            ref[(r, c)] = raw_verify(e, qd[r:r + 1], qp[r:r + 1], dd[c:c + 1], dp[c:c + 1], np.array([[0]]))
    want = vfo.verify_pairs(qd, qp, dd, dp, np.array([[0, 1, 2], [0, 1, 2]]))
    for r in range(2):
        same({key: v[:, :1] for key, v in ref[(r, 1)].items()}, [[want[r][1]]])
    for reps, k in ((13, 5), (26, 10)):                                    # 130 and 520 pairs
        Q = 2 * reps
        cand = rng.randint(0, N, size=(Q, k))
        got = raw_verify(e, np.tile(qd, (reps, 1, 1)), np.tile(qp, (reps, 1, 1)), dd, dp, cand)
        for r in range(Q):
            for s in range(k):
                one = ref[(r % 2, int(cand[r, s]))]
                for key in got:
                    assert np.array_equal(got[key][r, s], one[key][0, 0]), (key, Q * k, r, s)


def test_every_refused_argument_writes_nothing(dlc, e):
    L = dlc._lib
    Q, k, N, P, H = 2, 2, 3, 4, 6
    rng = np.random.RandomState(7)
    qd, qp, dd, dp = scene(rng, Q, N, P, H)
    qb, db = padded(e, qd, 2), padded(e, dd, 2)
    qpt = torch.from_numpy(qp.astype(np.int32)).to(e.device)
    dpt = torch.from_numpy(dp.astype(np.int32)).to(e.device)
    ct = torch.zeros((Q, k + 1), dtype=torch.int64, device=e.device)
    pairs = Q * k
    i32 = lambda n: torch.full((n,), SENTINEL32, dtype=torch.int32, device=e.device)
    inl, nm, hyp, match = i32(pairs + 1), i32(pairs + 1), i32(2 * pairs + 1), i32(pairs * P + 1)
    mask = torch.full((pairs + 1,), SENTINEL, dtype=torch.int64, device=e.device)
    dist = torch.full((pairs * P * P + 1,), SENTINEL, dtype=torch.int64, device=e.device)
    need = e.lib.dlc_verify_pairs_workspace_bytes(Q, k, P)
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=e.device)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    A, S, W = L.DLC_ERR_BAD_ARG, L.DLC_ERR_BAD_SHAPE, L.DLC_ERR_WORKSPACE

    def call(q=p(qb), ldq=qb.stride(0), qp_=p(qpt), Q=Q, d=p(db), ldd=db.stride(0), dp_=p(dpt), N=N, P=P, H=H, c=p(ct),
             ldc=ct.stride(0), k=k, model=SIM, tol=3, s16=32, mutual=1, o1=p(inl), o2=p(nm), o3=p(hyp), o4=p(mask), o5=p(match),
             o6=p(dist), w=p(ws), wb=need):
        return e.lib.dlc_verify_pairs(e.ctx, q, ldq, qp_, Q, d, ldd, dp_, N, P, H, c, ldc, k, model, tol, s16, mutual, o1, o2, o3,
                                      o4, o5, o6, w, wb, None)

    cases = [
        (dict(q=None), A), (dict(qp_=None), A), (dict(d=None), A), (dict(dp_=None), A), (dict(c=None), A), (dict(o1=None), A),
        (dict(o2=None), A), (dict(q=off(qb, 4)), A), (dict(d=off(db, 4)), A), (dict(c=off(ct, 4)), A), (dict(qp_=off(qpt, 2)), A),
        (dict(dp_=off(dpt, 2)), A), (dict(o1=off(inl, 2)), A), (dict(o2=off(nm, 2)), A), (dict(o3=off(hyp, 2)), A),
        (dict(o4=off(mask, 4)), A), (dict(o5=off(match, 2)), A), (dict(o6=off(dist, 4)), A),
        (dict(Q=0), A), (dict(N=0), A), (dict(P=0), A), (dict(H=0), A), (dict(k=0), A), (dict(k=L.DLC_MAX_K + 1), A),
        (dict(ldq=H - 1), A), (dict(ldd=H - 1), A), (dict(ldc=k - 1), A), (dict(model=2), A), (dict(model=-1), A),
        (dict(tol=-1), A), (dict(tol=256), A), (dict(s16=15), A), (dict(s16=257), A), (dict(s16=-16), A), (dict(mutual=2), A),
        (dict(mutual=-1), A), (dict(P=65), S), (dict(Q=1 << 40), S), (dict(N=1 << 31), S),
        (dict(w=None), W), (dict(wb=need - 1), W), (dict(wb=0), W), (dict(w=off(ws, 8)), W),
    ]
    before = [t.clone() for t in (qb, db, qpt, dpt, ct)]
    for kw, status in cases:
        assert call(**kw) == status, sorted(kw)
        assert e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    for t in (inl, nm, hyp, match):
        assert (t == SENTINEL32).all()
    assert (mask == SENTINEL).all() and (dist == SENTINEL).all() and (ws == 0x5A).all()
    for t, b in zip((qb, db, qpt, dpt, ct), before):
        assert torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t, b.view(torch.int64) if b.dtype == torch.float64 else b)
    assert call() == 0 and call(o3=None, o4=None, o5=None, o6=None) == 0      # and the call they were derived from is accepted
    torch.cuda.synchronize()
    assert inl[pairs] == SENTINEL32 and dist[pairs * P * P] == SENTINEL and mask[pairs] == SENTINEL


# ---- through the surface -------------------------------------------------------------------------------------------------
def test_engine_wrapper_and_grown_store(dlc, e):
    rng = np.random.RandomState(21)
    n, P, H, k = 11, 30, 24, 3
    desc = rng.standard_normal((n, P, H))
    pts = rng.randint(0, 200, size=(n, P, 2)).astype(np.int32)
    for f in range(4, n):                                                  # frames 4.. revisit frame f - 4: shuffled, shifted
        perm = rng.permutation(P)
        desc[f] = desc[f - 4][perm] + 1e-3 * rng.standard_normal((P, H))
        pts[f] = pts[f - 4][perm] + (f, 2 * f)
        pts[f][:8] = rng.randint(0, 200, size=(8, 2))                      # 8 of the 30 moved elsewhere
    v = dlc.GeometricVerifier(patches=P, width=H, capacity=2, min_inliers=15, tol=0)      # grows 2 -> 4 -> 8 -> 16
    ids_all, got_inl, got_nm, got_acc = [], [], [], []
    for lo in range(0, n, 3):
        hi = min(n, lo + 3)
        first = v.append(desc[lo:hi], pts[lo:hi])
        assert first == lo and len(v) == hi
        ids = rng.randint(-1, hi, size=(hi - lo, k))                       # a candidate of the same batch is legal; -1 is none
        ids[:, 0] = np.maximum(np.arange(lo, hi) - 4, -1)
        inl, nm = v.verify(lo, torch.from_numpy(ids).to(e.device))
        ids_all.append(ids); got_inl.append(inl.cpu().numpy()); got_nm.append(nm.cpu().numpy())
        got_acc.append(v.accept(lo, ids).cpu().numpy())
    assert v.capacity == 16
    ids_all, got_inl, got_nm, got_acc = (np.concatenate(a) for a in (ids_all, got_inl, got_nm, got_acc))
    want = vfo.verify_pairs(desc, pts, desc, pts, ids_all, model=SIM, tol=0, S=32, mutual=1)
    assert np.array_equal(got_inl, np.array([[w["inliers"] for w in row] for row in want]))
    assert np.array_equal(got_nm, np.array([[w["n_matches"] for w in row] for row in want]))
    assert np.array_equal(got_acc, (got_inl >= 15) & (ids_all >= 0))
    assert (got_inl[4:, 0] >= 22).all() and (got_inl[:4, 0] == 0).all()   # the revisits are found, frames without one are not
    # apply: the lists a detector would hand over
    s = torch.from_numpy(rng.rand(3, k)).to(e.device)
    i = torch.from_numpy(ids_all[6:9]).to(e.device)
    gs, gi = v.apply(s, i, first_id=6)
    acc = got_acc[6:9]
    for r in range(3):
        kept = [int(x) for x, a in zip(ids_all[6 + r], acc[r]) if a]
        assert gi[r].tolist() == kept + [-1] * (k - len(kept))
        assert gs[r].tolist()[:len(kept)] == [float(x) for x, a in zip(s[r].tolist(), acc[r]) if a]
        assert all(x == float("-inf") for x in gs[r].tolist()[len(kept):])
    # the engine call and the one-call function, with the optional results
    dt, pt = torch.from_numpy(desc).to(e.device), torch.from_numpy(pts).to(e.device)
    it = torch.from_numpy(ids_all).to(e.device)
    inl, nm, hyp, mask, match = e.verify_pairs(dt, pt, dt, pt, it, tol=0, with_mask=True, with_match=True)
    assert np.array_equal(inl.cpu().numpy(), got_inl) and np.array_equal(nm.cpu().numpy(), got_nm)
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), np.array([[w["mask"] for w in row] for row in want], dtype=np.uint64))
    assert np.array_equal(hyp.cpu().numpy(), np.array([[w["hyp"] for w in row] for row in want]))
    assert np.array_equal(match.cpu().numpy(), np.array([[w["match"] for w in row] for row in want]))
    a, b = dlc.verify_candidates(desc, pts, desc, pts, ids_all, tol=0)
    assert isinstance(a, np.ndarray) and np.array_equal(a, got_inl) and np.array_equal(b, got_nm)
    t_inl, _ = e.verify_pairs(dt, pt, dt, pt, it, model="translation", tol=0, max_scale=None, mutual=False)
    assert np.array_equal(t_inl.cpu().numpy(), np.array([[w["inliers"] for w in row] for row in
                                                         vfo.verify_pairs(desc, pts, desc, pts, ids_all, model=TRANS, tol=0, S=0, mutual=0)]))
    for bad in (lambda: e.verify_pairs(dt, pt, dt, pt, it, model="affine"), lambda: e.verify_pairs(dt, pt, dt, pt, it, tol=256),
                lambda: e.verify_pairs(dt, pt, dt, pt, it, max_scale=0.5), lambda: e.verify_pairs(dt, pt, dt, pt.long(), it),
                lambda: e.verify_pairs(dt, pt, dt[:, :29], pt[:, :29], it), lambda: e.verify_pairs(dt, pt, dt, pt, it.int()),
                lambda: e.verify_pairs(dt.float(), pt, dt, pt, it), lambda: e.verify_pairs(dt, pt, dt, pt, it[:5]),
                lambda: v.append(desc[:2, :29], pts[:2, :29]), lambda: v.verify(n - 1, ids_all[:3])):
        with pytest.raises(ValueError):
            bad()


def run_cli(dataset, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", dataset] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


CLI_ARGS = ["--network", "sdav", "--metric", "cosine", "--exclusion", "2", "--k", "3", "--batch", "5", "--threshold", "-1"]


def test_cli_prints_only_verified_candidates(dlc, e, tmp_path):
    """The 20 golden frames through `loop_closure --verify`: what is printed is exactly the candidates of the run without
    --verify whose ORACLE inlier count reaches the limit, each followed by its verify line; the run without --verify
    prints what the CLI printed before the feature existed (tests/golden/verify_cli_parent.txt, captured then).  The
    limit is the oracle's largest count over the candidates, so that some are printed and some are not (the weights are
    untrained: the counts are small)."""
    data = tmp_path / "frames"
    data.mkdir()
    files = real_frames.frame_paths()
    for f in files:
        shutil.copy(f, str(data))
    plain = run_cli(str(data), *CLI_ARGS)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    assert plain.stdout == open(os.path.join(GOLDEN, "verify_cli_parent.txt")).read()
    assert "verify" not in plain.stdout and "frames\t20\tkey-frames\t20" in plain.stderr
    # the oracle over what the CLI's front-end and encoder produce
    from deeploopcloser_amd import pipeline
    net = dlc.SDAV()
    frames = np.stack([dlc.read_ppm(f) for f in files])
    desc, pts = pipeline.sdav_descriptors_from_frames(frames, net, return_key_points=True)
    assert np.array_equal(bits(desc.cpu().numpy()), bits(pipeline.sdav_descriptors_from_frames(frames, net).cpu().numpy()))
    desc, pts = desc.cpu().numpy(), pts.cpu().numpy()
    assert pts.shape == (20, 30, 2) and pts.dtype == np.int32 and pts.min() >= 0
    lines = plain.stdout.splitlines()
    assert lines and all(l.startswith("loop\t") for l in lines)
    oracle = []
    for l in lines:
        frame, match = int(l.split("\t")[1]), int(l.split("\t")[3])
        oracle.append(vfo.verify_pair(desc[frame], pts[frame], desc[match], pts[match], model=SIM, tol=3, S=32, mutual=1))
    counts = [w["inliers"] for w in oracle]
    limit = max(counts)
    want = []
    for l, w in zip(lines, oracle):
        if w["inliers"] >= limit:
            want += [l, "verify\t%d\t%d" % (w["inliers"], w["n_matches"])]
    print("CLI: %d candidates, oracle counts %d..%d, %d reach %d" % (len(lines), min(counts), limit, len(want) // 2, limit))
    assert 0 < len(want) // 2 < len(lines)                                 # the limit separates the candidates
    checked = run_cli(str(data), *CLI_ARGS, "--verify", str(limit))
    assert checked.returncode == 0, checked.stdout + checked.stderr
    assert checked.stdout.splitlines() == want
    assert "frames\t20\tkey-frames\t20" in checked.stderr
