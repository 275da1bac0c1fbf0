"""Half-tile champion hints of the cosine top-k (include/dlc.h, "the half-tile hints").

On the one-pass MFMA plan the score kernel writes, per (query, half tile of 128 rows), which row of the half tile's best
group holds its maximum (a*) and how high the group's other seven rows can score (r2); the 512-thread selection then
re-scores that one row instead of the group's eight where r2 rules the others out.  Nothing observable may change:

  * dlc_cosine_topk == oracle/cosine.py's exact top-k, index for index (tests/test_gpu_parity.py's comparison);
  * dlc_cosine_select_topk with the hints == the same call with DLC_SELECT_NO_HINTS, BIT FOR BIT in fp64 scores, fp32
    scores, rows and status, from one dlc_cosine_score_groups workspace.

Every shape sits on the one-pass plan: n > 16384 rows, q > 4 queries, and d < 512 or >= 249 tiles of 256 rows.
The only tolerances are test_gpu_parity's (fp64 scores against the oracle's BLAS sums: 1e-12; their fp32 roundings: one
rounding, 1.2e-7) and, where the hint array itself is read, the library's own dlc_cosine_score_error_bound.
"""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()          # raises loudly if libdlc_hip.so is missing


def stored(eng, x, dtype):
    return eng.normalize(torch.from_numpy(np.ascontiguousarray(x)).to(eng.device), dtype)


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def oracle_topk(q_st, db_st, k):
    from oracle import cosine as ocos
    return ocos.cosine_topk(f64(q_st), f64(db_st), k)


def check(eng, q_st, db_st, k, tau_scale=None, want=None):
    """Both properties for one (queries, database, k).  Returns the one-shot call's TopK and the oracle's (scores, rows)."""
    nq, d = q_st.shape
    n = db_st.shape[0]
    top = eng.match_topk(q_st, db_st, k, details=True, tau_scale=tau_scale)
    torch.cuda.synchronize()
    es, ei = oracle_topk(q_st, db_st, k) if want is None else want
    kk = es.shape[1]
    i, s = top.idx.cpu().numpy(), top.scores.cpu().numpy()
    assert np.all(i[:, kk:] == -1) and np.all(np.isneginf(s[:, kk:]))
    assert np.array_equal(i[:, :kk], ei)
    assert np.abs(s[:, :kk] - es).max() < 1.2e-7
    assert np.abs(top.scores_f64.cpu().numpy()[:, :kk] - es).max() < 1e-12
    # the two-stage call, hints on and off, from ONE score pass
    ws = torch.empty(eng.topk_workspace_bytes(nq, n, d, k), dtype=torch.uint8, device=eng.device)
    eng.score_groups(q_st, db_st, k, ws)
    got = []
    for hints in (True, False):
        o_s = torch.empty((nq, k), dtype=torch.float32, device=eng.device)
        o_i = torch.empty((nq, k), dtype=torch.int64, device=eng.device)
        o_s64 = torch.empty((nq, k), dtype=torch.float64, device=eng.device)
        o_st = torch.empty((nq,), dtype=torch.int32, device=eng.device)
        eng.select_topk(q_st, db_st, k, ws, o_s, o_i, scores_f64=o_s64, status=o_st, tau_scale=tau_scale, hints=hints)
        torch.cuda.synchronize()
        got.append((o_s64.view(torch.int64).clone(), o_s.view(torch.int32).clone(), o_i.clone(), o_st.clone()))
    for on, off in zip(got[0], got[1]):
        assert torch.equal(on, off)
    # ... and the one-shot call (which always takes the hints) hands out the same bits
    assert torch.equal(got[1][0], top.scores_f64.view(torch.int64)) and torch.equal(got[1][1], top.scores.view(torch.int32))
    assert torch.equal(got[1][2], top.idx) and torch.equal(got[1][3], top.status)
    return top, (es, ei)


RANDOM_SHAPES = [(5, 16385, 64, 20),       # the smallest one-pass call; n % 8 = 1
                 (256, 16640, 128, 20),    # one full query block, whole tiles
                 (37, 20001, 448, 1),      # the MASKQ form (37 queries), n % 8 != 0, k = 1
                 (300, 17000, 64, 128),    # two query blocks (the second masked), the largest k
                 (64, 63744, 512, 20)]     # d >= 512: one pass because there are 249 tiles


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("nq,n,d,k", RANDOM_SHAPES)
def test_random_unit_rows(eng, dtype, nq, n, d, k):
    rng = np.random.RandomState(nq * 31 + n)
    db_st = stored(eng, rng.standard_normal((n, d)).astype(np.float32), dtype)
    q_st = stored(eng, rng.standard_normal((nq, d)).astype(np.float32), dtype)
    top, _ = check(eng, q_st, db_st, k)
    assert set(top.status.cpu().tolist()) <= {0, 2}


def _align(x):
    return (x + 255) // 256 * 256


@gpu
@pytest.mark.parametrize("nq,n,d,k", [(37, 20001, 448, 1), (256, 16640, 128, 20)])
def test_hint_array_states_the_half_tiles_best_group(eng, nq, n, d, k):
    """What the score pass writes (the array sits behind the group and half-tile maxima in the workspace, entry
    ht * q + query): for every
    (query, half tile) G* is the LOWEST group whose maximum is the half tile's, row a* of it scores the maximum and no
    other row of G* scores above r2 -- held against the fp64 scores of the stored rows with the library's own error
    bound tau (an fp32 score is within tau of the fp64 one, so a maximum of fp32 scores is within tau of the fp64 maximum)."""
    rng = np.random.RandomState(5)
    db_st = stored(eng, rng.standard_normal((n, d)).astype(np.float32), "bf16")
    q_st = stored(eng, rng.standard_normal((nq, d)).astype(np.float32), "bf16")
    ws = torch.empty(eng.topk_workspace_bytes(nq, n, d, k), dtype=torch.uint8, device=eng.device)
    ws.fill_(0xff)
    eng.score_groups(q_st, db_st, k, ws)
    torch.cuda.synchronize()
    ntiles = (n + 255) // 256
    ldg, ldt, nh = ntiles * 32, ntiles * 2, (n + 127) // 128
    o_t = _align(nq * ldg * 4)
    o_h = o_t + _align(nq * ldt * 4)
    raw = ws.cpu().numpy()
    gmax = raw[:nq * ldg * 4].view(np.float32).reshape(nq, ldg)
    tmax = raw[o_t:o_t + nq * ldt * 4].view(np.float32).reshape(nq, ldt)[:, :nh]
    hint = raw[o_h:o_h + nh * nq * 8].view(np.int32).reshape(nh, nq, 2).transpose(1, 0, 2)     # stored half tile major
    r2 = hint[..., 0].copy().view(np.float32)
    gstar, astar = hint[..., 1] >> 3, hint[..., 1] & 7
    assert gstar.min() >= 0 and gstar.max() <= 15
    ng = (n + 7) // 8
    g_abs = np.arange(nh)[None, :] * 16 + gstar
    assert g_abs.max() < ng
    qq = np.arange(nq)[:, None]
    assert np.array_equal(gmax[qq, g_abs], tmax)                                   # G* holds the half tile's maximum ...
    lower = np.arange(16)[None, None, :] < gstar[..., None]                        # ... and no group in front of it does
    gm = np.full((nq, nh * 16), -np.inf, dtype=np.float32)
    gm[:, :ng] = gmax[:, :ng]
    assert not np.any((gm.reshape(nq, nh, 16) == tmax[..., None]) & lower)
    assert np.all(r2 <= tmax)
    tau = eng.score_error_bound(nq, n, d, k)
    s = f64(q_st) @ f64(db_st).T                                                   # [nq, n] fp64 scores
    sp = np.full((nq, nh * 128), -np.inf)
    sp[:, :n] = s
    grp = sp.reshape(nq, nh * 16, 8)[qq, g_abs]                                    # [nq, nh, 8]: the rows of G*
    row = g_abs * 8 + astar
    assert row.max() < n
    best = np.take_along_axis(grp, astar[..., None], axis=2)[..., 0]
    assert np.abs(best - tmax).max() <= tau                                        # row a* scores the maximum
    others = grp.copy()
    np.put_along_axis(others, astar[..., None], -np.inf, axis=2)
    assert np.all(others.max(axis=2) <= r2.astype(np.float64) + tau)               # r2 bounds the other seven


# ---------------------------------------------------------------------------------------------------------------------
# crafted cases: bf16, d = 128, n = 16640 (65 tiles), k = 4; query 0 is the crafted one, seven random ones beside it
N0, D0, K0, NQ0 = 16640, 128, 4, 8


def crafted(eng, n=N0, seed=11):
    rng = np.random.RandomState(seed)
    db_st = stored(eng, rng.standard_normal((n, D0)).astype(np.float32), "bf16")
    q_st = stored(eng, rng.standard_normal((NQ0, D0)).astype(np.float32), "bf16")
    return db_st, q_st


@gpu
@pytest.mark.parametrize("src,dst", [(128 * 41 + 8 * 2 + 2, 128 * 41 + 8 * 2 + 5),       # the copy in the same group
                                     (128 * 41 + 8 * 2 + 1, 128 * 41 + 8 * 9 + 4),       # another group of the half tile
                                     (128 * 41 + 8 * 2 + 1, 128 * 97 + 8 * 15 + 7)])     # another half tile
def test_exact_copy_of_the_best_row(eng, src, dst):
    db_st, q_st = crafted(eng)
    db_st[dst] = db_st[src]
    q_st[0] = db_st[src]
    top, _ = check(eng, q_st, db_st, K0)
    assert top.idx[0, :2].cpu().tolist() == [src, dst]                             # both, the lower index first
    assert float(top.scores_f64[0, 0]) == float(top.scores_f64[0, 1])


@gpu
def test_best_row_is_the_last_row_of_a_ragged_database(eng):
    """n % 8 = 3: the last group's five missing rows are copies of row n - 1 in the score pass, so the group's runner-up
    equals its maximum and the group is re-scored whole; rows past n must never come back."""
    n = N0 - 5
    assert n % 8 == 3 and n > 16384
    db_st, q_st = crafted(eng, n=n)
    q_st[0] = db_st[n - 1]
    top, _ = check(eng, q_st, db_st, K0)
    assert int(top.idx[0, 0]) == n - 1 and int(top.idx.max()) < n


@gpu
def test_runner_up_one_ulp_away_in_the_same_group(eng):
    """The best row's neighbour in its group is the same vector with its last element one bf16 ulp off: the group's
    runner-up scores far above the k-th group maximum, the hint cannot rule it out, and both rows come back in the
    oracle's order."""
    db_st, q_st = crafted(eng)
    r = 128 * 33 + 8 * 6 + 3
    bits = db_st.view(torch.int16)
    bits[r + 1] = bits[r]
    bits[r + 1, D0 - 1] += 1
    q_st[0] = db_st[r]
    top, (es, ei) = check(eng, q_st, db_st, K0)
    assert sorted(top.idx[0, :2].cpu().tolist()) == [r, r + 1]
    assert es[0, 1] > es[0, 2] + 0.1                           # (nothing else in the database comes near the pair)


@gpu
def test_crowded_copies_take_the_exhaustive_pass(eng):
    """bench.py --crowded: kg * 8 + 1 exact copies of query 0's row, evenly spread -- the selected groups hold at most
    kg * 8 of them, the k-th score ties with a row left behind, the certificate refuses (status 1 inside the call) and the
    exhaustive pass resolves the query (status 2 handed out), with and without hints."""
    db_st, q_st = crafted(eng)
    copies = eng.groups_per_query(K0) * 8 + 1
    where = np.unique(np.linspace(0, N0 - 1, copies).astype(np.int64))
    q_st[0] = db_st[int(where[0])]
    db_st[torch.as_tensor(where, device=eng.device)] = q_st[0]
    top, _ = check(eng, q_st, db_st, K0)
    assert int(top.status[0]) == 2
    assert top.idx[0].cpu().tolist() == where[:K0].tolist()


@gpu
def test_zero_query(eng):
    db_st, q_st = crafted(eng)
    q_st[0] = 0
    top, _ = check(eng, q_st, db_st, K0)
    assert top.idx[0].cpu().tolist() == [0, 1, 2, 3]                               # every score is 0: the lowest rows
    assert np.all(top.scores_f64[0].cpu().numpy() == 0.0)


@gpu
def test_infinite_tau_scale_skips_nothing(eng):
    """tau_scale = +inf for one query certifies nothing and may skip nothing: u_k - 2 tau is -inf, no runner-up is below
    it, every selected group is re-scored whole and the exhaustive pass decides -- the same lists as ever."""
    db_st, q_st = crafted(eng)
    ts = torch.ones((NQ0,), dtype=torch.float32, device=eng.device)
    ts[0] = float("inf")
    top, _ = check(eng, q_st, db_st, K0, tau_scale=ts)
    assert int(top.status[0]) == 2 and set(top.status[1:].cpu().tolist()) == {0}


# ---------------------------------------------------------------------------------------------------------------------
def test_workspace_grows_by_the_hint_array():
    """CPU: dlc_cosine_topk_workspace_bytes = the arrays of the plan + q * ldt 8-byte hints behind the half-tile maxima,
    each rounded up to 256 bytes (ldt = 2 * tiles of 256 rows).  Shapes whose plan has no other array: one pass (MFMA or, for
    <= 4 queries, the bandwidth kernel), more than 16384 rows, short enough rows that the re-score is not spread."""
    from deeploopcloser_amd import _lib
    lib = _lib.load()
    for q, n, d, k in [(256, 1_000_000, 4096, 20), (5, 16385, 64, 20), (37, 20001, 448, 1), (300, 17000, 64, 128),
                       (64, 63744, 512, 20), (2, 100_000, 64, 20)]:
        ntiles = (n + 255) // 256
        ldg, ldt = ntiles * 32, ntiles * 2
        hint = _align(q * ldt * 8)
        rest = _align(q * ldg * 4) + _align(q * ldt * 4) + _align(q * 4) + _align(q * k * 8)
        assert lib.dlc_cosine_topk_workspace_bytes(q, n, d, k) == rest + hint, (q, n, d, k)
    for q, n, d, k in [(256, 1000, 4096, 20), (1, 1063, 75008, 20), (8, 9000, 4096, 20), (5, 1000, 8192, 10), (1, 1, 64, 1)]:
        w = lib.dlc_cosine_topk_workspace_bytes(q, n, d, k)                        # every other plan: the room is there too
        ntiles = (n + 255) // 256
        assert w % 256 == 0 and w >= _align(q * ntiles * 32 * 4) + _align(q * ntiles * 2 * 4) + _align(q * ntiles * 2 * 8)
