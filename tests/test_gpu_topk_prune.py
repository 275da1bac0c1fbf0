"""The pruned score pass of dlc_cosine_topk (include/dlc.h, "the pruned score pass") against the unpruned one.

Engine.set_prune_mode: "off" writes every group maximum and hint (the call as it was), "on" is the default, "keep" makes a
repeated identical call start from its own final threshold, so that it writes exactly the half tiles pruning can never
drop -- deterministic at these sizes, where one dispatch round of the score kernel never sees a refreshed threshold.
Between the two calls of a keep run the tests fill the group-maximum and hint arrays of the engine's workspace with 0xff
(NaNs / impossible hints): whatever the second call reads and did not write is garbage.

Nothing observable may change: fp64 scores, fp32 scores, rows and status agree BIT FOR BIT across the three modes, and with
oracle/cosine.py as tests/test_gpu_topk_hints.py compares (rows identical; fp64 scores within 1e-12 of the oracle's BLAS
sums, their fp32 roundings within one rounding, 1.2e-7).  No test looks at what a pruned call skipped: that depends on
timing by design.
"""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    e = d.default_engine()          # raises loudly if libdlc_hip.so is missing
    yield e
    e.set_prune_mode("on")


def stored(eng, x, dtype):
    return eng.normalize(torch.from_numpy(np.ascontiguousarray(x)).to(eng.device), dtype)


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def oracle_topk(q_st, db_st, k):
    from oracle import cosine as ocos
    return ocos.cosine_topk(f64(q_st), f64(db_st), k)


def _align(x):
    return (x + 255) // 256 * 256


def bits(top):
    torch.cuda.synchronize()
    return (top.scores_f64.view(torch.int64).clone(), top.scores.view(torch.int32).clone(), top.idx.clone(), top.status.clone())


def garble_group_maxima_and_hints(eng, nq, n, d, k):
    """0xff over the gmax and hint arrays of the workspace match_topk uses on this stream (the half-tile maxima and the
    prune state behind the workspace stay)."""
    need = eng.topk_workspace_bytes(nq, n, d, k) + eng.lib.dlc_cosine_topk_prune_bytes(nq, n, d, k)
    ws = eng.workspace("topk", need)
    ntiles = (n + 255) // 256
    ldg, ldt = ntiles * 32, ntiles * 2
    o_t = _align(nq * ldg * 4)
    o_h = o_t + _align(nq * ldt * 4)
    ws[:nq * ldg * 4] = 0xff
    ws[o_h:o_h + nq * ldt * 8] = 0xff
    torch.cuda.synchronize()


def match(eng, mode, q_st, db_st, k, tau_scale=None):
    """match_topk(details=True) under one mode, as bits.  keep: the call twice, the arrays garbled in between."""
    nq, d = q_st.shape
    eng.set_prune_mode(mode)
    try:
        top = eng.match_topk(q_st, db_st, k, details=True, tau_scale=tau_scale)
        if mode == "keep":
            first = bits(top)
            garble_group_maxima_and_hints(eng, nq, db_st.shape[0], d, k)
            top = eng.match_topk(q_st, db_st, k, details=True, tau_scale=tau_scale)
            for a, b in zip(first, bits(top)):
                assert torch.equal(a, b)
        return top, bits(top)
    finally:
        eng.set_prune_mode("on")


def check_modes(eng, q_st, db_st, k, tau_scale=None, modes=("off", "on", "keep")):
    """All modes agree bit for bit, and with the oracle.  Returns the reference ("off") TopK and the oracle's (scores, rows)."""
    ref_top, ref = match(eng, "off", q_st, db_st, k, tau_scale)
    for mode in modes[1:]:
        _, got = match(eng, mode, q_st, db_st, k, tau_scale)
        for name, a, b in zip(("scores_f64", "scores", "idx", "status"), ref, got):
            assert torch.equal(a, b), (mode, name)
    es, ei = oracle_topk(q_st, db_st, k)
    kk = es.shape[1]
    i, s = ref_top.idx.cpu().numpy(), ref_top.scores.cpu().numpy()
    assert np.all(i[:, kk:] == -1) and np.all(np.isneginf(s[:, kk:]))
    assert np.array_equal(i[:, :kk], ei)
    assert np.abs(s[:, :kk] - es).max() < 1.2e-7
    assert np.abs(ref_top.scores_f64.cpu().numpy()[:, :kk] - es).max() < 1e-12
    return ref_top, (es, ei)


SHAPES = [(5, 16385, 64, 20),        # the smallest one-pass call
          (256, 16640, 128, 20),     # one full query block
          (37, 20001, 448, 1)]       # masked queries, n % 8 != 0


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("nq,n,d,k", SHAPES)
def test_modes_agree_on_random_unit_rows(eng, dtype, nq, n, d, k):
    assert eng.lib.dlc_cosine_topk_prune_bytes(nq, n, d, k) > 0            # (the shape does prune)
    rng = np.random.RandomState(nq * 31 + n)
    db_st = stored(eng, rng.standard_normal((n, d)).astype(np.float32), dtype)
    q_st = stored(eng, rng.standard_normal((nq, d)).astype(np.float32), dtype)
    top, _ = check_modes(eng, q_st, db_st, k)
    assert set(top.status.cpu().tolist()) <= {0, 2}


@gpu
def test_more_groups_than_classes_takes_the_off_route(eng):
    """kg = 128 + 4 > 64 classes: the call does not prune in any mode (no room is asked for), and still matches."""
    nq, n, d, k = 300, 17000, 64, 128
    assert eng.lib.dlc_cosine_topk_prune_bytes(nq, n, d, k) == 0
    rng = np.random.RandomState(nq * 31 + n)
    db_st = stored(eng, rng.standard_normal((n, d)).astype(np.float32), "bf16")
    q_st = stored(eng, rng.standard_normal((nq, d)).astype(np.float32), "bf16")
    check_modes(eng, q_st, db_st, k)


# crafted cases: bf16, d = 128, n = 16640 (65 tiles, 130 half tiles), k = 4 (kg = kt = 8); query 0 is the crafted one
N0, D0, K0, NQ0 = 16640, 128, 4, 8


def crafted(eng, seed=11):
    rng = np.random.RandomState(seed)
    db_st = stored(eng, rng.standard_normal((N0, D0)).astype(np.float32), "bf16")
    q_st = stored(eng, rng.standard_normal((NQ0, D0)).astype(np.float32), "bf16")
    return db_st, q_st


@gpu
def test_crowded_copies_take_the_exhaustive_pass_behind_a_pruned_score_pass(eng):
    """kg * 8 + 1 exact copies of query 0's row, evenly spread: the k-th score ties with a row left behind, the certificate
    refuses and the exhaustive pass decides -- in keep mode from group maxima of which only the top half tiles' are real."""
    db_st, q_st = crafted(eng)
    copies = eng.groups_per_query(K0) * 8 + 1
    where = np.unique(np.linspace(0, N0 - 1, copies).astype(np.int64))
    q_st[0] = db_st[int(where[0])]
    db_st[torch.as_tensor(where, device=eng.device)] = q_st[0]
    s = f64(q_st[0:1]) @ f64(db_st[torch.as_tensor(where, device=eng.device)]).T
    assert len(where) == copies and np.all(s == s[0, 0])                   # the copies tie, exactly
    top, (es, ei) = check_modes(eng, q_st, db_st, K0, modes=("off", "keep"))
    assert int(top.status[0]) == 2                                         # reached under "off": the case tests something
    assert ei[0].tolist() == where[:K0].tolist() and np.all(es[0] == s[0, 0])


@gpu
def test_near_ties_below_the_final_threshold_take_whole_half_tiles(eng):
    """30 near-copies of query 0's row in 30 different half tiles, each one bf16 ulp further off in the element where the
    query is largest, and a tau_scale for query 0 that makes them all near-ties of the k-th score: the exhaustive pass's
    bound theta = s_k - tau falls BELOW thr_final (the 8th largest half-tile maximum), so half tiles whose group maxima a
    pruned score pass did not write qualify -- the pass must take their 16 groups whole."""
    db_st, q_st = crafted(eng)
    r = 128 * 3 + 17
    q_st[0] = db_st[r]
    e = int(torch.argmax(q_st[0].float().abs()))
    raw = db_st.view(torch.int16)
    planted = [128 * (5 + 4 * j) + 8 * (j % 16) + (j % 8) for j in range(30)]          # half tiles 5, 9, ..., 121
    for j, row in enumerate(planted):
        raw[row] = raw[r]
        raw[row, e] -= j + 1                                                # j + 1 ulps towards zero: a slightly lower score
    s = (f64(q_st[0:1]) @ f64(db_st[torch.as_tensor([r] + planted, device=eng.device)]).T)[0]
    assert np.all(np.diff(s) < 0)                                           # strictly descending: r, then the planted rows
    tau = eng.score_error_bound(NQ0, N0, D0, K0)
    ts = torch.ones((NQ0,), dtype=torch.float32, device=eng.device)
    ts[0] = float(2.0 * (s[0] - s[-1]) / tau)                               # tau_0 = twice the whole spread of the near-ties
    assert float(ts[0]) > 1.0
    top, _ = check_modes(eng, q_st, db_st, K0, tau_scale=ts, modes=("off", "keep"))
    assert int(top.status[0]) == 2 and set(top.status[1:].cpu().tolist()) == {0}
    assert top.idx[0].cpu().tolist() == [r] + planted[:K0 - 1]
    # the gap is really there: from a score_groups workspace (always whole), query 0's half-tile maxima between theta and
    # the kt-th largest of them
    ws = torch.empty(eng.topk_workspace_bytes(NQ0, N0, D0, K0), dtype=torch.uint8, device=eng.device)
    eng.score_groups(q_st, db_st, K0, ws)
    torch.cuda.synchronize()
    ntiles = (N0 + 255) // 256
    o_t = _align(NQ0 * ntiles * 32 * 4)
    tmax = ws[o_t:o_t + NQ0 * ntiles * 2 * 4].cpu().numpy().view(np.float32).reshape(NQ0, ntiles * 2)[0]
    kt = eng.groups_per_query(K0)
    thr_final = np.sort(tmax)[::-1][kt - 1]
    theta = float(top.scores_f64[0, K0 - 1]) - tau * float(ts[0])
    assert int(((tmax.astype(np.float64) >= theta) & (tmax < thr_final)).sum()) >= 20
