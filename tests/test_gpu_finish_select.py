"""The filtered selection of the cosine top-k finish (include/dlc.h, "the filtered selection") against the general one.

The 512-thread finish finds its kt best half tiles, and the kg best groups inside them, by a threshold filter followed by a
ranking of what passed, reads the half-tile maxima straight from the workspace up to 8192 half tiles, and ranks only the
rows it re-scored.  DLC_SELECT_SERIAL (Engine.select_topk / select_groups, serial=True) runs the one-by-one extraction and
the full rankings instead.  Nothing observable may differ:

  * from ONE dlc_cosine_score_groups workspace, dlc_cosine_select_topk with flags 0, SERIAL, NO_HINTS and SERIAL | NO_HINTS
    hands out the same fp64 scores, fp32 scores, rows and status BIT FOR BIT;
  * dlc_cosine_select_groups with and without SERIAL: the same group ids and maxima, the bound column included;
  * dlc_cosine_topk under every prune mode (off / on / keep) hands out those same bits;
  * the default path == oracle/cosine.py's exact top-k, index for index (tests/test_gpu_topk_hints.py's comparison and
    tolerances: fp64 scores within 1e-12 of the oracle's BLAS sums, their fp32 roundings within one rounding, 1.2e-7).

Shapes: d = 64 throughout (the selection does not depend on d); n = 16512 is just past the small-database plan (129 half
tiles: fewer keys than slots, no threshold), 70000 gives every lane more than one value, 1048576 / 1048704 are the last
register-path size (8192 half tiles) and the first staged one (8193).
"""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
D = 64


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    e = d.default_engine()          # raises loudly if libdlc_hip.so is missing
    yield e
    e.set_prune_mode("on")


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def random_rows(eng, n, dtype, seed):
    g = torch.Generator(device=eng.device)
    g.manual_seed(seed)
    return eng.normalize(torch.randn((n, D), generator=g, device=eng.device), dtype)


def select_bits(eng, q_st, db_st, k, ws, hints, serial):
    nq = q_st.shape[0]
    o_s = torch.empty((nq, k), dtype=torch.float32, device=eng.device)
    o_i = torch.empty((nq, k), dtype=torch.int64, device=eng.device)
    o_s64 = torch.empty((nq, k), dtype=torch.float64, device=eng.device)
    o_st = torch.empty((nq,), dtype=torch.int32, device=eng.device)
    eng.select_topk(q_st, db_st, k, ws, o_s, o_i, scores_f64=o_s64, status=o_st, hints=hints, serial=serial)
    torch.cuda.synchronize()
    return (o_s64.view(torch.int64).clone(), o_s.view(torch.int32).clone(), o_i.clone(), o_st.clone())


def groups_bits(eng, q_st, db_st, k, ws, serial):
    nq, kg = q_st.shape[0], eng.groups_per_query(k)
    ids = torch.empty((nq, kg), dtype=torch.int32, device=eng.device)
    mx = torch.empty((nq, kg + 1), dtype=torch.float32, device=eng.device)
    eng.select_groups(q_st, db_st, k, ws, ids, mx, serial=serial)
    torch.cuda.synchronize()
    return ids.clone(), mx.view(torch.int32).clone()


NAMES = ("scores_f64", "scores", "idx", "status")


def check(eng, q_st, db_st, k, modes=("off", "on", "keep")):
    """Every property of the module docstring for one (queries, database, k).  -> (fp64 scores, rows, status) as NumPy."""
    nq, n = q_st.shape[0], db_st.shape[0]
    ws = torch.empty(eng.topk_workspace_bytes(nq, n, D, k), dtype=torch.uint8, device=eng.device)
    eng.score_groups(q_st, db_st, k, ws)
    g0, g1 = groups_bits(eng, q_st, db_st, k, ws, False), groups_bits(eng, q_st, db_st, k, ws, True)
    assert torch.equal(g0[0], g1[0]), "group ids"
    assert torch.equal(g0[1], g1[1]), "group maxima / bound column"
    ref = select_bits(eng, q_st, db_st, k, ws, True, False)
    for hints, serial in ((True, True), (False, False), (False, True)):
        got = select_bits(eng, q_st, db_st, k, ws, hints, serial)
        for name, a, b in zip(NAMES, ref, got):
            assert torch.equal(a, b), (name, "hints" if hints else "no hints", "serial" if serial else "filtered")
    try:
        for mode in modes:
            eng.set_prune_mode(mode)
            for _ in range(2 if mode == "keep" else 1):                 # keep: the second call starts from the first one's bound
                top = eng.match_topk(q_st, db_st, k, details=True)
                torch.cuda.synchronize()
                got = (top.scores_f64.view(torch.int64), top.scores.view(torch.int32), top.idx, top.status)
                for name, a, b in zip(NAMES, ref, got):
                    assert torch.equal(a, b), (name, "prune " + mode)
    finally:
        eng.set_prune_mode("on")
    from oracle import cosine as ocos
    es, ei = ocos.cosine_topk(f64(q_st), f64(db_st), k)
    kk = es.shape[1]
    s64 = ref[0].view(torch.float64).cpu().numpy()
    s32 = ref[1].view(torch.float32).cpu().numpy()
    idx = ref[2].cpu().numpy()
    assert np.all(idx[:, kk:] == -1) and np.all(np.isneginf(s32[:, kk:]))
    assert np.array_equal(idx[:, :kk], ei)
    assert np.abs(s32[:, :kk] - es).max() < 1.2e-7
    assert np.abs(s64[:, :kk] - es).max() < 1e-12
    return s64, idx, ref[3].cpu().numpy()


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("nq,n,k", [(1, 16512, 20), (5, 16512, 20), (256, 16512, 20), (5, 16512, 60),
                                    (7, 70000, 20), (7, 70000, 60),
                                    (6, 1048576, 20), (6, 1048704, 20)])
def test_random_unit_rows(eng, dtype, nq, n, k):
    db_st = random_rows(eng, n, dtype, n + k)
    q_st = random_rows(eng, nq, dtype, nq)
    _, _, status = check(eng, q_st, db_st, k)
    assert set(status.tolist()) <= {0, 2}


N1, K1, NQ1 = 70000, 20, 6          # crafted cases: query 0 is the crafted one, five random ones beside it
KT1 = K1 + 4


def crafted(eng, n=N1, seed=17):
    return random_rows(eng, n, "bf16", seed), random_rows(eng, NQ1, "bf16", seed + 1)


@gpu
def test_identical_rows(eng):
    """Every half tile has the same maximum: all 157 keys pass any threshold (more than 16 kg slots with k = 5: the general
    extraction runs), every score ties, nothing certifies and the exhaustive pass hands out the lowest rows."""
    n, k = 20000, 5
    db_st, q_st = crafted(eng, n=n)
    db_st[:] = db_st[0]
    assert (n + 127) // 128 > (k + 4) * 16
    _, idx, status = check(eng, q_st, db_st, k)
    assert np.array_equal(idx, np.tile(np.arange(k), (NQ1, 1)))
    assert set(status.tolist()) == {2}


@gpu
def test_kt_plus_one_tied_half_tiles(eng):
    """Exact copies of query 0's row in kt + 1 half tiles: their maxima tie, the kt lower ones are selected and the tied
    maximum is the bound of what is left behind -- the certificate refuses and the exhaustive pass finds the k lowest."""
    db_st, q_st = crafted(eng)
    hts = np.unique(np.linspace(3, (N1 + 127) // 128 - 2, KT1 + 1).astype(np.int64))
    assert hts.size == KT1 + 1
    rows = hts * 128 + (hts * 37) % 128
    q_st[0] = db_st[int(rows[0])]
    db_st[torch.as_tensor(rows, device=eng.device)] = q_st[0]
    _, idx, status = check(eng, q_st, db_st, K1)
    assert idx[0].tolist() == rows[:K1].tolist()
    assert int(status[0]) == 2


def plant_near_copies(eng, db_st, q_st, rows, seed=5):
    """Rows `rows` of the database become query 0 plus a little noise: its top-k, all distinct scores."""
    g = torch.Generator(device=eng.device)
    g.manual_seed(seed)
    base = q_st[0].float()
    noise = torch.randn((len(rows), D), generator=g, device=eng.device)
    scale = torch.linspace(0.02, 0.2, len(rows), device=eng.device)[:, None]
    db_st[torch.as_tensor(rows, device=eng.device)] = eng.normalize(base[None, :] + scale * noise / np.sqrt(D), "bf16")


@gpu
@pytest.mark.parametrize("where", ["first_eighth", "lane_5", "one_half_tile"])
def test_the_top_sits_in_one_slice(eng, where):
    """The threshold comes from lane maxima of single waves: with the best rows all in wave 0's slice, all in half tiles
    = 5 mod 64 (one lane of every wave at 8192 half tiles), or all in ONE half tile, it is found elsewhere or falls low --
    the lists stay the oracle's."""
    n = 1048576 if where == "lane_5" else N1
    db_st, q_st = crafted(eng, n=n)
    rng = np.random.RandomState(3)
    nh = n // 128 if n % 128 == 0 else n // 128 + 1
    if where == "first_eighth":
        rows = rng.choice(n // 8 - 128, 30, replace=False)
    elif where == "lane_5":
        hts = 5 + 64 * rng.choice(nh // 64, 30, replace=False)
        rows = hts * 128 + rng.randint(0, 128, size=30)
    else:
        rows = 128 * 211 + rng.choice(128, 30, replace=False)
    rows = np.sort(rows)
    plant_near_copies(eng, db_st, q_st, rows)
    _, idx, _ = check(eng, q_st, db_st, K1, modes=("on",) if where == "lane_5" else ("off", "on", "keep"))
    assert set(idx[0].tolist()) <= set(rows.tolist())


@gpu
def test_scores_ascending_with_the_row_index(eng):
    """Every query's score grows with the row index: the whole top sits in the last wave's last lanes, and the pruned
    score pass sees its threshold rise with every tile."""
    n = N1
    g = torch.Generator(device=eng.device)
    g.manual_seed(23)
    q_st = random_rows(eng, 1, "bf16", 29).repeat(NQ1, 1).contiguous()
    alpha = (0.9 * torch.arange(1, n + 1, device=eng.device, dtype=torch.float32) / n)[:, None]
    noise = torch.randn((n, D), generator=g, device=eng.device) / np.sqrt(D)
    db_st = eng.normalize(alpha * q_st[0].float()[None, :] + torch.sqrt(1 - alpha * alpha) * noise, "bf16")
    _, idx, _ = check(eng, q_st, db_st, K1)
    assert idx.min() > n - n // 4


@gpu
@pytest.mark.parametrize("limit0", [-1, 126, 128, 128 * KT1 - 1])
def test_older_than_limits(eng, limit0):
    """dlc_cosine_topk_older: query i sees the rows below limit0 + i -- 0, 0 and 1 rows; 126 .. 128; 128 .. 130 (one half
    tile and the first row of the next); 128 kt - 1 .. 128 kt + 1 (kt half tiles, one row less and one more)."""
    from oracle import cosine as ocos
    db_st, q_st = crafted(eng, n=16512)
    q_st = q_st[:3].contiguous()
    top = eng.match_topk(q_st, db_st, K1, details=True, older_than=limit0)
    torch.cuda.synchronize()
    idx, s64 = top.idx.cpu().numpy(), top.scores_f64.cpu().numpy()
    for i in range(3):
        vis = max(0, limit0 + i)
        kk = min(K1, vis)
        assert np.all(idx[i, kk:] == -1) and np.all(np.isneginf(s64[i, kk:]))
        if kk:
            es, ei = ocos.cosine_topk(f64(q_st[i:i + 1]), f64(db_st[:vis]), kk)
            assert np.array_equal(idx[i, :kk], ei[0])
            assert np.abs(s64[i, :kk] - es[0]).max() < 1e-12
