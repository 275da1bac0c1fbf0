"""The K tail of score_gemm_kernel (cosine_topk.hip): no DMA for a K tile past the workgroup's last one, and waits
that count what is really in flight.

What goes wrong when a tail wait is one short, or a skipped issue is still counted, is a stale or half-landed K tile
under the MFMAs.  So:

  * the data are random (fixed seed) and drawn PER K TILE: elements of tile t are b_t + N(0, 1) with b_t = 2, 2.5, 3 by
    t % 3, in the database and in the queries.  Every tile's share of every score is then positive and large -- about
    64 b_t^2 / (|q| |x|) -- and differs from the share of the tiles two and three before it, whose data a ring slot held
    last; `_tile_shares_are_large` asserts, in fp64 on the CPU, that the smallest share of any tile in any score is more
    than 100 tau.  A dropped, repeated or half-landed tile moves a score by thousands of tau.
  * every case is checked twice over: the dense fp32 scores (dlc_cosine_scores) against the fp64 product of the stored
    bits, elementwise within the library's own bound dlc_cosine_score_error_bound (tau, what the certificate of every
    selection rests on; tests/test_gpu_parity.py::test_score_error_bound_holds), and the top-k indices (k = 5) equal to
    the fp64 oracle's, scores within one fp32 rounding (1.2e-7, as everywhere in test_gpu_parity.py);
  * every call is made twice and the two results must be bit-equal: a race on a tail half shows up as a difference.

Shapes are the smallest that reach each branch.
  One pass: d = 64 .. 320 is nk = 1 .. 5 K tiles: the prologue alone decides nk = 1 and 2 (no second tile to issue,
    wait 0 / wait 8), nk = 3, 4, 5 add one, two and three steady iterations in front of the two tail iterations.
    n = 1, 255, 257, 513: one row (every DMA row clamped), a tile short of one row, a second and a third tile.
    q = 8, 200, 256, 257: MASKQ with one and with three live column blocks, the unmasked form, a second query block.
    GEMM_DENSE through cosine_scores for every shape; match_topk on n >= 255 (the small-database plan: GEMM_DENSE
    again, then the row selection); GEMM_GROUPS needs more than 16 384 rows, so n = 16 640 at d = 64 and d = 192.
  Split-K (GEMM_PARTIAL): few rows x long rows, `SPLIT_SHAPES` below, with the chunking each one expects.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 5
SEED = 20261020


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()          # raises loudly if libdlc_hip.so is missing


def _draw(rng, rows, d):
    """rows x d, K tile t (64 columns) drawn as b_t + N(0, 1), b_t = 2 + 0.5 * (t % 3)."""
    bias = np.repeat(2.0 + 0.5 * (np.arange(d // 64) % 3), 64)
    return (rng.standard_normal((rows, d)) + bias).astype(np.float32)


_cache = {}


def _operands(eng, dtype, d, n, nq):
    """Stored (normalised, rounded) database [n, d] and queries [nq, d] and the fp64 product of the stored bits, made
    once per (dtype, d, n, nq) and never modified: the cases below slice them (rows are normalised one by one, so a
    slice of the stored rows is the stored slice)."""
    key = (dtype, d, n, nq)
    if key not in _cache:
        rng = np.random.RandomState((SEED + 7919 * d + n) % (2 ** 31) + (dtype == "f16"))
        db_st = eng.normalize(torch.from_numpy(_draw(rng, n, d)).to(eng.device), dtype)
        q_st = eng.normalize(torch.from_numpy(_draw(rng, nq, d)).to(eng.device), dtype)
        assert db_st.shape[1] == d and q_st.shape[1] == d
        dbn = db_st.float().cpu().numpy().astype(np.float64)
        qn = q_st.float().cpu().numpy().astype(np.float64)
        _cache[key] = (db_st, q_st, dbn, qn, qn @ dbn.T)
    return _cache[key]


def _tile_shares_are_large(qn, dbn, tau):
    """Every K tile's share of every score is more than 100 tau (fp64, on the CPU; a sample of the rows where the
    operands are large)."""
    qs, dbs = qn[:64], dbn[:2048]
    smallest = min(float(np.abs(qs[:, t:t + 64] @ dbs[:, t:t + 64].T).min()) for t in range(0, qn.shape[1], 64))
    assert smallest > 100.0 * tau, (smallest, tau)


def _check_dense(eng, q_st, db_st, ref, tau, what):
    s = eng.cosine_scores(q_st, db_st)
    s2 = eng.cosine_scores(q_st, db_st)
    torch.cuda.synchronize()
    assert torch.equal(s, s2), ("dense scores differ between two calls", what)
    err = float(np.abs(s.cpu().numpy().astype(np.float64) - ref).max())
    print("%s: dense max|err| = %.3g, tau = %.3g" % (what, err, tau))
    assert s.shape == ref.shape and err <= tau, (what, err, tau)


def _check_topk(eng, q_st, db_st, qn, dbn, what):
    from oracle import cosine as ocos
    s, i = eng.match_topk(q_st, db_st, K)
    s2, i2 = eng.match_topk(q_st, db_st, K)
    torch.cuda.synchronize()
    assert torch.equal(i, i2) and torch.equal(s, s2), ("top-k differs between two calls", what)
    es, ei = ocos.cosine_topk(qn, dbn, K)
    assert np.array_equal(i.cpu().numpy(), ei), ("top-k indices differ from the fp64 oracle's", what)
    assert np.abs(s.cpu().numpy() - es).max() < 1.2e-7, what


# --------------------------------------------------------------------------- one pass: nk = 1 .. 5
N_MAX, Q_MAX = 513, 257


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 128, 192, 256, 320])
@pytest.mark.parametrize("n", [1, 255, 257, 513])
@pytest.mark.parametrize("nq", [8, 200, 256, 257])
def test_one_pass_dense_and_small_database_topk(eng, dtype, d, n, nq):
    db_all, q_all, dbn_all, qn_all, ref_all = _operands(eng, dtype, d, N_MAX, Q_MAX)
    assert eng.lib.dlc_cosine_scores_workspace_bytes(nq, n, d) == 0            # one pass: no split-K partials planned
    tau = eng.score_error_bound(nq, n, d, K)
    _tile_shares_are_large(qn_all, dbn_all, tau)
    what = "%s d=%d n=%d q=%d" % (dtype, d, n, nq)
    _check_dense(eng, q_all[:nq], db_all[:n], ref_all[:nq, :n], tau, what)
    if n >= 255:
        _check_topk(eng, q_all[:nq], db_all[:n], qn_all[:nq], dbn_all[:n], what)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("nq", [8, 200, 256, 257])
def test_one_pass_group_maxima_topk(eng, dtype, d, nq):
    """More than 16 384 rows: the GEMM_GROUPS epilogue (group and half-tile maxima, hints) and the hierarchical
    selection behind it.  66 tiles, nk = 1 (the prologue issues one tile, its wait is 0) and nk = 3."""
    n = 16640
    db_st, q_st, dbn, qn, ref = _operands(eng, dtype, d, n, Q_MAX)
    tau = eng.score_error_bound(nq, n, d, K)
    _tile_shares_are_large(qn, dbn, tau)
    what = "%s d=%d n=%d q=%d" % (dtype, d, n, nq)
    _check_topk(eng, q_st[:nq], db_st, qn[:nq], dbn, what)
    _check_dense(eng, q_st[:nq], db_st, ref[:nq], tau, what)


# --------------------------------------------------------------------------- split-K: a short last chunk
# (nq, n, d, chunks, K tiles per chunk, K tiles of the last chunk).  split_plan (cosine_topk.hip) cuts K when fewer
# than 256 workgroups would run and d >= 512: it takes the chunk count ns (kchunk = ceil(nk / ns)) that minimises
#   ceil(workgroups * ns / 256) * (1.6 * kchunk + 8) + 2 * ns * (partial bytes) / 3e6 + 5   [us]
# going up in ns and moving only for a gain of 10 %.  300 rows are two database tiles; with one query block that is 2
# workgroups per chunk, one round of the chip for every ns, so the cost falls with kchunk until the 10 % rule stops it:
# at chunks of 5 for the widths below, of 4 for 36 K tiles (9 chunks; the 10 % rule passes over 8 chunks of 5).
# Every shape is planned at 0.30-0.51 of its one-pass cost (19-25 us against 42-77 us), far inside the 10 % rule, so a
# retuned constant moves the chunk count before it moves a shape off split-K -- and the test reads the chunk count back
# from the library (the partial-score room it asks for), so either shows as a failure here and not as a case silently
# run on another path.  A full chunk of 5 runs 3 steady iterations and the 2 tail iterations; the last chunk's 1, 2, 3
# K tiles are what the prologue and the tail must get right on their own.  (300 rows x 2304 is 9 chunks of 4 at q = 8:
# a last chunk as long as the others, kept as the even case.)
SPLIT_SHAPES = [
    (8, 300, 1344, 5, 5, 1),        # 21 K tiles
    (8, 300, 1728, 6, 5, 2),        # 27
    (8, 300, 2112, 7, 5, 3),        # 33
    (256, 300, 1984, 7, 5, 1),      # 31, unmasked query block
    (200, 300, 1728, 6, 5, 2),      # 27, MASKQ with three live column blocks
    (257, 300, 2752, 9, 5, 3),      # 43, two query blocks (4 workgroups per chunk)
    (8, 300, 2304, 9, 4, 4),        # 36, no short chunk
]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("nq,n,d,chunks,kchunk,last", SPLIT_SHAPES)
def test_split_k_short_last_chunk(eng, dtype, nq, n, d, chunks, kchunk, last):
    nk = d // 64
    assert (chunks - 1) * kchunk + last == nk and -(-nk // chunks) == kchunk       # the table is consistent
    room = eng.lib.dlc_cosine_scores_workspace_bytes(nq, n, d)                     # chunks * q * (tiles * 256) * 4 bytes
    per_chunk = nq * (-(-n // 256) * 256) * 4
    assert room > 0 and room % per_chunk == 0 and room // per_chunk == chunks, \
        "split_plan no longer cuts %d x %d x %d into %d chunks of %d K tiles (it plans %.2f chunks): pick another " \
        "width from its cost model" % (nq, n, d, chunks, kchunk, room / per_chunk)
    db_st, q_st, dbn, qn, ref = _operands(eng, dtype, d, n, nq)
    tau = eng.score_error_bound(nq, n, d, K)
    _tile_shares_are_large(qn, dbn, tau)
    what = "%s split-K d=%d n=%d q=%d (%d x %d + %d)" % (dtype, d, n, nq, chunks - 1, kchunk, last)
    _check_dense(eng, q_st, db_st, ref, tau, what)
    _check_topk(eng, q_st, db_st, qn, dbn, what)
