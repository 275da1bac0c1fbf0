"""BASELINE.json full sizes on the GPU, through size-independent properties (the
fp64 oracle cannot finish these in seconds): batch invariance, symmetry, agreement
of the all-vs-all kernels with the per-pair entry points and with the oracle on
sampled entries, planted-neighbour recall, sharded == unsharded."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N_FRAMES = 1063            # outdoor_kennedylong (configs[1], configs[2])


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def descriptors(dlc):
    g = torch.Generator(device="cuda")
    g.manual_seed(42)
    x = torch.rand((N_FRAMES, 30, 1681), generator=g, device="cuda", dtype=torch.float64)
    net = dlc.SDAV(seed=2)
    h = net.transform_tensor(x)
    return net, x, h


def test_sdav_encode_kennedylong_batch_invariance(dlc, descriptors):
    """1063 frames in one call == the same frames in chunks (bit-exact), + oracle on one frame."""
    from oracle import sdav as osdav
    net, x, h = descriptors
    assert h.shape == (N_FRAMES * 30, 2500)
    for lo, hi in ((0, 1), (500, 517), (1050, 1063)):
        part = net.transform_tensor(x[lo:hi])
        assert torch.equal(part, h[lo * 30:hi * 30])
    ws, bs = net.get_weights()
    ref = osdav.transform(x[777:778].cpu().numpy(), ws, bs)
    assert np.abs(h[777 * 30:778 * 30].cpu().numpy() - ref).max() < 1e-10
    assert torch.isfinite(h).all() and float(h.min()) >= 0.0 and float(h.max()) <= 1.0


@pytest.mark.parametrize("scale", ["reference", "fan_in"])
def test_sdav_encode_split_mode_kennedylong(dlc, scale):
    """The tolerance mode at the reference's full size, 1063 frames (31 890 rows), both weight regimes, on tiled REAL frames
    and on random ones: descriptor relative L2 against the fp64 encoder (itself held to 1e-10 of the oracle above) below
    north_star's 1e-4; chunks == one batch bit for bit."""
    import real_frames
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    exact = dlc.SDAV(seed=9, weight_scale=scale)
    fast = dlc.SDAV(seed=9, dtype="f16x2", weight_scale=scale)
    for name, x in (("real", real_frames.tiled_patches(dlc, N_FRAMES)),
                    ("random", torch.rand((N_FRAMES, 30, 1681), generator=g, device="cuda", dtype=torch.float64))):
        ref = exact.transform_tensor(x)
        got = fast.transform_tensor(x)
        assert got.shape == ref.shape and got.dtype == torch.float64
        l2 = (got - ref).norm(dim=1) / ref.norm(dim=1)
        print("SDAV f16x2 at 1063 %s frames, %s weights: relative L2 max %.3g median %.3g" % (name, scale, float(l2.max()), float(l2.median())))
        assert float(l2.max()) < 1e-4
        assert torch.equal(fast.transform_tensor(x[500:517]), got[500 * 30:517 * 30])


def test_similarity_matrix_kennedylong_properties(dlc, descriptors):
    from oracle import similarity as osim
    _, _, h = descriptors
    ds = h.reshape(N_FRAMES, 30, 2500)
    calc = dlc.SimilarityCalculator(ds)
    mf = calc.similarity_matrix(as_int64=False)
    mi = calc.similarity_matrix(as_int64=True)
    assert mf.shape == (N_FRAMES, N_FRAMES) and np.array_equal(mf, mf.T) and np.array_equal(mi, mi.T)
    assert np.all(np.diag(mf) == -1) and np.all(np.diag(mi) == -1)
    fin = np.isfinite(mf)
    assert np.array_equal(mi[fin], np.trunc(mf[fin]).astype(np.int64))
    dsn = ds.cpu().numpy()
    score = osim.distinctive_score(osim.average_response(dsn))
    np.testing.assert_allclose(calc._score.cpu().numpy(), score, rtol=1e-12)
    rng = np.random.RandomState(0)
    for _ in range(40):
        i, j = sorted(rng.choice(N_FRAMES, 2, replace=False))
        idx = osim.match_features(dsn[i], dsn[j])
        d = osim.weighted_distances(dsn[i], dsn[j], idx, score)
        with np.errstate(divide="ignore"):
            want = np.sum(10 - 10 * np.log(d))
        assert (np.isinf(want) and mf[i, j] == want) or abs(mf[i, j] - want) <= 1e-9 * abs(want)
        assert calc.similarity_score(dsn[i], dsn[j]) == mf[i, j]          # per-pair entry == matrix entry
    # every entry, against launches that walk other Gram blocks in another order: a frame range scored on its own
    # (same distinctive score) is that range of the full matrix, bit for bit
    eng = calc.engine
    for lo, hi in ((0, 500), (300, 1000), (563, N_FRAMES)):
        sub, _ = eng.sdav_similarity_matrix(ds[lo:hi], calc._score, 10.0, -10.0, want_int64=False)
        assert np.array_equal(sub.cpu().numpy(), mf[lo:hi, lo:hi]), (lo, hi)


def _oracle_pair(dsn, sc, i, j):
    from oracle import similarity as osim
    d = osim.weighted_distances(dsn[i], dsn[j], osim.match_features(dsn[i], dsn[j]), sc)
    with np.errstate(divide="ignore"):
        return np.sum(10 - 10 * np.log(d))


def _both_routes_and_oracle(eng, ds, n_oracle, seed):
    """The arg-min filter (int8 MFMA products + direct fp64 evaluations) and the fp64 Gram form of
    dlc_sdav_similarity_matrix on the same dataset: equal bit for bit; and the oracle (SimilarityCalculator.py:30-49
    restated) on n_oracle frame pairs -- FIRST the pairs the filter reports as holding a directly evaluated arg-min
    (direct_pairs), then random ones.  Returns (direct evaluations, pairs that had one, oracle pairs of that kind)."""
    from oracle import similarity as osim
    n = ds.shape[0]
    score = eng.distinctive_score(ds, 0.5, 0.2)
    stats = torch.zeros((2,), dtype=torch.int64, device=eng.device)
    dmap = torch.empty((n, n), dtype=torch.uint8, device=eng.device)
    f_i8, i_i8 = (t.clone() for t in eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, stats=stats, direct_pairs=dmap))
    f_64, i_64 = eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, force_f64=True)
    assert torch.equal(f_i8.isnan(), f_64.isnan()) and torch.equal(torch.nan_to_num(f_i8), torch.nan_to_num(f_64))
    assert torch.equal(i_i8, i_64)
    assert int(stats[1]) == 0
    mf = f_i8.cpu().numpy()
    direct = np.argwhere(dmap.cpu().numpy() != 0)
    assert np.all(direct[:, 0] < direct[:, 1]) if len(direct) else True
    rng = np.random.RandomState(seed)
    pairs = [tuple(p) for p in direct[rng.permutation(len(direct))[:n_oracle * 2 // 3]]]
    n_direct = len(pairs)
    while len(pairs) < n_oracle:
        i, j = sorted(rng.choice(n, 2, replace=False))
        pairs.append((i, j))
    dsn, sc = ds.cpu().numpy(), score.cpu().numpy()
    np.testing.assert_allclose(sc, osim.distinctive_score(osim.average_response(dsn)), rtol=1e-12)
    for i, j in pairs:
        want = _oracle_pair(dsn, sc, i, j)
        assert (np.isinf(want) and mf[i, j] == want) or abs(mf[i, j] - want) <= 1e-9 * abs(want), (i, j, mf[i, j], want)
    return int(stats[0]), len(direct), n_direct


@pytest.mark.parametrize("kind", ["encoder", "saturated", "uniform", "twins"])
def test_similarity_filter_equals_fp64_route_full_size(dlc, descriptors, kind):
    """configs[1] at the reference's full shape, 1063 x 30 x 2500 (564 453 frame pairs, 508 M arg-mins): the int8 arg-min
    filter == the fp64 Gram form bit for bit, and == the oracle on 300 pairs led by the ones with a directly evaluated
    arg-min -- on encoder outputs, sigmoid-saturated values (most entries within 1e-9 of 0 or 1), uniform values, and
    saturated data with copies of patches inside frames and of whole frames (exact ties: hashes, first index)."""
    eng = dlc.default_engine()
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 + len(kind))
    shape = (N_FRAMES, 30, 2500)
    if kind == "encoder":
        ds = descriptors[2].reshape(shape)
    elif kind == "uniform":
        ds = torch.rand(shape, generator=g, device="cuda", dtype=torch.float64)
    else:
        ds = torch.sigmoid(35.0 * torch.randn(shape, generator=g, device="cuda", dtype=torch.float64))
        if kind == "twins":
            ds[:, 1] = ds[:, 0]; ds[:, 7] = ds[:, 6]; ds[::3, 29] = ds[::3, 11]       # copies inside frames
            ds[100] = ds[5]; ds[1062] = ds[1061]; ds[500, :10] = ds[20, :10]          # copies of frames / half frames
            ds[300:310, 4] = 0.0; ds[300:310, 5] = 0.0; ds[700, 2] = 1.0              # blank patches
    direct, pairs, checked = _both_routes_and_oracle(eng, ds, 300, seed=len(kind))
    print("similarity filter, %s data: %d of %d arg-mins evaluated directly, in %d frame pairs (%d of them among the 300 "
          "oracle pairs)" % (kind, direct, N_FRAMES * (N_FRAMES - 1) // 2 * 30, pairs, checked))


@pytest.mark.parametrize("n,p,h", [(500, 30, 2560), (700, 16, 1024), (400, 32, 2048)])
def test_similarity_filter_equals_fp64_route_unpadded_k(dlc, n, p, h):
    """Hundreds of frames with a descriptor width that is a multiple of 256: the product kernel's LAST k-step is all data
    (at H = 2500 it is 60 columns of zero padding, which hides an accumulator read too early behind the last MFMAs --
    docs/LAB.md 9.2), for 2, 4 and 2 frames per 64-column unit.  Filter == fp64 Gram form bit for bit, == the oracle on
    60 pairs led by the directly evaluated ones."""
    eng = dlc.default_engine()
    g = torch.Generator(device="cuda")
    g.manual_seed(n + p + h)
    ds = torch.sigmoid(6.0 * torch.randn((n, p, h), generator=g, device="cuda", dtype=torch.float64))
    _both_routes_and_oracle(eng, ds, 60, n)


@pytest.mark.parametrize("n_frames", [220, N_FRAMES])
def test_similarity_filter_real_frames_tiled(dlc, n_frames):
    """Real-image statistics at the reference's full size: the 20 real frames tiled to 220 and to 1063 frames
    (create_similarity_matrix.py:23-38 runs on the 1063 frames of outdoor_kennedylong; the repo carries 20 of them), encoded
    with the reference's N(0,1) initialiser, where real images saturate the encoder, AND with 1/sqrt(fan_in) weights, where
    every descriptor column stays within 1e-3 of its own mean while the means spread over [0.15, 0.88] -- the data on which
    r03's filter, quantising against ONE global range, sent every arg-min (722 700 of 722 700 at 220 frames) to the direct
    evaluation.  Filter == fp64 Gram form bit for bit, == the oracle on 300 pairs led by the directly evaluated ones; the
    filter keeps the call (stats[1] = 0) and decides all but a small fraction of the arg-mins itself."""
    import config1_common as c1
    import real_frames
    eng = dlc.default_engine()
    xs = real_frames.tiled_patches(dlc, n_frames)
    n = xs.shape[0]
    assert n == n_frames
    for scale in ("reference", "fan_in"):
        net = dlc.SDAV(seed=c1.SEED, weight_scale=scale)
        ds = net.transform_tensor(xs).reshape(n, 30, 2500)
        direct, pairs, checked = _both_routes_and_oracle(eng, ds, 300, seed=3)
        total = n * (n - 1) // 2 * 30
        print("similarity filter, %d tiled real frames, %s weights: %d of %d arg-mins evaluated directly (%.3f %%) in %d frame "
              "pairs (%d among the oracle pairs)" % (n, scale, direct, total, 100.0 * direct / total, pairs, checked))
        assert direct <= 0.02 * total, (scale, direct, total)


def test_similarity_matrix_two_gram_chunks(dlc):
    """More frames than one 8 GiB Gram block holds (1500 x 30 patches: row chunks of 768 + 731 frames, the second
    launch's triangle starting at row0 > 0): == frame ranges scored alone, bit for bit, and the oracle on sampled pairs."""
    from oracle import similarity as osim
    eng = dlc.default_engine()
    n, p, h = 1500, 30, 64
    g = torch.Generator(device=eng.device); g.manual_seed(21)
    ds = torch.rand((n, p, h), generator=g, device=eng.device, dtype=torch.float64)
    score = eng.distinctive_score(ds, 0.5, 0.2)
    mf, _ = eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, want_int64=False)
    mf = mf.cpu().numpy()
    assert np.array_equal(mf, mf.T) and np.all(np.diag(mf) == -1)
    for lo, hi in ((0, 760), (700, n), (760, 1300)):
        sub, _ = eng.sdav_similarity_matrix(ds[lo:hi], score, 10.0, -10.0, want_int64=False)
        assert np.array_equal(sub.cpu().numpy(), mf[lo:hi, lo:hi]), (lo, hi)
    dsn, sc = ds.cpu().numpy(), score.cpu().numpy()
    rng = np.random.RandomState(1)
    for _ in range(8):
        i, j = sorted(rng.choice(n, 2, replace=False))
        d = osim.weighted_distances(dsn[i], dsn[j], osim.match_features(dsn[i], dsn[j]), sc)
        want = np.sum(10 - 10 * np.log(d))
        assert abs(mf[i, j] - want) <= 1e-9 * abs(want)


@pytest.mark.parametrize("n,p,h", [(300, 13, 64), (420, 7, 96), (257, 30, 66), (129, 32, 80)])
def test_similarity_matrix_odd_patch_counts(dlc, n, p, h):
    """Patch counts that do not divide the Gram tiles (the wanted-block walk steps a remainder per block column), sizes
    that put the Gram on the LDS-DMA kernel: == the oracle on sampled pairs, == frame ranges scored alone."""
    from oracle import similarity as osim
    eng = dlc.default_engine()
    g = torch.Generator(device=eng.device); g.manual_seed(n + p)
    ds = torch.rand((n, p, h), generator=g, device=eng.device, dtype=torch.float64)
    score = eng.distinctive_score(ds, 0.5, 0.2)
    mf, _ = eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, want_int64=False)
    mf = mf.cpu().numpy()
    assert np.array_equal(mf, mf.T) and np.all(np.diag(mf) == -1)
    for lo, hi in ((0, n // 2), (n // 3, n), (n // 2 - 5, n // 2 + 40)):
        sub, _ = eng.sdav_similarity_matrix(ds[lo:hi], score, 10.0, -10.0, want_int64=False)
        assert np.array_equal(sub.cpu().numpy(), mf[lo:hi, lo:hi]), (lo, hi)
    dsn, sc = ds.cpu().numpy(), score.cpu().numpy()
    rng = np.random.RandomState(2)
    for _ in range(10):
        i, j = sorted(rng.choice(n, 2, replace=False))
        d = osim.weighted_distances(dsn[i], dsn[j], osim.match_features(dsn[i], dsn[j]), sc)
        want = np.sum(10 - 10 * np.log(d))
        assert abs(mf[i, j] - want) <= 1e-9 * abs(want)


def test_distance_matrix_kennedylong_properties(dlc):
    from oracle import distance as odist
    rng = np.random.RandomState(1)
    desc = rng.randint(-128, 128, size=(N_FRAMES, 2243)).astype(np.int8)
    m = dlc.DistanceCalculator.distance_matrix(desc)
    assert m.shape == (N_FRAMES, N_FRAMES) and np.array_equal(m, m.T) and np.all(np.diag(m) == 0)
    for _ in range(50):
        i, j = rng.randint(0, N_FRAMES, 2)
        assert m[i, j] == odist.calculate_distance(desc[i], desc[j])
    assert m.max() <= 8 * 2243


def test_cosine_config4_shape_properties(dlc):
    """configs[3]: 100k x 4096 DB, 256 queries: recall@1 on planted neighbours, self-match,
    8 row shards + merge == one shard."""
    eng = dlc.default_engine()
    n, d, nq, k = 100_000, 4096, 256, 20
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    x = torch.rand((n, d), generator=g, device="cuda", dtype=torch.float32)
    db = eng.normalize(x, "bf16", center=True)
    pi = torch.randperm(n, generator=g, device="cuda")[:nq]
    q = eng.normalize(x[pi] + 0.17 * torch.randn((nq, d), generator=g, device="cuda"), "bf16", center=True)
    del x
    top = eng.match_topk(q, db, k, details=True)
    s, i = top.scores, top.idx
    assert torch.equal(i[:, 0], pi)                                     # recall@1 = 1
    assert torch.all(s[:, :-1] >= s[:, 1:])                             # sorted
    assert int(top.status.max()) in (0, 2)
    s_self, i_self = eng.match_topk(db[pi], db, 1)
    assert torch.equal(i_self[:, 0], pi) and float((s_self - 1).abs().max()) < 5e-3
    for parts in (4, 8):                # 25 000-row shards: the whole database's plan; 12 500-row shards: the small-database plan
        ps, pidx = [], []
        for r in range(parts):
            lo, hi = dlc.shard_bounds(n, parts, r)
            t = eng.match_topk(q, db[lo:hi], k, row_offset=lo, details=True)
            ps.append(t.scores_f64.clone()), pidx.append(t.idx.clone())
        m = eng.topk_merge(torch.stack(ps), torch.stack(pidx), details=True)
        assert torch.equal(m.idx, i) and torch.equal(m.scores_f64, top.scores_f64) and torch.equal(m.scores, s)   # bit for bit
    # exact scores of the returned rows, recomputed in fp64 on the host
    rows = db[i[:8].reshape(-1)].double().reshape(8, k, d)
    ref = torch.einsum("qkd,qd->qk", rows, q[:8].double())
    assert float((ref - top.scores_f64[:8]).abs().max()) < 1e-12 and float((ref - s[:8].double()).abs().max()) < 1.2e-7


@pytest.mark.parametrize("n", [3_000_000, 3_400_000])
def test_select_kernel_large_shard_paths(dlc, n):
    """nh = n/128 half-tile maxima: 94 KB of LDS at 3.0 M rows (needs the >48 KB attribute), in-place
    global path beyond 96 KB at 3.4 M rows.  Narrow descriptors keep it cheap; result vs torch.
    The rows are N(0,1) vectors of norm ~8 (one of norm ~32), NOT the normaliser's output: the certificate's norm
    precondition (include/dlc.h, NORMS) is met by the database measuring them (stored=True -> norm_bound -> tau_scale), not
    by margin."""
    eng = dlc.default_engine()
    g = torch.Generator(device="cuda")
    g.manual_seed(n)
    db = torch.randn((n, 64), generator=g, device="cuda").to(torch.bfloat16)
    q = torch.randn((8, 64), generator=g, device="cuda").to(torch.bfloat16)
    db[n - 1] = q[0] * 4                       # the very last row must be found
    db[12345] = db[n - 7]                      # an exact tie far apart
    kdb = dlc.KeyframeDatabase(db, stored=True)
    assert float(kdb.norm_bound) >= float(db[n - 1].double().norm()) and float(kdb.tau_scale(q).min()) > 30.0
    s, i = kdb.match_topk(q, 5)
    ref = q.double() @ db.double().T                                    # [8, n] fp64 on the GPU (plumbing: checker only)
    rs, ri = torch.sort(ref, dim=1, descending=True, stable=True)
    assert torch.equal(i, ri[:, :5]) and float((s.double() - rs[:, :5]).abs().max()) < 1e-4
    assert int(i[0, 0]) == n - 1
    p = dlc.MatchPipeline(kdb, 5)                                       # cooperative kernel: always the global path
    s2, i2 = p.result(p.submit(q))
    assert torch.equal(i2, i) and torch.equal(s2, s)


def test_score_gemm_every_element_repeated(dlc):
    """Race screen for the LDS-DMA pipeline of the score GEMM: the dense epilogue exposes EVERY
    accumulator (256 queries x 20 k rows, K = 4096 = 64 K tiles), checked against an fp64 product,
    for several launches on fresh random data (a mis-ordered wait shows up as rare wrong tiles)."""
    eng = dlc.default_engine()
    g = torch.Generator(device="cuda")
    for rep in range(5):
        g.manual_seed(100 + rep)
        n = 20000 + 37 * rep if rep < 4 else 131072 + 5      # the last one: two full dispatch rounds under load
        db = torch.randn((n, 4096), generator=g, device="cuda").to(torch.bfloat16)
        q = torch.randn((256 - rep, 4096), generator=g, device="cuda").to(torch.bfloat16)
        s = eng.cosine_scores(q, db)
        ref = q.double() @ db.double().T
        err = (s.double() - ref).abs().max().item()
        assert err < 2e-3 * 64 ** 0.5, err              # |x| ~ N(0,1): fp32 accumulation of 4096 products
        rel = ((s.double() - ref).abs() / (ref.abs() + 64.0)).max().item()
        assert rel < 1e-5, rel


def test_cosine_config5_fp16_one_million_rows(dlc):
    """configs[4]: 1 M x 4096 fp16 key-frames, 256 queries, top-20, on one GPU.  Planted-neighbour recall,
    8 row shards + merge == unsharded (bit for bit: 125 000-row shards and the whole take the same plan),
    the MatchPipeline result == the one-shot call, and for a sample of queries the exact top-20 of an fp64
    product over ALL 1 M rows (computed on the GPU in row chunks -- the checker, not the product)."""
    eng = dlc.default_engine()
    n, d, nq, k, chunk = 1_000_000, 4096, 256, 20, 50_000
    g = torch.Generator(device="cuda")
    g.manual_seed(2025)
    pi = torch.randperm(n, generator=g, device="cuda")[:nq]
    db = torch.empty((n, d), dtype=torch.float16, device="cuda")
    planted = torch.empty((nq, d), dtype=torch.float32, device="cuda")
    for c0 in range(0, n, chunk):
        x = torch.rand((chunk, d), generator=g, device="cuda", dtype=torch.float32)
        sel = torch.nonzero((pi >= c0) & (pi < c0 + chunk)).flatten()
        planted[sel] = x[pi[sel] - c0]
        eng.normalize(x, "f16", center=True, out=db[c0:c0 + chunk])
        del x
    q = eng.normalize(planted + 0.17 * torch.randn((nq, d), generator=g, device="cuda"), "f16", center=True)
    top = eng.match_topk(q, db, k, details=True)
    s, i = top.scores, top.idx
    assert torch.equal(i[:, 0], pi)                                     # recall@1 = 1.0
    assert torch.all(s[:, :-1] >= s[:, 1:]) and int(i.min()) >= 0 and int(i.max()) < n
    print("config 5: %d of %d queries certified at once" % (int((top.status == 0).sum()), nq))
    # 8 shards (one rank's 125 000 rows each) + merge == unsharded
    ps, pidx = [], []
    for r in range(8):
        lo, hi = dlc.shard_bounds(n, 8, r)
        t = eng.match_topk(q, db[lo:hi], k, row_offset=lo, details=True)
        ps.append(t.scores_f64.clone()), pidx.append(t.idx.clone())
    m = eng.topk_merge(torch.stack(ps), torch.stack(pidx), details=True)
    assert torch.equal(m.idx, i) and torch.equal(m.scores, s) and torch.equal(m.scores_f64, top.scores_f64)
    # two-stream pipeline (what bench.py --pipeline runs) == one-shot
    pipe = dlc.MatchPipeline(dlc.KeyframeDatabase(db, dtype="f16", stored=True), k)
    s2, i2 = pipe.result(pipe.submit(q))
    assert torch.equal(i2, i) and torch.equal(s2, s)
    # sampled queries against the fp64 scores of the whole database
    sample = torch.tensor([0, 1, 17, 100, 128, 200, 254, 255], device="cuda")
    qs = q[sample].double()
    ref = torch.empty((sample.numel(), n), dtype=torch.float64, device="cuda")
    for c0 in range(0, n, chunk):
        ref[:, c0:c0 + chunk] = qs @ db[c0:c0 + chunk].double().T
    rs, ri = torch.sort(ref, dim=1, descending=True, stable=True)
    assert torch.equal(i[sample], ri[:, :k])
    assert float((top.scores_f64[sample] - rs[:, :k]).abs().max()) < 1e-12
    assert float((s[sample].double() - rs[:, :k]).abs().max()) < 1.2e-7


def test_cnn_vtl_transform_kennedylong_multi_chunk(dlc):
    """configs[2]: CnnVtl.transform on 1063 frames of 192x240, in one chunk (the default) and in three of 355 / 354 /
    354 frames inside the call == the same frames encoded range by range and frame by frame, bit for bit; == the
    oracle on sampled frames."""
    from oracle import cnn_vtl as ocnn
    eng = dlc.default_engine()
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    frames = torch.randint(0, 256, (N_FRAMES, 192, 240, 3), generator=g, device="cuda").to(torch.float64)
    net = dlc.CnnVtl(input_shape=[N_FRAMES, 192, 240, 3], seed=5, mask_seed=9, frame_chunk=504)
    d = net.transform_tensor(frames)
    whole = dlc.CnnVtl(input_shape=[N_FRAMES, 192, 240, 3], seed=5, mask_seed=9)
    assert whole.frame_chunk >= N_FRAMES
    assert torch.equal(whole.transform_tensor(frames), d)
    del whole
    assert d.shape == (N_FRAMES, net.columns.size) and d.dtype == torch.int8 and net.columns.size <= 2243
    for lo, hi in ((0, 504), (504, 1008), (1008, 1063), (503, 505), (1062, 1063), (700, 701)):
        assert torch.equal(net.transform_tensor(frames[lo:hi]), d[lo:hi]), (lo, hi)
    small = dlc.CnnVtl(input_shape=[N_FRAMES, 192, 240, 3], seed=5, mask_seed=9, frame_chunk=100)
    assert torch.equal(small.transform_tensor(frames[400:650]), d[400:650])
    ws, bs = ocnn.init_weights(5)
    cols = ocnn.column_indices(net.layer_sizes, 99.59, seed=9)
    pick = [0, 503, 504, 1007, 1008, 1062]
    ref = ocnn.transform(frames[pick].cpu().numpy(), ws, bs, cols)
    assert np.array_equal(d[pick].cpu().numpy(), ref)
    # the distance matrix over these descriptors: symmetric, zero diagonal, sampled entries == the oracle
    from oracle import distance as odist
    m = dlc.DistanceCalculator.distance_matrix(d)
    dn = d.cpu().numpy()
    assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0)
    rng = np.random.RandomState(3)
    for _ in range(40):
        a, b = rng.randint(0, N_FRAMES, 2)
        assert m[a, b] == odist.calculate_distance(dn[a], dn[b])


def test_config2_and_config3_on_tiled_real_frames(dlc):
    """configs[1] (cosine over the flattened SDAV descriptors) and configs[2] (cnn_vtl) at the reference's full size on
    REAL-image statistics: the 20 real frames tiled to 1063 (exact copies, copies with pixels moved by one step, blanked
    blocks).  cnn_vtl: every int8 byte of sampled frames == the oracle, exact copies give identical descriptors, the
    1063 x 1063 distance matrix is symmetric with a zero diagonal, zero between exact copies, == the oracle on sampled
    pairs.  Cosine: the top-20 of every frame over the 75 008-wide place descriptors == the oracle's, all 21 260 slots
    (scores crowd: a frame, its copies and near copies), the exact copies tie and go by index.  (A frame's best match
    need not be itself: rows are unit vectors ROUNDED to bf16, and a near copy whose rounded row is a hair longer scores
    higher -- the oracle, which works on the stored rows, agrees.)"""
    import real_frames
    from oracle import cnn_vtl as ocnn, cosine as ocos, distance as odist
    eng = dlc.default_engine()
    frames = real_frames.tiled_bgr_frames(dlc, N_FRAMES)
    net = dlc.CnnVtl(input_shape=[N_FRAMES, 192, 240, 3], seed=5, mask_seed=9)
    d = net.transform_tensor(frames)
    assert d.shape == (N_FRAMES, net.columns.size) and d.dtype == torch.int8
    ws, bs = ocnn.init_weights(5)
    cols = ocnn.column_indices(net.layer_sizes, 99.59, seed=9)
    pick = [0, 19, 20, 41, 77, 500, 1062]
    assert np.array_equal(d[pick].cpu().numpy(), ocnn.transform(frames[pick].cpu().numpy(), ws, bs, cols))
    assert torch.equal(d[:20], d[20:40]) and torch.equal(d[:20], d[40:60])          # copies 0 and 1 are exact
    m = dlc.DistanceCalculator.distance_matrix(d)
    dn = d.cpu().numpy()
    assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0)
    assert np.all(m[np.arange(20), np.arange(20) + 20] == 0) and np.all(m[np.arange(20), np.arange(20) + 40] == 0)
    rng = np.random.RandomState(4)
    for _ in range(40):
        a, b = rng.randint(0, N_FRAMES, 2)
        assert m[a, b] == odist.calculate_distance(dn[a], dn[b])
    del frames, d, net

    xs = real_frames.tiled_patches(dlc, N_FRAMES)
    h = dlc.SDAV(seed=2).transform_tensor(xs)
    db = dlc.KeyframeDatabase(h.reshape(N_FRAMES, 30 * 2500), dtype="bf16", center=True)
    rows = db.rows
    top = eng.match_topk(rows, rows, 20, details=True)
    rh = rows.float().cpu().numpy().astype(np.float64)
    es, ei = ocos.topk_from_scores(ocos.scores(rh, rh), 20)
    resolved = int((top.status == 2).sum())
    print("config-2 top-20 on tiled real frames: %d of %d queries resolved by the exhaustive pass" % (resolved, N_FRAMES))
    assert np.array_equal(top.idx.cpu().numpy(), ei)                               # identical indices, all 21 260 slots
    assert np.abs(top.scores_f64.cpu().numpy() - es).max() < 1e-12
    # frame f and its exact copies f + 20, f + 40 are the same stored row: they tie in every other frame's list and go by index
    ti = top.idx.cpu().numpy()
    for f in range(20):
        for q in (100 + f, 500 + f):
            pos = [int(np.nonzero(ti[q] == r)[0][0]) for r in (f, f + 20, f + 40) if (ti[q] == r).any()]
            assert pos == sorted(pos)


def test_cosine_matrix_config2_dense_full(dlc, descriptors):
    """configs[1]: the FULL 1063 x 1063 cosine matrix over the flattened 75 000-d SDAV place descriptors
    (stored width 75 008, split-K) against the fp64 oracle on sampled rows, its symmetry and unit diagonal,
    and the top-20 read off it (small-database plan) against the oracle's exact top-20 for every frame."""
    from oracle import cosine as ocos
    eng = dlc.default_engine()
    _, _, h = descriptors
    place = h.reshape(N_FRAMES, 30 * 2500)
    db = dlc.KeyframeDatabase(place, dtype="bf16", center=True)
    rows = db.rows
    assert rows.shape == (N_FRAMES, 75008)
    s = eng.cosine_scores(rows, rows)
    assert s.shape == (N_FRAMES, N_FRAMES)
    assert torch.equal(s, eng.cosine_scores(rows, rows))                 # chunk-ordered reduction: reproducible
    assert float((s - s.T).abs().max()) == 0.0                          # same products, same order, both ways
    assert float((torch.diagonal(s) - 1).abs().max()) < 5e-3
    rh = rows.float().cpu().numpy().astype(np.float64)
    pick = np.array([0, 1, 255, 256, 511, 777, 1024, 1062])
    ref = ocos.scores(rh[pick], rh)
    assert np.abs(s[pick].cpu().numpy() - ref).max() < 2e-5
    assert np.abs(s[pick].cpu().numpy() - ref).max() < eng.lib.dlc_cosine_score_error_bound(N_FRAMES, N_FRAMES, 75008, 20)
    top = eng.match_topk(rows, rows, 20, details=True)
    ts, ti = top.scores, top.idx
    full = ocos.scores(rh, rh)
    es, ei = ocos.topk_from_scores(full, 20)
    # 21 260 slots over crowded scores (untrained encoder on random frames: every frame looks alike): the order is
    # decided on fp64 re-scores, queries whose k-th score the certificate cannot clear go through the exhaustive pass
    resolved = int((top.status == 2).sum())
    print("config-2 top-20: %d of %d queries resolved by the exhaustive pass" % (resolved, N_FRAMES))
    assert np.array_equal(ti.cpu().numpy(), ei)                         # identical indices, all 21 260 slots
    assert np.abs(top.scores_f64.cpu().numpy() - es).max() < 1e-12 and np.abs(ts.cpu().numpy() - es).max() < 1.2e-7
    assert np.array_equal(ti[:, 0].cpu().numpy(), np.arange(N_FRAMES))  # every frame's best match is itself


def test_gemm_dma_every_element_repeated(dlc):
    """Race screen for the LDS-DMA ring of the fp64 GEMM (a mis-ordered wait or a stage refilled too early shows up
    as rare wrong tiles): every output element of several launches on fresh random data against torch's fp64 product,
    at the SDAV layer shape (K = 2500: 157 K tiles, a tail of 4), a convolution shape through the conv entry point
    (SAME padding: zero-page pieces) and a Gram-like [N,K] product."""
    from deeploopcloser_amd import _lib as L
    eng = dlc.default_engine()
    g = torch.Generator(device="cuda")
    for rep in range(3):
        g.manual_seed(500 + rep)
        m = 31890 + 17 * rep
        a = torch.rand((m, 2500), generator=g, device="cuda", dtype=torch.float64)
        w = torch.randn((2500, 2500), generator=g, device="cuda", dtype=torch.float64) / 50.0
        b = torch.randn((2500,), generator=g, device="cuda", dtype=torch.float64)
        got = eng.gemm_bias_act(a, w, b, act=L.DLC_ACT_SIGMOID)
        ref = torch.sigmoid(a @ w + b)
        assert float((got - ref).abs().max()) < 1e-12, rep
        del a, w, got, ref
        # conv3-like: 384 frames of 10 x 13 x 256 -> 384 filters, 3 x 3 SAME (M = 49 920 rows, K = 2304)
        x = torch.randn((384 + rep, 10, 13, 256), generator=g, device="cuda", dtype=torch.float64)
        k = torch.randn((3 * 3 * 256, 384), generator=g, device="cuda", dtype=torch.float64) / 48.0
        bias = torch.randn((384,), generator=g, device="cuda", dtype=torch.float64)
        y = eng.conv2d(x, k, bias, 3, 3, 1, 1, 1, 10, 13, L.DLC_ACT_RELU)
        ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), k.reshape(3, 3, 256, 384).permute(3, 2, 0, 1), bias, padding=1)
        ref = torch.relu(ref).permute(0, 2, 3, 1)
        assert float((y - ref).abs().max()) < 1e-11, rep
        del x, y, ref
        p = torch.randn((20000 + 30 * rep, 1000), generator=g, device="cuda", dtype=torch.float64)
        got = eng.gemm_bias_act(p[:12800], p, None, act=L.DLC_ACT_NONE, blayout=L.DLC_B_NK)
        assert float((got - p[:12800] @ p.T).abs().max()) < 1e-10, rep
        del p, got


@pytest.mark.parametrize("scale", ["reference", "fan_in"])
def test_split_encoder_every_element_repeated(dlc, scale):
    """Race screen for the tolerance-mode encoder's LDS ring (dlc_sdav_encode_split: 2 1/2 slices with counted waits,
    a stale slot shows up as a few wrong elements): the reference's 1063 frames (31 890 rows) through 1681 -> 2500 x 5,
    three launches on fresh data, every element against the fp64 chain within the propagated bound of
    tests/precision_bounds.py; a repeat on the same data gives the same bits."""
    import precision_bounds as pb
    eng = dlc.default_engine()
    g = torch.Generator(device="cuda")
    dims = [1681] + [2500] * 5
    worst = 0.0
    for rep in range(3):
        g.manual_seed(900 + rep)
        x = torch.rand((31890, 1681), generator=g, device="cuda", dtype=torch.float64)
        ws = [torch.randn((k, n), generator=g, device="cuda", dtype=torch.float64) / (k ** 0.5 if scale == "fan_in" else 1.0)
              for k, n in zip(dims[:-1], dims[1:])]
        bs = [0.1 * torch.randn((n,), generator=g, device="cuda", dtype=torch.float64) for n in dims[1:]]
        panels = eng.sdav_split_panels(ws)
        got = eng.sdav_encode_split(x, dims, panels, bs)
        again = eng.sdav_encode_split(x, dims, panels, bs)
        assert torch.equal(got, again), rep
        (h, e), = pb.split_chain_bound(x, ws, bs)[-1:]
        worst = max(worst, pb.ratio(got - h, e))
        assert worst <= 1.0, (rep, worst)
        del x, ws, panels, got, again, h, e
    print("split encoder, 31 890 rows, %s weights, 3 launches: worst err/bound %.3g" % (scale, worst))


@pytest.mark.parametrize("batch", [32, 50])
def test_streaming_detector_kennedylong_two_batches_in_flight(dlc, descriptors, batch):
    """configs[1]'s 1063 frames arriving in batches, with the REFERENCE's similarity (create_similarity_matrix.py:34-38 as a
    robot runs it): SdavLoopClosureDetector.submit / result (the strip's product kernel alone on the second stream, the
    small kernels of the neighbouring batches beside it) returns the lists of query_and_insert bit for bit, and both equal
    a stable ranking of the all-vs-all call's columns on sampled frames."""
    net, x, h = descriptors
    eng = dlc.default_engine()
    desc = h.reshape(N_FRAMES, 30, 2500)
    score = eng.distinctive_score(desc, 0.5, 0.2)
    k, excl = 5, 30
    plain = dlc.SdavLoopClosureDetector(score, patches=30, width=2500, k=k, exclusion=excl, capacity=N_FRAMES)
    piped = dlc.SdavLoopClosureDetector(score, patches=30, width=2500, k=k, exclusion=excl, capacity=N_FRAMES)
    want, got, prev = [], [], None
    for lo in range(0, N_FRAMES, batch):
        want.append(plain.query_and_insert(desc[lo:lo + batch]))
        t = piped.submit(desc[lo:lo + batch])
        if prev is not None:
            got.append(piped.result(prev))
        prev = t
    got.append(piped.result(prev))
    ws, wi = torch.cat([w[0] for w in want]), torch.cat([w[1] for w in want])
    gs, gi = torch.cat([o[0] for o in got]), torch.cat([o[1] for o in got])
    torch.cuda.synchronize()
    assert torch.equal(wi, gi)
    assert torch.equal(torch.nan_to_num(ws, posinf=1e300, neginf=-1e300), torch.nan_to_num(gs, posinf=1e300, neginf=-1e300))
    assert int(piped.stream.stats[1]) == 0 and len(piped) == N_FRAMES
    col = eng.sdav_similarity_matrix(desc, score, 10.0, -10.0, want_int64=False)[0].cpu().numpy()
    gi_h = gi.cpu().numpy()
    for f in range(excl + 1, N_FRAMES, 37):
        c = col[:f - excl, f]
        order = np.lexsort((np.arange(len(c)), -c))[:k]
        assert np.array_equal(gi_h[f, :len(order)], order), f
