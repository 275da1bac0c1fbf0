"""GPU VLAD pooling and k-means (dlc_vlad_assign, dlc_vlad_encode, dlc_kmeans_step through the raw C ABI; Vlad,
KeyframeDatabase and the CLI on top) against the NumPy restatement of the definition (tests/vlad_oracle.py, pinned by
test_vlad_cpu.py).  The definition fixes every rounding, so every comparison is `==` on the int64 views: zero tolerance.
Inputs carry NaN-filled padding columns that would poison every result if they were read; outputs sit in sentinel-filled
buffers wider than what may be written."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import vlad_oracle as vo

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A
NONE, INTRA = 0, 1


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


def padded(e, m, pad):
    """m [rows, H] as the first H columns of a [rows, H + pad] device matrix whose other columns are NaN."""
    buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=torch.float64, device=e.device)
    buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m)).to(e.device)
    return buf


def sentinel_f64(e, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.int64, device=e.device).view(torch.float64)


def sentinel_i32(e, n):
    return torch.full((n,), SENTINEL32, dtype=torch.int32, device=e.device)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def workspace(e, need):
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device=e.device)


def raw_assign(e, xb, H, cb, K, with_dist=True):
    """dlc_vlad_assign into sentinel-framed outputs -> (a int32 [rows], dist words int64 [rows])."""
    rows = xb.shape[0]
    a, d = sentinel_i32(e, rows + 2), sentinel_f64(e, rows + 2)
    rc = e.lib.dlc_vlad_assign(e.ctx, p(xb), rows, H, xb.stride(0), p(cb), K, cb.stride(0), C.c_void_p(a.data_ptr() + 4),
                               C.c_void_p(d.data_ptr() + 8) if with_dist else None, None)
    assert rc == 0, e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    a, d = a.cpu().numpy(), d.view(torch.int64).cpu().numpy()
    assert a[0] == a[-1] == SENTINEL32 and d[0] == d[-1] == SENTINEL
    if not with_dist:
        assert (d == SENTINEL).all()
    return a[1:-1], d[1:-1]


def raw_encode(e, xb, frames, P, H, cb, K, norm, extra=3, with_assign=True):
    """dlc_vlad_encode into a sentinel-filled [frames, K * H + extra] buffer -> (its words int64, a int32 [frames * P])."""
    out = sentinel_f64(e, frames, K * H + extra)
    a = sentinel_i32(e, frames * P) if with_assign else None
    need = e.lib.dlc_vlad_encode_workspace_bytes(frames, P, H, K)
    ws = workspace(e, need)
    rc = e.lib.dlc_vlad_encode(e.ctx, p(xb), frames, P, H, xb.stride(0), p(cb), K, cb.stride(0), norm, p(out), out.stride(0),
                               p(a), p(ws), need, None)
    assert rc == 0, e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    return out.view(torch.int64).cpu().numpy(), (a.cpu().numpy() if with_assign else None)


def same_rows(words, want, KH):
    """The first KH words of every row equal the oracle's bits; the others still hold the sentinel."""
    return (words[:, KH:] == SENTINEL).all() and np.array_equal(words[:, :KH], bits(want))


# ---- assign / encode: the grid ----------------------------------------------------------------------------------------------
# H crosses the LDS chunk of 32 columns (64 | 65), K the register tiles' words (16 | 17: (8, 1) -> (4, 2); 32 | 33 -> (4, 4);
# 64 | 65: a second word tile) and the accumulator tile widths (K <= 32 / 64 / 128 / 256 -> 256 / 128 / 64 / 32 columns: H = 200
# and 300 either side of them); frames * P crosses the row tiles of 64 and 128 (17 * 30 = 510); H = 2049 the tree's 2048 leaves.
GRID = [(H, K) for H in (1, 7, 64, 65, 200) for K in (1, 2, 16, 17, 64, 256)]
EXTRA = [(65, 32), (65, 33), (7, 65), (33, 129), (300, 16), (300, 33), (2049, 1), (2049, 2)]


@pytest.mark.parametrize("H,K", GRID + EXTRA)
def test_assign_and_encode_bits(e, H, K):
    rng = np.random.RandomState(H * 1000 + K)
    c = rng.standard_normal((K, H))
    cb = padded(e, c, 3)
    shapes = [(P, frames) for P in (1, 5, 30) for frames in (1, 3, 17)] if H <= 300 else [(5, 3)]
    for P, frames in shapes:
        x = rng.standard_normal((frames * P, H)) + c[rng.randint(0, K, size=frames * P)] * (rng.rand(frames * P, 1) < 0.5)
        xb = padded(e, x, 5)
        want_a, want_d = vo.assign(x, c)
        a, d = raw_assign(e, xb, H, cb, K)
        assert np.array_equal(a, want_a) and np.array_equal(d, bits(want_d)), (P, frames)
        for norm in (NONE, INTRA):
            want, _ = vo.vlad_encode(x, c, P, norm)
            words, a = raw_encode(e, xb, frames, P, H, cb, K, norm)
            assert np.array_equal(a, want_a), (P, frames, norm)
            assert same_rows(words, want, K * H), (P, frames, norm)


def test_intra_norm_over_three_tree_levels(e):
    """H = 2048 * 2048 + 5: the norm's TREE needs the third level of the LDS fold.  One word and one patch, so the
    definition is R = x - c and R / sqrt(TREE(R * R)), stated here with the oracle's bottom-up TREE."""
    H = 2048 * 2048 + 5
    rng = np.random.RandomState(9)
    x, c = rng.standard_normal((1, H)), rng.standard_normal((1, H))
    R = x[0] - c[0]
    want = R / np.sqrt(vo.tree_pairwise(R * R))
    words, a = raw_encode(e, padded(e, x, 1), 1, 1, H, padded(e, c, 1), 1, INTRA, extra=2)
    assert a.tolist() == [0] and same_rows(words, want[None], H)


def test_ties_duplicates_and_nan_on_the_device(e):
    c = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.25, 0.5]])              # word 2 copies word 0
    x = np.array([[0.5, 0.0], [0.0, 0.0], [np.nan, 1.0], [1.0, 0.0]])
    xb, cb = padded(e, x, 2), padded(e, c, 1)
    a, d = raw_assign(e, xb, 2, cb, 4)
    assert a.tolist() == [0, 0, -1, 1]
    want_a, want_d = vo.assign(x, c)
    assert np.array_equal(a, want_a) and np.array_equal(np.delete(d, 2), np.delete(bits(want_d), 2))
    assert np.isnan(d.view(np.float64)[2])
    a2, _ = raw_assign(e, xb, 2, cb, 4, with_dist=False)
    assert np.array_equal(a2, a)
    for norm in (NONE, INTRA):
        want, _ = vo.vlad_encode(x, c, 4, norm)
        words, a = raw_encode(e, xb, 1, 4, 2, cb, 4, norm)
        assert same_rows(words, want, 8) and a.tolist() == [0, 0, -1, 1]
        assert not np.isnan(words[:, :8].view(np.float64)).any()                 # the NaN row contributes nowhere
        assert (words[0, 4:8] == 0).all()                                        # the copy and the empty word: +0.0
    # many rows on a dyadic grid: ties everywhere, a word at every K-tile seam copied at a higher index
    rng = np.random.RandomState(1)
    for K in (17, 70):
        c = rng.randint(-2, 3, size=(K, 3)) / 2.0
        c[K - 1] = c[0]
        c[16] = c[3]
        x = rng.randint(-4, 5, size=(300, 3)) / 4.0
        want_a, want_d = vo.assign(x, c)
        a, d = raw_assign(e, padded(e, x, 1), 3, padded(e, c, 2), K)
        assert np.array_equal(a, want_a) and np.array_equal(d, bits(want_d))
        assert not (a == K - 1).any() or not (c[:K - 1] == c[K - 1]).all(1).any()
    # +inf can win
    a, d = raw_assign(e, padded(e, np.array([[1.0]]), 1), 1, padded(e, np.array([[np.nan], [np.inf]]), 1), 2)
    assert a.tolist() == [1] and d.view(np.float64)[0] == np.inf


def test_a_frame_does_not_depend_on_its_batch(e):
    rng = np.random.RandomState(2)
    H, K, P, frames = 40, 20, 30, 17
    c, x = rng.standard_normal((K, H)), rng.standard_normal((frames * P, H))
    cb = padded(e, c, 0)
    for norm in (NONE, INTRA):
        whole, _ = raw_encode(e, padded(e, x, 3), frames, P, H, cb, K, norm)
        for lo in range(0, frames, 7):
            hi = min(frames, lo + 7)
            part, _ = raw_encode(e, padded(e, x[lo * P:hi * P], 1), hi - lo, P, H, cb, K, norm, extra=9)
            assert np.array_equal(part[:, :K * H], whole[lo:hi, :K * H])
        for f in (0, 8, 16):
            one, _ = raw_encode(e, padded(e, x[f * P:f * P + P], 0), 1, P, H, cb, K, norm, extra=0, with_assign=False)
            assert np.array_equal(one[0], whole[f, :K * H])


# ---- the k-means step -----------------------------------------------------------------------------------------------------
def raw_step(e, xb, rows, H, cb, K, prev):
    """dlc_kmeans_step into sentinel-framed outputs -> (c_out [K, H] words, a, counts, inertia word, changed)."""
    c_out = sentinel_f64(e, K, H + 2)
    a = sentinel_i32(e, rows + 2)
    counts = torch.full((K + 2,), SENTINEL, dtype=torch.int64, device=e.device)
    inertia = sentinel_f64(e, 3)
    changed = torch.full((3,), SENTINEL, dtype=torch.int64, device=e.device)
    need = e.lib.dlc_kmeans_step_workspace_bytes(rows, H, K)
    ws = workspace(e, need)
    rc = e.lib.dlc_kmeans_step(e.ctx, p(xb), rows, H, xb.stride(0), p(cb), K, cb.stride(0), p(c_out), c_out.stride(0), p(prev),
                               C.c_void_p(a.data_ptr() + 4), C.c_void_p(counts.data_ptr() + 8), C.c_void_p(inertia.data_ptr() + 8),
                               C.c_void_p(changed.data_ptr() + 8), p(ws), need, None)
    assert rc == 0, e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    cw, a, counts = c_out.view(torch.int64).cpu().numpy(), a.cpu().numpy(), counts.cpu().numpy()
    iw, ch = inertia.view(torch.int64).cpu().numpy(), changed.cpu().numpy()
    assert (cw[:, H:] == SENTINEL).all() and a[0] == a[-1] == SENTINEL32 and counts[0] == counts[-1] == SENTINEL
    assert iw[0] == iw[2] == SENTINEL and ch[0] == ch[2] == SENTINEL
    return cw[:, :H], a[1:-1], counts[1:-1], iw[1], int(ch[1])


@pytest.mark.parametrize("rows", [1, 1023, 1024, 1025, 3000])
def test_kmeans_step_bits(e, rows):
    H, K = 33, 8
    rng = np.random.RandomState(rows)
    centres = rng.standard_normal((K, H)) * 2
    x = centres[rng.randint(0, K - 1, size=rows)] + 0.5 * rng.standard_normal((rows, H))      # (word K - 1 far from everything)
    c = centres + 0.3 * rng.standard_normal((K, H))
    c[K - 1] = 40.0                                                   # an empty word keeps its centre
    if rows > 4:
        x[3] = np.nan                                                 # a row of no word
    xb = padded(e, x, 3)
    prev = None
    for step in range(3):                                             # three consecutive steps, each fed the device's own result
        want_c, want_a, want_n, want_s, want_ch = vo.kmeans_step(x, c, None if prev is None else prev.cpu().numpy())
        cw, a, counts, iw, ch = raw_step(e, xb, rows, H, padded(e, c, 1), K, prev)
        assert np.array_equal(a, want_a) and np.array_equal(counts, want_n) and ch == want_ch, step
        assert np.array_equal(cw, bits(want_c)) and iw == bits([want_s])[0], step
        assert counts[K - 1] == 0 and np.array_equal(cw[K - 1], bits(c[K - 1]))
        c = cw.copy().view(np.float64)
        prev = torch.from_numpy(a.copy()).to(e.device)
    assert rows <= K or want_ch < rows


def test_fit_is_deterministic_and_is_the_oracles_lloyd(dlc, e):
    rng = np.random.RandomState(4)
    x = rng.standard_normal((6, 64))[rng.randint(0, 6, size=1500)] + 0.2 * rng.standard_normal((1500, 64))
    a = dlc.Vlad(n_words=8, seed=3).fit(x, iters=6)
    b = dlc.Vlad(n_words=8, seed=3).fit(torch.from_numpy(x).to(e.device).view(50, 30, 64), iters=6)
    ca, cb = a.centroids.cpu().numpy(), b.centroids.cpu().numpy()
    assert np.array_equal(bits(ca), bits(cb)) and a.inertia_ == b.inertia_ and 1 <= a.n_iter_ == len(a.inertia_) <= 6
    assert np.array_equal(bits(ca), bits(vo.lloyd(x, 8, 6, 3)))
    assert all(s1 <= s0 for s0, s1 in zip(a.inertia_, a.inertia_[1:]))


def test_vlad_surface(dlc, e, tmp_path):
    rng = np.random.RandomState(6)
    x = rng.standard_normal((7 * 30, 20))
    v = dlc.Vlad(n_words=5, seed=1).fit(x, iters=4)
    c = v.centroids.cpu().numpy()
    want, want_a = vo.vlad_encode(x, c, 30, INTRA)
    got = v.transform(x)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(want)) and (v.width, v.dim) == (20, 100)
    t = v.transform_tensor(torch.from_numpy(x).to(e.device).view(7, 30, 20))
    assert t.device == e.device and np.array_equal(bits(t.cpu().numpy()), bits(want))
    assert np.array_equal(bits(dlc.vlad_frame_descriptors(x, v).cpu().numpy()), bits(want))
    assert np.array_equal(v.assign(x).cpu().numpy(), want_a)
    path = str(tmp_path / "book.npz")
    v.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["centroids", "inertia", "norm", "seed"] and str(z["norm"]) == "intra" and int(z["seed"]) == 1
    w = dlc.Vlad.load(path)
    assert (w.n_words, w.norm, w.seed, w.inertia_) == (5, "intra", 1, v.inertia_)
    assert np.array_equal(bits(w.transform(x)), bits(want))
    none = dlc.Vlad(n_words=5, norm="none").set_codebook(c)
    assert np.array_equal(bits(none.transform(x)), bits(vo.vlad_encode(x, c, 30, NONE)[0]))
    # engine wrappers: a row-strided view is taken as it is, out= wider than K * H keeps its other columns
    xb = padded(e, x, 4)[:, :20]
    out = sentinel_f64(e, 7, 103)
    r = e.vlad_encode(xb, v.centroids, out=out)
    assert r.data_ptr() == out.data_ptr() and same_rows(out.view(torch.int64).cpu().numpy(), want, 100)
    a, d = e.vlad_assign(xb, v.centroids, with_dist=True)
    assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(bits(d.cpu().numpy()), bits(vo.assign(x, c)[1]))
    for bad in (lambda: dlc.Vlad(n_words=0), lambda: dlc.Vlad(n_words=257), lambda: dlc.Vlad(norm="l2"),
                lambda: dlc.Vlad(n_words=5).transform(x), lambda: v.transform(x[:, :19]), lambda: v.transform(x[:31]),
                lambda: dlc.Vlad(n_words=300 // 2).fit(x[:100]), lambda: v.set_codebook(c[:4]), lambda: v.fit(x, iters=0),
                lambda: e.vlad_encode(xb, v.centroids, norm="l2"), lambda: e.vlad_encode(xb, v.centroids, patches=0),
                lambda: e.vlad_encode(xb, v.centroids, out=out[:, :99]), lambda: e.vlad_assign(xb.float(), v.centroids),
                lambda: e.kmeans_step(xb, v.centroids, prev_assign=torch.zeros(3, dtype=torch.int32, device=e.device))):
        with pytest.raises(ValueError):
            bad()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_every_refused_argument_writes_nothing(dlc, e):
    L = dlc._lib
    rows, H, K, P = 12, 6, 3, 4
    frames = rows // P
    rng = np.random.RandomState(7)
    xb, cb = padded(e, rng.standard_normal((rows, H)), 2), padded(e, rng.standard_normal((K, H)), 2)
    out, c_out = sentinel_f64(e, frames, K * H + 2), sentinel_f64(e, K, H)
    a, d = sentinel_i32(e, rows), sentinel_f64(e, rows)
    counts = torch.full((K,), SENTINEL, dtype=torch.int64, device=e.device)
    inertia, changed = sentinel_f64(e, 1), torch.full((1,), SENTINEL, dtype=torch.int64, device=e.device)
    prev = torch.zeros(rows, dtype=torch.int32, device=e.device)
    ws = workspace(e, max(e.lib.dlc_vlad_encode_workspace_bytes(frames, P, H, K), e.lib.dlc_kmeans_step_workspace_bytes(rows, H, K)) + 64)
    ldx, ldc = xb.stride(0), cb.stride(0)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    A, S, W = L.DLC_ERR_BAD_ARG, L.DLC_ERR_BAD_SHAPE, L.DLC_ERR_WORKSPACE

    def assign(x=p(xb), rows=rows, H=H, ldx=ldx, c=p(cb), K=K, ldc=ldc, a_=p(a), d_=p(d)):
        return e.lib.dlc_vlad_assign(e.ctx, x, rows, H, ldx, c, K, ldc, a_, d_, None)

    def encode(x=p(xb), frames=frames, P=P, H=H, ldx=ldx, c=p(cb), K=K, ldc=ldc, norm=INTRA, o=p(out), ld_out=out.stride(0),
               a_=p(a), w=p(ws), wb=ws.numel()):
        return e.lib.dlc_vlad_encode(e.ctx, x, frames, P, H, ldx, c, K, ldc, norm, o, ld_out, a_, w, wb, None)

    def step(x=p(xb), rows=rows, H=H, ldx=ldx, c=p(cb), K=K, ldc=ldc, co=p(c_out), ldco=H, pv=p(prev), a_=p(a), n=p(counts),
             s=p(inertia), ch=p(changed), w=p(ws), wb=ws.numel()):
        return e.lib.dlc_kmeans_step(e.ctx, x, rows, H, ldx, c, K, ldc, co, ldco, pv, a_, n, s, ch, w, wb, None)

    cases = [
        (assign, dict(x=None), A), (assign, dict(c=None), A), (assign, dict(a_=None), A), (assign, dict(rows=0), A),
        (assign, dict(H=0), A), (assign, dict(K=0), A), (assign, dict(ldx=H - 1), A), (assign, dict(ldc=H - 1), A),
        (assign, dict(x=off(xb, 4)), A), (assign, dict(a_=off(a, 2)), A), (assign, dict(d_=off(d, 4)), A),
        (assign, dict(K=257), S), (assign, dict(rows=1 << 31), S), (assign, dict(H=1 << 30, ldx=1 << 30, ldc=1 << 30), S),
        (encode, dict(x=None), A), (encode, dict(c=None), A), (encode, dict(o=None), A), (encode, dict(frames=0), A),
        (encode, dict(P=0), A), (encode, dict(H=0), A), (encode, dict(K=0), A), (encode, dict(ldx=H - 1), A),
        (encode, dict(ldc=H - 1), A), (encode, dict(ld_out=K * H - 1), A), (encode, dict(norm=2), A), (encode, dict(norm=-1), A),
        (encode, dict(o=off(out, 4)), A), (encode, dict(a_=off(a, 2)), A),
        (encode, dict(P=1025), S), (encode, dict(K=257), S), (encode, dict(frames=1 << 31), S),
        (encode, dict(w=None), W), (encode, dict(wb=16), W), (encode, dict(w=off(ws, 8)), W),
        (step, dict(x=None), A), (step, dict(c=None), A), (step, dict(co=None), A), (step, dict(a_=None), A), (step, dict(n=None), A),
        (step, dict(s=None), A), (step, dict(ch=None), A), (step, dict(rows=0), A), (step, dict(H=0), A), (step, dict(K=0), A),
        (step, dict(ldx=H - 1), A), (step, dict(ldc=H - 1), A), (step, dict(ldco=H - 1), A), (step, dict(co=off(cb, 0)), A),
        (step, dict(co=off(cb, 8 * ldc), ldco=ldc), A), (step, dict(pv=p(a)), A), (step, dict(co=off(c_out, 4)), A),
        (step, dict(pv=off(prev, 2)), A), (step, dict(K=257), S), (step, dict(rows=1 << 31), S),
        (step, dict(w=None), W), (step, dict(wb=64), W), (step, dict(w=off(ws, 8)), W),
    ]
    before = [t.clone() for t in (xb, cb, prev)]
    for fn, kw, status in cases:
        assert fn(**kw) == status, (fn.__name__, sorted(kw))
        assert e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    for t in (out, c_out, d, inertia):
        assert (t.view(torch.int64) == SENTINEL).all()
    assert (a == SENTINEL32).all() and (counts == SENTINEL).all() and (changed == SENTINEL).all()
    for t, b in zip((xb, cb, prev), before):
        assert torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t, b.view(torch.int64) if b.dtype == torch.float64 else b)
    assert assign() == 0 and encode() == 0 and step() == 0            # and the calls they were derived from are accepted
    torch.cuda.synchronize()


# ---- through the surface -------------------------------------------------------------------------------------------------
def test_planted_scene_through_the_database(dlc, e):
    """Vlad.fit -> transform -> KeyframeDatabase -> match_topk finds the place of all 40 permuted revisits; the
    concatenation through the same calls finds what test_vlad_cpu.py recorded."""
    from test_vlad_cpu import PLANTED_CODEBOOK_SEED, PLANTED_FLAT_HITS, PLANTED_SEED
    db, q = vo.planted_scene(seed=PLANTED_SEED)
    v = dlc.Vlad(n_words=16, seed=PLANTED_CODEBOOK_SEED).fit(db, iters=10)
    assert np.array_equal(bits(v.centroids.cpu().numpy()), bits(vo.lloyd(db.reshape(-1, 64), 16, 10, PLANTED_CODEBOOK_SEED)))

    def hits(d_rows, q_rows):
        kdb = dlc.KeyframeDatabase(d_rows.to(torch.float32), dtype="bf16")
        _, i = kdb.match_topk(kdb.prepare_queries(q_rows.to(torch.float32)), 1)
        return int((i[:, 0].cpu() == torch.arange(40)).sum())
    vlad_hits = hits(v.transform_tensor(db), v.transform_tensor(q))
    flat = hits(dlc.flatten_frame_descriptors(db.reshape(-1, 64)).to(e.device), dlc.flatten_frame_descriptors(q.reshape(-1, 64)).to(e.device))
    print("planted scene on the device: concatenation %d / 40, VLAD %d / 40" % (flat, vlad_hits))
    assert vlad_hits == 40
    assert flat == PLANTED_FLAT_HITS


def run_module(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd." + module, os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_train_vlad_then_loop_closure(dlc, tmp_path):
    book = str(tmp_path / "book.npz")
    res = run_module("train_vlad", "--words", "16", "--iters", "5", "--seed", "2", "--save", book)
    assert res.returncode == 0, res.stdout + res.stderr
    fields = res.stdout.strip().split("\t")
    assert fields[0] == "codebook" and fields[1:7] == ["rows", "510", "words", "16", "width", "2500"], res.stdout
    with np.load(book) as z:
        assert z["centroids"].shape == (16, 2500) and z["centroids"].dtype == np.float64 and np.isfinite(z["centroids"]).all()
        assert 1 <= len(z["inertia"]) <= 5 and int(z["seed"]) == 2
    runs = [run_module("loop_closure", "--network", "sdav", "--metric", "cosine", "--pool", "vlad", "--codebook", book,
                       "--exclusion", "2", "--k", "2", "--batch", "4", "--threshold", "-1") for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
        assert "frames\t17\tkey-frames\t17" in r.stderr
        lines = r.stdout.splitlines()
        assert lines and all(l.startswith("loop\t") and len(l.split("\t")) == 6 for l in lines)
        for l in lines:
            _, frame, _, match, _, score = l.split("\t")
            assert 0 <= int(match) < int(frame) and -1.0001 <= float(score) <= 1.0001
    assert runs[0].stdout == runs[1].stdout
