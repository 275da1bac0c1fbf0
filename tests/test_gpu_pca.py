"""GPU PCA projection (dlc_pca_project through the raw C ABI; Engine.pca_project, Pca, KeyframeDatabase and the CLI on
top) against the NumPy restatement of the definition (tests/pca_oracle.py, pinned by test_pca_cpu.py).  The definition
fixes every rounding, so the projection is compared with `==` on the int64 views: zero tolerance.  Inputs carry
NaN-filled padding columns that would poison every result if they were read; outputs sit in sentinel-filled buffers
wider than what may be written.  Pca.fit is held to 64 x the recorded difference of the oracle's own two routes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import pca_oracle as po
import vlad_oracle as vo

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
AUTO, ONE_PASS, SPLIT = 0, 1, 2
F32, F64 = 2, 3


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


def padded(e, m, pad, dtype=torch.float64):
    """m [rows, H] as the first H columns of a [rows, H + pad] device matrix whose other columns are NaN."""
    buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=dtype, device=e.device)
    buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m)).to(e.device)
    return buf


def sentinel_f64(e, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.int64, device=e.device).view(torch.float64)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device) if a is not None else None


def raw_project(e, xb, D, bb, M, mean, scale, plan, extra=3):
    """dlc_pca_project into a sentinel-filled [rows, M + extra] buffer -> its words int64."""
    rows = xb.shape[0]
    out = sentinel_f64(e, rows, M + extra)
    need = e.lib.dlc_pca_project_workspace_bytes(rows, D, M, plan)
    ws = torch.empty(need, dtype=torch.uint8, device=e.device) if need else None
    assert (need > 0) == (plan == SPLIT) or plan == AUTO
    rc = e.lib.dlc_pca_project(e.ctx, p(xb), rows, D, xb.stride(0), p(mean), F64 if bb.dtype == torch.float64 else F32, p(bb), M,
                               bb.stride(0), p(scale), p(out), out.stride(0), plan, p(ws), need, None)
    assert rc == 0, e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    return out.view(torch.int64).cpu().numpy()


def same_rows(words, want, M):
    """The first M words of every row equal the oracle's bits; the others still hold the sentinel."""
    return (words[:, M:] == SENTINEL).all() and np.array_equal(words[:, :M], bits(want))


def same_up_to_nan(words, want):
    """Equal bits, except that a NaN is any NaN (its payload is the machine's)."""
    got = words.view(np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(words[~nan], bits(want)[~nan])


# ---- the grid ------------------------------------------------------------------------------------------------------------
# The kernel's tiles: rows 2 (rows <= 2) or 8 -- rows 1 | 3 cross the switch, 3, 17, 33 and 65 leave a ragged last tile;
# columns 256, or 512 under ONE_PASS with rows > 2 and M > 256 -- M = 257 crosses the first and selects the second, the
# extra M = 600 crosses it; the LDS slab of 128 columns of x and the 8 basis rows in flight -- D = 7, 1023 (7 slabs + 127)
# and 1025 are ragged in both; the chunk of 1024 -- D = 1023 | 1024 | 1025, 2049 (3 chunks) and 3 * 1024 + 5 (4); a SPLIT
# workgroup spans one chunk, so every case with D > 1024 has partial sums of several workgroups added by the finish.
GRID = [(1, 1, 1), (1, 7, 2), (3, 1023, 63), (3, 1024, 64), (17, 1025, 65), (17, 2049, 130), (33, 3077, 257), (33, 1, 257),
        (65, 7, 1), (65, 1023, 2), (1, 1024, 63), (3, 1025, 64), (17, 2049, 65), (33, 3077, 130), (65, 3077, 257), (1, 2049, 130),
        (9, 1030, 600), (2, 300, 5)]


@pytest.mark.parametrize("rows,D,M", GRID)
def test_projection_bits(e, rows, D, M):
    rng = np.random.RandomState(rows * 100000 + D * 10 + M)
    x, mean, scale = rng.standard_normal((rows, D)), rng.standard_normal(D), rng.uniform(0.5, 2.0, M)
    xb, mu, sc = padded(e, x, 3), dev(e, mean), dev(e, scale)
    for dtype in (np.float64, np.float32):
        basis = rng.standard_normal((D, M)).astype(dtype)
        bb = padded(e, basis, 5, torch.float64 if dtype == np.float64 else torch.float32)
        for with_mean in (False, True):
            for with_scale in (False, True):
                want = po.project(x, basis, mean if with_mean else None, scale if with_scale else None)
                for plan in (ONE_PASS, AUTO, SPLIT):
                    if plan == SPLIT and rows > 64:
                        out = sentinel_f64(e, rows, M)
                        ws = torch.empty(rows * M * 8 * 4 + 256, dtype=torch.uint8, device=e.device)
                        assert e.lib.dlc_pca_project_workspace_bytes(rows, D, M, SPLIT) == 0
                        assert e.lib.dlc_pca_project(e.ctx, p(xb), rows, D, xb.stride(0), None, F64 if dtype == np.float64 else F32,
                                                     p(bb), M, bb.stride(0), None, p(out), M, SPLIT, p(ws), ws.numel(),
                                                     None) == -2                       # DLC_ERR_BAD_SHAPE
                        torch.cuda.synchronize()
                        assert (out.view(torch.int64) == SENTINEL).all()
                        continue
                    words = raw_project(e, xb, D, bb, M, mu if with_mean else None, sc if with_scale else None, plan)
                    assert same_rows(words, want, M), (dtype.__name__, with_mean, with_scale, plan)


def test_reference_width(e):
    """2 x 40 000 x 64: the width of a 16-word VLAD row of the reference's SDAV, 40 chunks."""
    rng = np.random.RandomState(40)
    x, mean, scale = rng.standard_normal((2, 40000)), rng.standard_normal(40000), rng.uniform(0.5, 2.0, 64)
    basis = rng.standard_normal((40000, 64))
    want = po.project(x, basis, mean, scale)
    xb, bb = padded(e, x, 1), padded(e, basis, 1)
    for plan in (ONE_PASS, AUTO, SPLIT):
        assert same_rows(raw_project(e, xb, 40000, bb, 64, dev(e, mean), dev(e, scale), plan), want, 64), plan
    assert e.lib.dlc_pca_project_workspace_bytes(2, 40000, 64, AUTO) >= 2 * 40 * 64 * 8     # AUTO splits a streamed frame


def test_a_row_does_not_depend_on_its_batch(e):
    rng = np.random.RandomState(33)
    D, M = 2500, 70
    x, mean, scale, basis = rng.standard_normal((33, D)), rng.standard_normal(D), rng.uniform(0.5, 2.0, M), rng.standard_normal((D, M))
    want = bits(po.project(x, basis, mean, scale))
    bb, mu, sc = padded(e, basis, 2), dev(e, mean), dev(e, scale)
    for plan in (ONE_PASS, AUTO, SPLIT):
        for slab, pad in ((33, 3), (5, 0), (1, 7)):
            got = np.concatenate([raw_project(e, padded(e, x[lo:lo + slab], pad), D, bb, M, mu, sc, plan)[:, :M]
                                  for lo in range(0, 33, slab)])
            assert np.array_equal(got, want), (plan, slab)


def test_special_values_stay_in_their_row(e):
    rng = np.random.RandomState(5)
    D, M = 1030, 9
    x, mean, basis = rng.standard_normal((6, D)), rng.standard_normal(D), rng.standard_normal((D, M))
    x[1, 3], x[2, 1027], x[3, 500], x[4, 0] = np.nan, np.inf, -np.inf, -0.0
    x[5] = mean                                                       # cancels exactly: every t_d is +0.0
    basis[:, 0] = -np.abs(basis[:, 0])                                # +0.0 * negative = -0.0; +0.0 + -0.0 = +0.0
    want = po.project(x, basis, mean, None)
    assert np.isnan(want[1]).all() and np.isfinite(want[0]).all() and np.isfinite(want[4]).all() and not np.isfinite(want[2]).any()
    assert (bits(want[5]) == 0).all()                                 # +0.0, as defined
    for plan in (ONE_PASS, SPLIT):
        words = raw_project(e, padded(e, x, 2), D, padded(e, basis, 2), M, dev(e, mean), None, plan)
        assert (words[:, M:] == SENTINEL).all() and same_up_to_nan(words[:, :M], want), plan
    # a row of -0.0 without a mean: every product is -0.0 or +0.0 and s starts at +0.0
    z = np.full((1, D), -0.0)
    want = po.project(z, basis, None, None)
    assert (bits(want) == 0).all()
    assert same_rows(raw_project(e, padded(e, z, 1), D, padded(e, basis, 1), M, None, None, SPLIT), want, M)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_every_refused_argument_writes_nothing(dlc, e):
    L = dlc._lib
    rows, D, M = 6, 1030, 5
    rng = np.random.RandomState(7)
    xb, bb = padded(e, rng.standard_normal((rows, D)), 2), padded(e, rng.standard_normal((D, M)), 2)
    mean, scale = dev(e, rng.standard_normal(D)), dev(e, rng.uniform(0.5, 2.0, M))
    out = sentinel_f64(e, rows, M + 2)
    ws = torch.empty(e.lib.dlc_pca_project_workspace_bytes(rows, D, M, SPLIT) + 64, dtype=torch.uint8, device=e.device)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    A, S, W = L.DLC_ERR_BAD_ARG, L.DLC_ERR_BAD_SHAPE, L.DLC_ERR_WORKSPACE

    def project(x=p(xb), rows=rows, D=D, ldx=xb.stride(0), mu=p(mean), dt=F64, b=p(bb), M=M, ldb=bb.stride(0), sc=p(scale), o=p(out),
                ld_out=out.stride(0), plan=SPLIT, w=p(ws), wb=ws.numel()):
        return e.lib.dlc_pca_project(e.ctx, x, rows, D, ldx, mu, dt, b, M, ldb, sc, o, ld_out, plan, w, wb, None)

    cases = [
        (dict(x=None), A), (dict(b=None), A), (dict(o=None), A), (dict(rows=0), A), (dict(D=0), A), (dict(M=0), A), (dict(rows=-1), A),
        (dict(ldx=D - 1), A), (dict(ldb=M - 1), A), (dict(ld_out=M - 1), A), (dict(dt=0), A), (dict(dt=4), A), (dict(plan=3), A),
        (dict(plan=-1), A), (dict(x=off(xb, 4)), A), (dict(mu=off(mean, 4)), A), (dict(sc=off(scale, 4)), A), (dict(o=off(out, 4)), A),
        (dict(b=off(bb, 4)), A), (dict(b=off(bb, 2), dt=F32), A),
        (dict(o=p(xb), ld_out=xb.stride(0)), A), (dict(o=p(mean), rows=1), A), (dict(o=p(bb), rows=1), A), (dict(o=p(scale), rows=1), A),
        (dict(M=8193, ldb=8193, ld_out=8193), S), (dict(rows=1 << 31), S), (dict(D=1 << 31, ldx=1 << 31), S), (dict(rows=65), S),
        (dict(w=None), W), (dict(wb=64), W), (dict(w=off(ws, 8)), W), (dict(plan=AUTO, w=None), W),
    ]
    before = [t.clone() for t in (xb, bb, mean, scale)]
    for kw, status in cases:
        assert project(**kw) == status, sorted(kw)
        assert e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    assert (out.view(torch.int64) == SENTINEL).all()
    for t, b in zip((xb, bb, mean, scale), before):
        assert torch.equal(t.view(torch.int64), b.view(torch.int64))
    assert project() == 0 and project(plan=ONE_PASS, w=None, wb=0) == 0      # and the calls they were derived from are accepted
    torch.cuda.synchronize()


# ---- Pca.fit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(48, 200), (200, 48)])
def test_fit_against_the_oracle(dlc, e, n, d):
    """Both routes (N <= D: Gram and back-projection; N > D: the covariance).  The device products differ from NumPy's by
    their summation order alone, the class of error RECORDED_DELTA measures: the fit stays within 64 x of it.  A dropped
    centring, a missing 1 / (N - 1) or a transposed basis is wrong by more than 1e-2."""
    x = po.yardstick_rows(n, d)
    r_var, r_vec = po.RECORDED_DELTA[(n, d)]
    mu, B, var, scale = po.fit_svd(x, 12)
    a = dlc.Pca(12).fit(x)
    b = dlc.Pca(12).fit(torch.from_numpy(x).to(e.device))
    for name in ("mean", "basis", "variance", "scale"):
        assert torch.equal(getattr(a, name).view(torch.int64), getattr(b, name).view(torch.int64)), name
    got_B, got_var = a.basis.cpu().numpy(), a.explained_variance_
    assert (a.width, a.dim, a.n_rows) == (d, 12, n) and got_B.shape == (d, 12)
    total = float(((x - mu) ** 2).sum()) / (n - 1)                              # train_pca's variance_kept divides by it
    assert abs(a.total_variance_ - total) <= 1e-12 * total and dlc.Pca(3).total_variance_ is None
    assert np.array_equal(bits(a.mean.cpu().numpy()), bits(mu))                 # dlc_kmeans_step's mean, a defined sum
    d_var, d_vec = float(np.max(np.abs(got_var - var) / var)), float(np.max(np.abs(got_B - B)))
    print("Pca.fit %d x %d: delta_var %.2e (bound %.1e), delta_vec %.2e (bound %.1e)" % (n, d, d_var, 64 * r_var, d_vec, 64 * r_vec))
    assert d_var <= 64 * r_var and d_vec <= 64 * r_vec
    assert (got_B[np.argmax(np.abs(got_B), axis=0), np.arange(12)] > 0).all()   # the sign rule
    assert np.array_equal(bits(a.scale.cpu().numpy()), bits(1.0 / np.sqrt(got_var + 0.0)))
    # whitened rows have covariance I within the same margin: 64 x the recorded delta, the smaller of the two
    y = a.transform(x)
    tol = 64 * min(r_var, r_vec)
    err = float(np.abs(y.T @ y / (n - 1) - np.eye(12)).max())
    print("Pca.fit %d x %d: whitened covariance off I by %.2e (bound %.1e)" % (n, d, err, tol))
    assert err <= tol
    with pytest.raises(ValueError):
        dlc.Pca(min(n, d)).fit(x[:, :min(n, d)][:min(n, d)])                    # centring leaves rank min(n, d) - 1
    with pytest.raises(ValueError):
        dlc.Pca(3).fit(np.where(np.arange(d) == 1, np.nan, x))


def test_fit_takes_max_rows_by_the_seed(dlc, e):
    x = po.yardstick_rows(200, 48)
    take = np.sort(np.random.RandomState(3).choice(200, 60, replace=False))
    a, b = dlc.Pca(5, max_rows=60, seed=3).fit(x), dlc.Pca(5).fit(x[take])
    assert a.n_rows == 60 and torch.equal(a.basis.view(torch.int64), b.basis.view(torch.int64))


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_pca_surface(dlc, e, tmp_path):
    x = po.yardstick_rows(48, 200)
    m = dlc.Pca(6, eps=1e-9).fit(x)
    arrays = lambda q: (q.basis.cpu().numpy(), q.mean.cpu().numpy(), q.scale.cpu().numpy() if q.scale is not None else None)
    want = po.project(x, *arrays(m))
    got = m.transform(x)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(want))
    t = m.transform_tensor(torch.from_numpy(x).to(e.device))
    assert t.device == e.device and np.array_equal(bits(t.cpu().numpy()), bits(want))
    assert np.array_equal(bits(m.scale.cpu().numpy()), bits(1.0 / np.sqrt(m.explained_variance_ + 1e-9)))
    path = str(tmp_path / "pca.npz")
    m.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["mean", "basis", "variance", "scale", "whiten", "eps", "n_rows"])
        assert z["basis"].shape == (200, 6) and z["basis"].dtype == np.float64 and bool(z["whiten"]) and float(z["eps"]) == 1e-9
        assert int(z["n_rows"]) == 48 and z["mean"].shape == (200,) and z["variance"].shape == (6,) and z["scale"].shape == (6,)
    w = dlc.Pca.load(path)
    assert (w.dim, w.width, w.whiten, w.eps, w.n_rows) == (6, 200, True, 1e-9, 48)
    assert np.array_equal(bits(w.transform(x)), bits(want))
    # an fp32 basis: rounded once at the end of fit, stored as fp32, projected exactly as the oracle does on the rounded basis
    f = dlc.Pca(6, basis="f32", whiten=False).fit(x)
    assert f.basis.dtype == torch.float32 and f.scale is None
    assert np.array_equal(f.basis.cpu().numpy(), dlc.Pca(6, whiten=False).fit(x).basis.cpu().numpy().astype(np.float32))
    assert np.array_equal(bits(f.transform(x)), bits(po.project(x, *arrays(f))))
    f.save(path)
    g = dlc.Pca.load(path)
    assert g.basis.dtype == torch.float32 and g.scale is None and not g.whiten
    assert np.array_equal(bits(g.transform(x)), bits(f.transform(x)))
    # the engine wrapper: a row-strided view is taken as it is, out= wider than M keeps its other columns
    xb = padded(e, x, 4)[:, :200]
    bb = padded(e, m.basis.cpu().numpy(), 3)[:, :6]
    out = sentinel_f64(e, 48, 9)
    for plan in ("auto", "one_pass", "split"):
        r = e.pca_project(xb, bb, m.mean, m.scale, out=out, plan=plan)
        assert r.data_ptr() == out.data_ptr() and r.shape == (48, 6) and same_rows(out.view(torch.int64).cpu().numpy(), want, 6)
    assert np.array_equal(bits(e.pca_project(xb, bb).cpu().numpy()), bits(po.project(x, m.basis.cpu().numpy())))
    big = torch.zeros((65, 200), dtype=torch.float64, device=e.device)
    for bad in (lambda: dlc.Pca(0), lambda: dlc.Pca(8193), lambda: dlc.Pca(4, basis="bf16"), lambda: dlc.Pca(4, eps=-1.0),
                lambda: dlc.Pca(4, max_rows=1), lambda: dlc.Pca(4).transform(x), lambda: m.transform(x[:, :199]),
                lambda: dlc.Pca(4).save(path), lambda: dlc.Pca(2).fit(x[:1]), lambda: e.pca_project(xb, bb, plan="fast"),
                lambda: e.pca_project(xb.float(), bb), lambda: e.pca_project(xb, bb[:199]), lambda: e.pca_project(xb, bb.half()),
                lambda: e.pca_project(xb, bb, m.mean[:199]), lambda: e.pca_project(xb, bb, None, m.scale[:5]),
                lambda: e.pca_project(xb, bb, out=out[:, :5]), lambda: e.pca_project(xb, bb, out=out[:47]),
                lambda: e.pca_project(big, bb, plan="split")):
        with pytest.raises(ValueError):
            bad()


def test_planted_scene_through_pca_and_the_database(dlc, e):
    """Vlad.fit -> Pca(16).fit on the 40 database rows -> KeyframeDatabase (bf16) -> match_topk: 40 of 40 (the smallest
    bf16 top-1 margin at 16 components is 0.3, test_pca_cpu.py)."""
    db, q = vo.planted_scene(seed=0)
    v = dlc.Vlad(n_words=16, seed=0).fit(db, iters=10)
    rows_db, rows_q = v.transform_tensor(db), v.transform_tensor(q)
    m = dlc.Pca(16).fit(rows_db)
    kdb = dlc.KeyframeDatabase(m.transform_tensor(rows_db).to(torch.float32), dtype="bf16")
    _, i = kdb.match_topk(kdb.prepare_queries(m.transform_tensor(rows_q).to(torch.float32)), 1)
    hits = int((i[:, 0].cpu() == torch.arange(40)).sum())
    print("planted scene on the device behind Pca(16): %d / 40" % hits)
    assert hits == 40


def run_module(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd." + module, os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_train_vlad_then_train_pca_then_loop_closure(dlc, tmp_path):
    book, model = str(tmp_path / "book.npz"), str(tmp_path / "pca.npz")
    res = run_module("train_vlad", "--words", "16", "--iters", "5", "--seed", "2", "--save", book)
    assert res.returncode == 0, res.stdout + res.stderr
    res = run_module("train_pca", "--pool", "vlad", "--codebook", book, "--components", "8", "--save", model)
    assert res.returncode == 0, res.stdout + res.stderr
    fields = res.stdout.strip().split("\t")
    assert fields[:8] == ["pca", "rows", "17", "width", "40000", "components", "8", "variance_kept"] and len(fields) == 9, res.stdout
    assert 0.0 < float(fields[8]) <= 1.0 + 1e-9
    with np.load(model) as z:
        assert z["basis"].shape == (40000, 8) and z["basis"].dtype == np.float64 and np.isfinite(z["basis"]).all()
        assert z["scale"].shape == (8,) and bool(z["whiten"]) and int(z["n_rows"]) == 17
    runs = [run_module("loop_closure", "--network", "sdav", "--metric", "cosine", "--pool", "vlad", "--codebook", book, "--pca", model,
                       "--exclusion", "2", "--k", "2", "--batch", "4", "--threshold", "-1") for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
        assert "frames\t17\tkey-frames\t17" in r.stderr
        lines = r.stdout.splitlines()
        assert lines and all(l.startswith("loop\t") and len(l.split("\t")) == 6 for l in lines)
        for l in lines:
            _, frame, _, match, _, score = l.split("\t")
            assert 0 <= int(match) < int(frame) and -1.0 <= float(score) <= 1.0
    assert runs[0].stdout == runs[1].stdout
    # a model of another width, and --pca behind another network or metric, are refused with a message
    r = run_module("loop_closure", "--network", "sdav", "--metric", "cosine", "--pca", model)
    assert r.returncode == 2 and "--pca: its rows are 40000 wide, the frame descriptor 75000" in r.stderr and r.stdout == ""
    r = run_module("loop_closure", "--pca", model)
    assert r.returncode == 2 and "--pca needs --network sdav --metric cosine" in r.stderr and r.stdout == ""
    r = run_module("loop_closure", "--network", "sdav", "--metric", "similarity", "--pca", model)
    assert r.returncode == 2 and "--pca needs --network sdav --metric cosine" in r.stderr and r.stdout == ""
