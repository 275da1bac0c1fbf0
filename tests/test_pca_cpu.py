"""PCA projection and fit without a GPU: tests/pca_oracle.py (the NumPy restatement of include/dlc.h, dlc_pca_project, and
of Pca.fit's recipe) against per-element Python loops; that the chunking is real; the header's constants and the
workspace arithmetic of the built library; how far the oracle's two fit routes differ (the yardstick the device fit is
held to); the planted scene behind the oracle PCA; the Python surface and the CLI's argument rules."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pca_oracle as po
import vlad_oracle as vo
from conftest import GOLDEN, ROOT


# ---- 1. the oracle is the definition ---------------------------------------------------------------------------------------------
def loops(x, basis, mean, scale, chunk=po.CHUNK):
    """dlc_pca_project element by element on Python floats (IEEE doubles, one rounding per operation)."""
    rows, D = x.shape
    M = basis.shape[1]
    out = np.empty((rows, M))
    for r in range(rows):
        for c in range(M):
            y = None
            for d0 in range(0, D, chunk):
                s = 0.0
                for d in range(d0, min(D, d0 + chunk)):
                    t = float(x[r, d]) - float(mean[d]) if mean is not None else float(x[r, d])
                    q = t * float(basis[d, c])
                    s = s + q
                y = s if y is None else y + s
            out[r, c] = y * float(scale[c]) if scale is not None else y
    return out


@pytest.mark.parametrize("rows,D,M", [(1, 1, 1), (3, 7, 2), (2, 1025, 3), (2, 2051, 2)])
@pytest.mark.parametrize("f32", [False, True])
def test_the_oracle_is_the_definition(rows, D, M, f32):
    rng = np.random.RandomState(rows * 1000 + D + M)
    x, mean, scale = rng.standard_normal((rows, D)), rng.standard_normal(D), rng.uniform(0.5, 2.0, M)
    basis = rng.standard_normal((D, M)).astype(np.float32 if f32 else np.float64)
    for mu in (None, mean):
        for sc in (None, scale):
            got, want = po.project(x, basis, mu, sc), loops(x, basis, mu, sc)
            assert got.dtype == np.float64 and (got.view(np.int64) == want.view(np.int64)).all()


def test_chunking_is_real():
    """The chunked sum is not one unbroken serial chain.  D = 1025 cannot show it: its second chunk is one product q, and
    s_0 + (+0.0 + q) is s_0 + q, the chain's own last step -- equal bits on every input.  From D = 1026 on the second
    chunk rounds a sum of its own and the bits part."""
    rng = np.random.RandomState(0)
    x, b = rng.standard_normal((4, 2048)), rng.standard_normal((2048, 8))
    same = lambda D: (po.project(x[:, :D], b[:D]).view(np.int64) == po.project_one_chain(x[:, :D], b[:D]).view(np.int64))
    assert same(1024).all() and same(1025).all()
    assert not same(1026).all() and not same(2048).all()


def test_the_sign_rule():
    B = np.array([[1.0, -3.0, 2.0], [-2.0, 3.0, -2.0], [0.5, 1.0, 1.0]])
    S = po.sign_rule(B)
    assert (S[:, 0] == -B[:, 0]).all() and (S[:, 1] == -B[:, 1]).all() and (S[:, 2] == B[:, 2]).all()   # ties: the lowest index


# ---- 2. the C ABI's host arithmetic ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeploopcloser_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deeploopcloser_amd", "csrc"), "-j4"])
    return _lib.load()


def test_header_constants(lib):
    from deeploopcloser_amd import _lib
    for name in ("dlc_pca_project_workspace_bytes", "dlc_pca_project"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dlc_abi_version() == 20 and _lib.DLC_ABI_VERSION == 20
    header = open(os.path.join(ROOT, "include", "dlc.h")).read()
    assert "#define DLC_PCA_CHUNK %d\n" % _lib.DLC_PCA_CHUNK in header and _lib.DLC_PCA_CHUNK == po.CHUNK == 1024
    assert "#define DLC_PCA_MAX_COMPONENTS %d\n" % _lib.DLC_PCA_MAX_COMPONENTS in header and _lib.DLC_PCA_MAX_COMPONENTS == 8192
    assert "#define DLC_PCA_SPLIT_MAX_ROWS %d\n" % _lib.DLC_PCA_SPLIT_MAX_ROWS in header and _lib.DLC_PCA_SPLIT_MAX_ROWS == 64
    assert "enum { DLC_PCA_PLAN_AUTO = %d, DLC_PCA_PLAN_ONE_PASS = %d, DLC_PCA_PLAN_SPLIT = %d };" % (
        _lib.DLC_PCA_PLAN_AUTO, _lib.DLC_PCA_PLAN_ONE_PASS, _lib.DLC_PCA_PLAN_SPLIT) in header
    assert (_lib.DLC_PCA_PLAN_AUTO, _lib.DLC_PCA_PLAN_ONE_PASS, _lib.DLC_PCA_PLAN_SPLIT) == (0, 1, 2)


def test_a_null_context_is_a_bad_argument(lib):
    from deeploopcloser_amd import _lib
    x, b, out = (C.c_double * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
    assert lib.dlc_pca_project(None, x, 2, 2, 2, None, _lib.DLC_F64, b, 2, 2, None, out, 2, 1, None, 0, None) == _lib.DLC_ERR_BAD_ARG
    assert not any(out)


def test_workspace_bytes(lib):
    ws = lib.dlc_pca_project_workspace_bytes
    AUTO, ONE, SPLIT = 0, 1, 2
    assert ws(1, 40000, 4096, SPLIT) >= 1 * 40 * 4096 * 8 and ws(1, 40000, 4096, SPLIT) % 256 == 0
    assert ws(64, 75000, 4096, SPLIT) >= 64 * 74 * 4096 * 8
    assert ws(3, 1025, 7, SPLIT) >= 3 * 2 * 7 * 8 and ws(1, 1, 1, SPLIT) >= 8
    assert ws(1063, 40000, 4096, ONE) == 0 and ws(1, 40000, 4096, ONE) == 0                # ONE_PASS needs none
    assert ws(1, 40000, 4096, AUTO) == ws(1, 40000, 4096, SPLIT)                           # AUTO: one frame is split
    assert ws(1063, 40000, 4096, AUTO) == 0 and ws(1, 1024, 4096, AUTO) == 0               # many rows, one chunk: one pass
    assert ws(2 ** 31 - 1, 2 ** 31 - 1, 8192, ONE) == 0 and ws(64, 2 ** 31 - 1, 8192, SPLIT) > 0
    for rows, D, M, plan in ((0, 8, 4, SPLIT), (-1, 8, 4, SPLIT), (65, 8, 4, SPLIT), (2 ** 31, 8, 4, AUTO), (1, 0, 4, SPLIT),
                             (1, 2 ** 31, 4, SPLIT), (1, 8, 0, SPLIT), (1, 8, 8193, SPLIT), (1, 8, 4, 3), (1, 8, 4, -1)):
        assert ws(rows, D, M, plan) == 0, (rows, D, M, plan)


# ---- 3. the fit yardstick -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(48, 200), (200, 48)])
def test_fit_routes_agree(n, d):
    """The oracle's two routes on a well separated spectrum: how far they differ is the summation-order error of the fit,
    recorded in pca_oracle.RECORDED_DELTA and the scale of the device test's margin."""
    x = po.yardstick_rows(n, d)
    a, b = po.fit_gram(x, 12), po.fit_svd(x, 12)
    ratios = b[2][:-1] / b[2][1:]
    d_var, d_vec = po.route_delta(a, b)
    r_var, r_vec = po.RECORDED_DELTA[(n, d)]
    print("fit yardstick %d x %d: variance ratios >= %.2f, delta_var %.2e (recorded %.1e), delta_vec %.2e (recorded %.1e)"
          % (n, d, ratios.min(), d_var, r_var, d_vec, r_vec))
    assert ratios.min() >= 2.8
    assert d_var < po.DELTA_CEILING and d_vec < po.DELTA_CEILING
    assert r_var < po.DELTA_CEILING and r_vec < po.DELTA_CEILING
    assert d_var <= 64 * r_var and d_vec <= 64 * r_vec                  # the recorded values are of this machine's class
    assert (a[0].view(np.int64) == b[0].view(np.int64)).all()           # one mean
    for fit in (a, b):                                                  # orthonormal, signed, whitening to I
        B = fit[1]
        assert np.abs(B.T @ B - np.eye(12)).max() < 1e-8
        assert (B[np.argmax(np.abs(B), axis=0), np.arange(12)] > 0).all()
        y = po.project(x, B, fit[0], fit[3])
        assert np.abs(y.T @ y / (n - 1) - np.eye(12)).max() < 1e-6
    with pytest.raises(ValueError):
        po.fit_svd(x[:5], 5)                                            # 5 rows: rank 4


# ---- 4. the planted scene ------------------------------------------------------------------------------------------------------
def bf16(a):
    """fp64 -> fp32 -> bf16 (to nearest even), as fp64 again."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def planted_vlad():
    db, q = vo.planted_scene(seed=0)
    c = vo.lloyd(db.reshape(-1, 64), 16, 10, 0)
    vd, _ = vo.vlad_encode(db.reshape(-1, 64), c, 30, vo.NORM_INTRA)
    vq, _ = vo.vlad_encode(q.reshape(-1, 64), c, 30, vo.NORM_INTRA)
    return vd, vq


def test_planted_scene_survives_the_projection():
    vd, vq = planted_vlad()
    assert vd.shape == (40, 1024)
    margins = {}
    for m in (8, 16, 32, 39):
        for whiten in (True, False):
            mu, B, _, scale = po.fit_svd(vd, m, whiten=whiten)
            pd, pq = po.project(vd, B, mu, scale), po.project(vq, B, mu, scale)
            assert vo.cosine_hits(pd, pq) == 40, (m, whiten)
            if whiten:
                unit = lambda a: bf16(a / np.linalg.norm(a, axis=1, keepdims=True))
                s = unit(pq) @ unit(pd).T
                top = np.sort(s, axis=1)
                assert (s.argmax(axis=1) == np.arange(40)).all()
                margins[m] = float((top[:, -1] - top[:, -2]).min())
    print("planted scene behind PCA: smallest bf16 top-1 margin %s" % ", ".join("%d: %.3f" % kv for kv in sorted(margins.items())))
    assert margins[16] > 0.1                                            # the device test uses 16 components


# ---- 5. the Python surface and the CLI's argument rules ----------------------------------------------------------------------------
def test_the_python_surface():
    import inspect
    import deeploopcloser_amd as dlc
    assert "Pca" in dlc.__all__ and dlc.pca.Pca is dlc.Pca
    p = inspect.signature(dlc.Pca.__init__).parameters
    assert list(p)[1:] == ["n_components", "whiten", "eps", "basis", "max_rows", "seed", "device"]
    assert [p[k].default for k in list(p)[2:]] == [True, 0.0, "f64", 4096, 0, None]
    for name in ("fit", "transform", "transform_tensor", "save", "load"):
        assert callable(getattr(dlc.Pca, name))
    for name in ("dim", "width", "explained_variance_"):
        assert isinstance(getattr(dlc.Pca, name), property)
    p = inspect.signature(dlc.Engine.pca_project).parameters
    assert list(p)[1:] == ["x", "basis", "mean", "scale", "out", "plan"] and p["plan"].default == "auto"
    from deeploopcloser_amd import loop_closure, pipeline
    p = inspect.signature(pipeline.sdav_place_descriptors_from_frames).parameters
    assert "pca" in p and p["pca"].default is None
    p = inspect.signature(loop_closure.describe_sdav_compact).parameters
    assert list(p) == ["files", "network", "key_points_fn", "pool", "pca"] and p["pca"].default is None


def run_cli(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd." + module, os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("models")
    paths = {}
    for name, width in (("narrow", 64), ("vlad4", 4 * 2500)):
        paths[name] = str(d / (name + ".npz"))
        with open(paths[name], "wb") as f:
            np.savez(f, mean=np.zeros(width), basis=np.zeros((width, 2), dtype=np.float32), variance=np.ones(2), scale=np.ones(2),
                     whiten=np.array(True), eps=np.array(0.0), n_rows=np.array(3, dtype=np.int64))
    paths["book"] = str(d / "book.npz")
    with open(paths["book"], "wb") as f:
        np.savez(f, centroids=np.zeros((4, 2500)), norm=np.array("intra"), seed=np.array(0), inertia=np.zeros(1))
    paths["junk"] = str(d / "junk.npz")
    with open(paths["junk"], "wb") as f:
        f.write(b"not an archive")
    return paths


@pytest.mark.parametrize("args,message", [
    (("--pca", "vlad4"), "--pca needs --network sdav --metric cosine"),
    (("--network", "sdav", "--metric", "similarity", "--pca", "vlad4"), "--pca needs --network sdav --metric cosine"),
    (("--network", "seqslam", "--metric", "sad", "--pca", "vlad4"), "--pca needs --network sdav --metric cosine"),
    (("--fuse", "sad,distance", "--pca", "vlad4"), "--pca needs --network sdav --metric cosine"),
    (("--network", "sdav", "--pca", "narrow"), "--pca: its rows are 64 wide, the frame descriptor 75000"),
    (("--network", "sdav", "--pca", "vlad4"), "--pca: its rows are 10000 wide, the frame descriptor 75000"),
    (("--network", "sdav", "--pool", "vlad", "--codebook", "book", "--pca", "narrow"), "--pca: its rows are 64 wide, the frame descriptor 10000"),
    (("--network", "sdav", "--pca", "junk"), "--pca: "),
    (("--network", "sdav", "--pca", "absent.npz"), "--pca: "),
])
def test_cli_refuses(args, message, models):
    res = run_cli("loop_closure", *[models.get(a, a) for a in args])
    assert res.returncode == 2 and "usage:" in res.stderr and "error: " + message in res.stderr, res.stdout + res.stderr
    assert res.stdout == ""


@pytest.mark.parametrize("args,message", [
    (("--save", "x.npz"), "the following arguments are required: --components"),
    (("--components", "0", "--save", "x.npz"), "--components must be 1..8192"),
    (("--components", "8193", "--save", "x.npz"), "--components must be 1..8192"),
    (("--components", "4", "--eps", "-1", "--save", "x.npz"), "--eps must be finite and >= 0"),
    (("--components", "4", "--pool", "vlad", "--save", "x.npz"), "--pool vlad needs --codebook"),
    (("--components", "4", "--codebook", "b.npz", "--save", "x.npz"), "--codebook needs --pool vlad"),
    (("--components", "4"), "the following arguments are required: --save"),
    (("--components", "4", "--pattern", "*.nothing", "--save", "x.npz"), "Specified dataset is empty"),
])
def test_train_pca_refuses(args, message):
    res = run_cli("train_pca", *args)
    assert res.returncode == 2 and "usage:" in res.stderr and message in res.stderr, res.stdout + res.stderr
    assert res.stdout == "" and not os.path.exists(os.path.join(ROOT, "x.npz"))


def test_the_pca_models_fields_and_refusals(tmp_path):
    """Pca.load's refusals need no device: they come before the model is uploaded."""
    from deeploopcloser_amd.pca import FIELDS, Pca
    assert FIELDS == ("mean", "basis", "variance", "scale", "whiten", "eps", "n_rows")
    good = dict(mean=np.zeros(5), basis=np.zeros((5, 2)), variance=np.ones(2), scale=np.ones(2), whiten=np.array(True),
                eps=np.array(0.0), n_rows=np.array(3, dtype=np.int64))
    for drop in FIELDS:
        path = str(tmp_path / ("no_%s.npz" % drop))
        with open(path, "wb") as f:
            np.savez(f, **{k: v for k, v in good.items() if k != drop})
        with pytest.raises(ValueError, match="lacks " + drop):
            Pca.load(path)
    for name, bad in (("basis", np.zeros(5)), ("basis", np.zeros((5, 2), dtype=np.int32)), ("mean", np.zeros(4)),
                      ("variance", np.ones(3)), ("scale", np.ones(1))):
        path = str(tmp_path / "bad.npz")
        with open(path, "wb") as f:
            np.savez(f, **dict(good, **{name: bad}))
        with pytest.raises(ValueError):
            Pca.load(path)
    path = str(tmp_path / "pickled.npz")
    with open(path, "wb") as f:
        np.savez(f, **dict(good, mean=np.array([None, 1], dtype=object)))
    with pytest.raises(ValueError):
        Pca.load(path)
