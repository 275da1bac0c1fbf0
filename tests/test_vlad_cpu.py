"""VLAD pooling and the k-means codebook without a GPU: tests/vlad_oracle.py (the NumPy restatement of include/dlc.h)
against per-element Python-float loops over the definition, the tie / duplicate / NaN rules, the empty word, permutation
invariance, the planted scene that motivates the feature, the C ABI's host-side refusals and the CLI's argument rules."""
import ctypes as C
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import vlad_oracle as vo
from conftest import GOLDEN, ROOT


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- 1. the oracle against plain loops over the definition ---------------------------------------------------------------------
def py_tree(v):
    P = 1
    while P < len(v):
        P <<= 1
    v = list(v) + [-0.0] * (P - len(v))

    def T(lo, n):
        return v[lo] if n == 1 else T(lo, n // 2) + T(lo + n // 2, n // 2)
    return T(0, P)


def py_dist(x, c):
    d = 0.0
    for h in range(len(x)):
        t = x[h] - c[h]
        q = t * t
        d = d + q
    return d


def py_assign(x, c):
    a, best = [], []
    for row in x:
        k_best, d_best = -1, float("nan")
        for k, word in enumerate(c):
            d = py_dist(row, word)
            if d != d:
                continue
            if k_best < 0 or d < d_best:
                k_best, d_best = k, d
        a.append(k_best)
        best.append(d_best)
    return a, best


def py_vlad(x, c, P, intra):
    x, c = [[float(v) for v in r] for r in x], [[float(v) for v in r] for r in c]
    K, H = len(c), len(c[0])
    a, _ = py_assign(x, c)
    out = []
    for f in range(len(x) // P):
        row = []
        for k in range(K):
            R, seen = [0.0] * H, False
            for p in range(P):
                n = f * P + p
                if a[n] != k:
                    continue
                for h in range(H):
                    r = x[n][h] - c[k][h]
                    R[h] = R[h] + r if seen else r
                seen = True
            if intra:
                s = py_tree([r * r for r in R])
                nk = math.sqrt(s)
                R = [0.0 if nk == 0.0 else r / nk for r in R]
            row += R
        out.append(row)
    return out, a


def py_kmeans(x, c, prev):
    x, c = [[float(v) for v in r] for r in x], [[float(v) for v in r] for r in c]
    K, H, B = len(c), len(c[0]), vo.KMEANS_BLOCK
    a, d = py_assign(x, c)
    nb = (len(x) + B - 1) // B
    counts = [sum(1 for v in a if v == k) for k in range(K)]
    c_out = []
    for k in range(K):
        row = []
        for h in range(H):
            S = []
            for b in range(nb):
                s = -0.0
                for n in range(b * B, min(len(x), b * B + B)):
                    if a[n] == k:
                        s = s + x[n][h]
                S.append(s)
            row.append(py_tree(S) / float(counts[k]) if counts[k] else c[k][h])
        c_out.append(row)
    inert = []
    for b in range(nb):
        s = 0.0
        for n in range(b * B, min(len(x), b * B + B)):
            if a[n] >= 0:
                s = s + d[n]
        inert.append(s)
    changed = len(x) if prev is None else sum(1 for n in range(len(x)) if prev[n] != a[n])
    return c_out, a, counts, py_tree(inert), changed


@pytest.mark.parametrize("frames,P,H,K", [(1, 1, 1, 1), (2, 3, 5, 2), (3, 5, 7, 4), (2, 6, 9, 3)])
@pytest.mark.parametrize("intra", [False, True])
def test_the_oracle_is_the_definition(frames, P, H, K, intra):
    rng = np.random.RandomState(frames * 100 + H)
    x, c = rng.standard_normal((frames * P, H)), rng.standard_normal((K, H))
    got, a = vo.vlad_encode(x, c, P, vo.NORM_INTRA if intra else vo.NORM_NONE)
    ref, ra = py_vlad(x.tolist(), c.tolist(), P, intra)
    assert a.tolist() == ra and a.dtype == np.int32
    assert np.array_equal(bits(got), bits(ref))
    a2, d2 = vo.assign(x, c)
    assert a2.tolist() == ra and np.array_equal(bits(d2), bits(py_assign(x.tolist(), c.tolist())[1]))


@pytest.mark.parametrize("rows", [1, 7, 1025, 2051])
def test_the_oracle_step_is_the_definition(rows):
    rng = np.random.RandomState(rows)
    x, c = rng.standard_normal((rows, 3)), rng.standard_normal((4, 3))
    c[3] = 50.0                                                      # an empty word
    prev = rng.randint(0, 4, size=rows).astype(np.int32)
    for pv in (None, prev):
        c_out, a, counts, inertia, changed = vo.kmeans_step(x, c, pv)
        rc, ra, rcounts, rin, rch = py_kmeans(x.tolist(), c.tolist(), None if pv is None else pv.tolist())
        assert a.tolist() == ra and counts.tolist() == rcounts and changed == rch
        assert np.array_equal(bits(c_out), bits(rc)) and struct.pack("d", inertia) == struct.pack("d", rin)
    assert counts[3] == 0 and np.array_equal(bits(c_out[3]), bits(c[3]))         # an empty word keeps its centre


def test_tree_is_not_a_left_to_right_sum():
    v = np.random.RandomState(3).standard_normal(1000)
    assert vo.tree(v) == py_tree(v.tolist())
    s = 0.0
    for t in v.tolist():
        s += t
    assert vo.tree(v) != s                                          # (the reason the oracle restates the order)
    assert struct.pack("d", float(vo.tree(np.array([-0.0])))) == struct.pack("d", -0.0)
    for n in (1, 2, 3, 5, 64, 100, 1000, 4097):
        w = np.random.RandomState(n).standard_normal((n, 3))
        assert np.array_equal(bits(vo.tree_pairwise(w)), bits(vo.tree(w)))


# ---- 2. ties, duplicates, NaN, empty words --------------------------------------------------------------------------------------
def test_ties_duplicates_and_nan():
    c = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.25, 0.5]])              # word 2 copies word 0
    x = np.array([[0.5, 0.0],                                                    # midway between words 0 and 1: the lower
                  [0.0, 0.0],                                                    # on words 0 and 2: never the copy
                  [np.nan, 1.0],                                                 # every distance NaN
                  [1.0, 0.0]])
    a, d = vo.assign(x, c)
    assert a.tolist() == [0, 0, -1, 1] and np.isnan(d[2]) and d[0] == 0.25
    out, _ = vo.vlad_encode(x, c, 4, vo.NORM_NONE)
    out = out.reshape(4, 2)
    assert np.array_equal(bits(out[0]), bits([0.5, 0.0]))           # (0.5, 0) - c0 first, then (0, 0) - c0 = +0.0 added
    assert np.array_equal(bits(out[2]), bits([0.0, 0.0])) and not np.isnan(out).any()     # the copy and the NaN row: nothing
    assert np.array_equal(bits(out[3]), bits([0.0, 0.0]))           # an empty word: +0.0
    out_i, _ = vo.vlad_encode(x, c, 4, vo.NORM_INTRA)
    assert np.array_equal(bits(out_i.reshape(4, 2)[0]), bits([1.0, 0.0]))
    assert np.array_equal(bits(out_i.reshape(4, 2)[1:]), bits(np.zeros((3, 2))))          # norm 0 -> +0.0
    # +inf can win: the only word that is not NaN
    a, d = vo.assign(np.array([[1.0]]), np.array([[np.nan], [np.inf]]))
    assert a.tolist() == [1] and d[0] == np.inf
    # a NaN row moves no centre and no count
    c_out, a, counts, inertia, changed = vo.kmeans_step(x, c)
    assert counts.tolist() == [2, 1, 0, 0] and a.tolist() == [0, 0, -1, 1] and changed == 4 and inertia == 0.25
    assert np.array_equal(bits(c_out), bits([[0.25, 0.0], [1.0, 0.0], [0.0, 0.0], [0.25, 0.5]]))


def test_none_is_exactly_permutation_invariant_on_a_dyadic_grid():
    rng = np.random.RandomState(5)
    x = rng.randint(-2048, 2048, size=(30, 16)) / 1024.0            # multiples of 2^-10: every sum below is exact
    c = rng.randint(-2048, 2048, size=(6, 16)) / 1024.0
    ref, _ = vo.vlad_encode(x, c, 30, vo.NORM_NONE)
    for seed in range(5):
        perm = np.random.RandomState(seed).permutation(30)
        got, _ = vo.vlad_encode(x[perm], c, 30, vo.NORM_NONE)
        assert np.array_equal(bits(got), bits(ref))


# ---- 3. the planted scene --------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_CODEBOOK_SEED = 0, 0
PLANTED_FLAT_HITS = 1                 # of 40; docs/LAB.md 30


def planted_descriptors():
    """(db flat, q flat, db vlad, q vlad) of the scene of docs/LAB.md 30: 40 places x 30 patches, 12 landmark types in 64-d,
    sigma 0.15; the revisit permuted + sigma 0.03; K = 16, 10 Lloyd steps on the database side."""
    db, q = vo.planted_scene(seed=PLANTED_SEED)
    c = vo.lloyd(db.reshape(-1, 64), 16, 10, PLANTED_CODEBOOK_SEED)
    vd, _ = vo.vlad_encode(db.reshape(-1, 64), c, 30, vo.NORM_INTRA)
    vq, _ = vo.vlad_encode(q.reshape(-1, 64), c, 30, vo.NORM_INTRA)
    return db.reshape(40, -1), q.reshape(40, -1), vd, vq


def test_planted_scene_vlad_finds_every_place_the_concatenation_few():
    fd, fq, vd, vq = planted_descriptors()
    flat, centred, vlad = vo.cosine_hits(fd, fq), vo.cosine_hits(fd - fd.mean(0), fq - fd.mean(0)), vo.cosine_hits(vd, vq)
    print("planted scene: concatenation %d / 40 (centred %d / 40), VLAD %d / 40" % (flat, centred, vlad))
    assert vlad == 40
    assert flat < 10 and centred < 10
    assert flat == PLANTED_FLAT_HITS


# ---- 4. the C ABI and the Python surface -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeploopcloser_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deeploopcloser_amd", "csrc"), "-j4"])
    return _lib.load()


def test_the_library_exports_the_entry_points(lib):
    from deeploopcloser_amd import _lib
    for name in ("dlc_vlad_assign", "dlc_vlad_encode_workspace_bytes", "dlc_vlad_encode", "dlc_kmeans_step_workspace_bytes",
                 "dlc_kmeans_step"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dlc_abi_version() == 20 and _lib.DLC_ABI_VERSION == 20
    header = open(os.path.join(ROOT, "include", "dlc.h")).read()
    assert "#define DLC_KMEANS_BLOCK %d\n" % _lib.DLC_KMEANS_BLOCK in header and _lib.DLC_KMEANS_BLOCK == vo.KMEANS_BLOCK == 1024
    assert "#define DLC_VLAD_MAX_WORDS %d\n" % _lib.DLC_VLAD_MAX_WORDS in header and _lib.DLC_VLAD_MAX_WORDS == 256
    assert "#define DLC_VLAD_MAX_PATCHES %d\n" % _lib.DLC_VLAD_MAX_PATCHES in header and _lib.DLC_VLAD_MAX_PATCHES == 1024
    assert "enum { DLC_VLAD_NORM_NONE = %d, DLC_VLAD_NORM_INTRA = %d };" % (_lib.DLC_VLAD_NORM_NONE, _lib.DLC_VLAD_NORM_INTRA) in header
    assert (_lib.DLC_VLAD_NORM_NONE, _lib.DLC_VLAD_NORM_INTRA) == (vo.NORM_NONE, vo.NORM_INTRA)


def test_a_null_context_is_a_bad_argument(lib):
    from deeploopcloser_amd import _lib
    x, c, out = (C.c_double * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
    a = (C.c_int32 * 4)()
    cnt, ch = (C.c_int64 * 2)(), (C.c_int64 * 1)()
    assert lib.dlc_vlad_assign(None, x, 4, 2, 2, c, 2, 2, a, None, None) == _lib.DLC_ERR_BAD_ARG
    assert lib.dlc_vlad_encode(None, x, 2, 2, 2, 2, c, 2, 2, 0, out, 4, None, None, 0, None) == _lib.DLC_ERR_BAD_ARG
    assert lib.dlc_kmeans_step(None, x, 4, 2, 2, c, 2, 2, out, 2, None, a, cnt, out, ch, None, 0, None) == _lib.DLC_ERR_BAD_ARG
    assert not any(out) and not any(a) and not any(cnt) and not any(ch)


def test_workspace_bytes(lib):
    enc, step = lib.dlc_vlad_encode_workspace_bytes, lib.dlc_kmeans_step_workspace_bytes
    assert enc(1063, 30, 2500, 16) >= 1063 * 30 * 4 and enc(1063, 30, 2500, 16) % 256 == 0
    assert 0 < enc(1, 1, 1, 1) <= enc(17, 30, 65, 256)
    assert enc(2 ** 31 - 1, 1024, 1, 256) > 0 and enc(1, 1, 2 ** 31 - 1, 1) > 0
    for frames, P, H, K in ((0, 30, 8, 4), (-1, 30, 8, 4), (2 ** 31, 30, 8, 4), (1, 0, 8, 4), (1, 1025, 8, 4), (1, 30, 0, 4),
                            (1, 30, 8, 0), (1, 30, 8, 257), (1, 30, 2 ** 31, 1), (1, 30, 2 ** 23, 256)):
        assert enc(frames, P, H, K) == 0, (frames, P, H, K)
    nb = 3
    assert step(3000, 33, 8) >= 8 * (3000 + nb * 8 * 33 + nb * (8 + 2)) and step(3000, 33, 8) % 256 == 0
    assert 0 < step(1, 1, 1) <= step(1025, 1, 1)
    for rows, H, K in ((0, 8, 4), (-3, 8, 4), (2 ** 31, 8, 4), (10, 0, 4), (10, 8, 0), (10, 8, 257), (10, 2 ** 31, 1),
                       (10, 2 ** 23, 256)):
        assert step(rows, H, K) == 0, (rows, H, K)


def test_the_python_surface():
    import inspect
    import deeploopcloser_amd as dlc
    for name in ("Vlad", "vlad_frame_descriptors"):
        assert name in dlc.__all__ and hasattr(dlc, name)
    assert dlc.vlad.Vlad is dlc.Vlad and dlc.matching.vlad_frame_descriptors is dlc.vlad_frame_descriptors
    p = inspect.signature(dlc.Vlad.__init__).parameters
    assert list(p)[1:4] == ["n_words", "norm", "seed"] and (p["n_words"].default, p["norm"].default, p["seed"].default) == (16, "intra", 0)
    assert inspect.signature(dlc.Vlad.fit).parameters["iters"].default == 20
    assert inspect.signature(dlc.Vlad.transform).parameters["patches"].default == 30
    for name in ("transform_tensor", "assign", "save", "load", "set_codebook"):
        assert callable(getattr(dlc.Vlad, name))
    assert list(inspect.signature(dlc.vlad_frame_descriptors).parameters) == ["h", "vlad", "patches"]
    for name in ("vlad_assign", "vlad_encode", "kmeans_step"):
        assert callable(getattr(dlc.Engine, name))
    from deeploopcloser_amd import loop_closure, pipeline
    p = inspect.signature(loop_closure.describe_sdav).parameters
    assert list(p) == ["files", "network", "key_points_fn", "pool"] and p["pool"].default is None
    assert list(inspect.signature(pipeline.sdav_place_descriptors_from_frames).parameters)[:3] == ["frames", "network", "vlad"]


# ---- 5. the CLI's argument rules ------------------------------------------------------------------------------------------------
def run_cli(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd." + module, os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def codebooks(tmp_path_factory):
    d = tmp_path_factory.mktemp("codebooks")
    paths = {}
    for name, width in (("narrow", 64), ("right", 2500)):
        paths[name] = str(d / (name + ".npz"))
        with open(paths[name], "wb") as f:
            np.savez(f, centroids=np.zeros((4, width)), norm=np.array("intra"), seed=np.array(0), inertia=np.zeros(1))
    paths["junk"] = str(d / "junk.npz")
    with open(paths["junk"], "wb") as f:
        f.write(b"not an archive")
    paths["absent"] = str(d / "absent.npz")
    return paths


@pytest.mark.parametrize("args,message", [
    (("--network", "sdav", "--pool", "vlad"), "--pool vlad needs --codebook"),
    (("--pool", "vlad", "--codebook", "right"), "--pool vlad needs --network sdav --metric cosine"),
    (("--network", "sdav", "--metric", "similarity", "--pool", "vlad", "--codebook", "right"), "--pool vlad needs --network sdav --metric cosine"),
    (("--network", "seqslam", "--metric", "sad", "--pool", "vlad", "--codebook", "right"), "--pool vlad needs --network sdav --metric cosine"),
    (("--fuse", "sad,distance", "--pool", "vlad", "--codebook", "right"), "--pool vlad needs --network sdav --metric cosine"),
    (("--network", "sdav", "--codebook", "right"), "--codebook needs --pool vlad"),
    (("--network", "sdav", "--pool", "flatten", "--codebook", "right"), "--codebook needs --pool vlad"),
    (("--network", "sdav", "--pool", "vlad", "--codebook", "narrow"), "--codebook: its words are 64 wide, the encoder's descriptors 2500"),
    (("--network", "sdav", "--pool", "vlad", "--codebook", "junk"), "--codebook: "),
    (("--network", "sdav", "--pool", "vlad", "--codebook", "absent"), "--codebook: "),
    (("--network", "sdav", "--pool", "mean"), "argument --pool: invalid choice"),
])
def test_cli_refuses(args, message, codebooks):
    res = run_cli("loop_closure", *[codebooks.get(a, a) for a in args])
    assert res.returncode == 2 and "usage:" in res.stderr and "error: " + message in res.stderr, res.stdout + res.stderr
    assert res.stdout == ""


@pytest.mark.parametrize("args,message", [
    (("--words", "0", "--save", "x.npz"), "--words must be 1..256"),
    (("--words", "257", "--save", "x.npz"), "--words must be 1..256"),
    (("--iters", "0", "--save", "x.npz"), "--iters must be >= 1"),
    (("--words", "4"), "the following arguments are required: --save"),
    (("--pattern", "*.nothing", "--save", "x.npz"), "Specified dataset is empty"),
])
def test_train_vlad_refuses(args, message):
    res = run_cli("train_vlad", *args)
    assert res.returncode == 2 and "usage:" in res.stderr and message in res.stderr, res.stdout + res.stderr
    assert res.stdout == "" and not os.path.exists(os.path.join(ROOT, "x.npz"))


@pytest.mark.parametrize("flags", [(), ("--pool", "flatten")])
def test_flatten_leaves_the_call_path_untouched(flags, monkeypatch):
    """Without --pool vlad the stream calls describe_sdav(files, network) exactly as it always has -- no pool argument --
    and describe_sdav without a pool returns what its flattening returns, the same object."""
    import argparse
    from deeploopcloser_amd import loop_closure
    calls = []

    class Net:
        input_shape = [30, 1681]

        def __init__(self, dtype=None):
            pass

    class Stop(Exception):
        pass

    def fake_describe(*a, **kw):
        calls.append((a, kw))
        raise Stop()
    import deeploopcloser_amd.sdav as sdav_mod
    monkeypatch.setattr(sdav_mod, "SDAV", Net)
    monkeypatch.setattr(loop_closure, "describe_sdav", fake_describe)
    args = argparse.Namespace(fuse=None, network="sdav", encoder_dtype="float64", weights=None, pool=flags[1] if flags else None,
                              codebook=None, positions=None, batch=16, metric="cosine")
    with pytest.raises(Stop):
        loop_closure._stream(args, ["a.ppm", "b.ppm"])
    (a, kw), = calls
    assert len(a) == 2 and a[0] == ["a.ppm", "b.ppm"] and isinstance(a[1], Net) and kw == {}


def test_describe_sdav_without_a_pool_is_the_flattening(monkeypatch):
    from deeploopcloser_amd import loop_closure
    marker = object()
    monkeypatch.setattr(loop_closure, "_describe_sdav_flat", lambda files, network, key_points_fn: marker)
    assert loop_closure.describe_sdav(["f"]) is marker and loop_closure.describe_sdav(["f"], None, None, None) is marker
