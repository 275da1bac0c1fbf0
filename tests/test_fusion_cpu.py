"""CPU checks of the multi-descriptor fusion (dlc_fuse_rows): the NumPy oracle of the definition in include/dlc.h
(tests/fusion_oracle.py) pinned on its own -- the two forms of TREE, that the order matters, padding, the consequences the
header states -- the C ABI's new symbols and host-side rejections, the Python surface and the CLI's argument rules.
No GPU is used."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_oracle as fo
from conftest import GOLDEN, ROOT
from sequence_oracle import same_bits


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---- 1. TREE ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_the_two_tree_forms_agree(c):
    rng = np.random.RandomState(c)
    a = rng.randn(3, c) * 10.0 ** rng.randint(-3, 4, size=(3, c))
    got = fo.tree_rows(a)
    for r in range(3):
        assert bits(got[r]) == bits(fo.tree_recursive(a[r]))


def test_tree_is_not_the_left_to_right_sum():
    """RandomState(11).randn(1000): the tree and a sequential loop round differently, so a kernel (or an oracle) that sums
    in the wrong order cannot pass the bit comparisons."""
    v = np.random.RandomState(11).randn(1000)
    t, s = fo.tree_recursive(v), fo.left_to_right(v)
    assert bits(t) != bits(s) and abs(t - s) < 1e-10
    assert fo.tree_recursive([1.0, 2.0, 3.0]) == 6.0 and bits(fo.tree_recursive([-0.0])) == bits(-0.0)
    # hand-worked: (1e16 + 1) + (1 + 1) = 1e16 + 2 in the tree; left to right the ones are lost one by one
    v = np.array([1e16, 1.0, 1.0, 1.0])
    assert fo.tree_recursive(v) == 1e16 + 2.0 and fo.left_to_right(v) == 1e16


@pytest.mark.parametrize("c", [1, 3, 255, 256, 257, 1000, 5000])
def test_padding_to_a_larger_power_of_two_keeps_the_bits(c):
    a = np.random.RandomState(c + 1).randn(2, c)
    a[1, 0] = -0.0
    if c == 1:
        a[0, 0] = -0.0                                            # a sum that is -0.0 stays -0.0 under the padding
    base = fo.tree_rows(a)
    p = 1
    while p < c:
        p *= 2
    for pad in (p, 2 * p, 8 * p):
        assert np.array_equal(bits(fo.tree_rows(a, pad_to=pad)), bits(base))


def test_a_kernel_shaped_evaluation_gives_the_tree():
    """Four cells per lane as (x0 + x1) + (x2 + x3), an xor-butterfly over 64 lanes, then a tree over 256-column chunks."""
    for c in (1, 3, 255, 256, 257, 1000, 5000):
        v = np.random.RandomState(c + 7).randn(c)
        chunks = -(-c // 256)
        x = np.full(chunks * 256, -0.0)
        x[:c] = v
        lanes = x.reshape(chunks, 64, 4)
        s = (lanes[:, :, 0] + lanes[:, :, 1]) + (lanes[:, :, 2] + lanes[:, :, 3])
        for off in (1, 2, 4, 8, 16, 32):
            s = s + s[:, np.arange(64) ^ off]
        assert (bits(s) == bits(s[:, :1])).all()                  # every lane ends with the chunk's node
        assert bits(fo.tree_rows(s[:, 0][None, :])[0]) == bits(fo.tree_recursive(v))


# ---- 2. the definition's consequences -----------------------------------------------------------------------------------------
def sources(rows, n, seed):
    rng = np.random.RandomState(seed)
    return [rng.randn(rows, n), rng.randn(rows, n).astype(np.float32),
            rng.randint(-2 ** 62, 2 ** 62, size=(rows, n)).astype(np.int64)]


def test_one_source_without_a_norm_is_a_conversion_copy():
    for s in sources(3, 37, 0):
        got = fo.fuse_rows([s], norm="none")
        assert same_bits(got, s.astype(np.float64))
    got = fo.fuse_rows([sources(3, 37, 0)[0]], norm="none", lower_is_better=True)
    assert same_bits(got, -sources(3, 37, 0)[0])


def test_zscore_negation_with_the_flag_leaves_the_bits():
    a, b, _ = sources(4, 130, 1)
    one = fo.fuse_rows([a, b], weights=[1.0, -0.5], lower_is_better=[False, True], limit0=120, limit_step=3)
    two = fo.fuse_rows([-a, -b], weights=[1.0, -0.5], lower_is_better=[True, False], limit0=120, limit_step=3)
    assert same_bits(one, two) and np.isnan(one[0, 120:]).all() and not np.isnan(one[0, :120]).any()


@pytest.mark.parametrize("norm", fo.NORMS)
def test_constant_rows_and_short_rows(norm):
    x = np.full((4, 6), 3.5)
    got = fo.fuse_rows([x], norm=norm, limit0=0, limit_step=1)    # c = 0, 1, 2, 3
    assert np.isnan(got[0]).all() and np.isnan(got[1, 1:]).all() and np.isnan(got[2, 2:]).all()
    want = 3.5 if norm == "none" else 0.0
    assert (got[1, :1] == want).all() and (got[2, :2] == want).all() and (got[3, :3] == want).all()
    y = np.array([[1.0, 3.0, 9.0]])
    two = fo.fuse_rows([y], norm=norm, limit0=2)[0]
    if norm == "zscore":                                          # mean 2, sd sqrt(2)
        assert same_bits(two[:2], np.array([-1.0, 1.0]) / np.sqrt(2.0))
    elif norm == "minmax":
        assert two[:2].tolist() == [0.0, 1.0]
    assert np.isnan(two[2])


@pytest.mark.parametrize("norm", ["zscore", "minmax"])
def test_a_nan_makes_the_row_nan(norm):
    x = np.random.RandomState(2).randn(2, 40)
    x[1, 17] = np.nan
    got = fo.fuse_rows([x, x], norm=norm)
    assert np.isnan(got[1]).all() and not np.isnan(got[0]).any()
    x[1, 17] = np.inf
    assert np.isnan(fo.fuse_rows([x], norm="zscore")[1]).all()


def test_minmax_lies_in_the_unit_interval():
    a, b, c = sources(5, 300, 3)
    for s, lib in ((a, False), (b, True), (c, False), (c, True)):
        got = fo.fuse_rows([s], norm="minmax", lower_is_better=lib)
        assert (got >= 0.0).all() and (got <= 1.0).all() and (got.min(1) == 0.0).all() and (got.max(1) == 1.0).all()
        best = np.argmin(s, 1) if lib else np.argmax(s, 1)
        assert (got[np.arange(5), best] == 1.0).all()
    z = np.array([[0.0, -0.0, 0.0]])                              # -0.0 below +0.0: lo = -0.0, hi = +0.0, range 0
    assert (fo.fuse_rows([z], norm="minmax") == 0.0).all()


def test_the_planted_scene_needs_both_members():
    a, d, true = fo.two_confusers_scene()
    rows = np.arange(a.shape[0])
    assert (np.argmax(a, 1) != true).all() and (np.argmin(d, 1) != true).all()
    assert (np.argmax(a, 1) != np.argmin(d, 1)).all()
    fused = fo.fuse_rows([a, d], lower_is_better=[False, True])
    assert (np.argmax(fused, 1) == true).all()
    second = np.sort(fused, 1)[:, -2]
    assert (fused[rows, true] - second > 1.0).all()               # by more than one standard deviation of a member


# ---- 3. the C ABI and the Python surface --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeploopcloser_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deeploopcloser_amd", "csrc"), "-j4"])
    return _lib.load()


def test_the_library_exports_the_entry_points(lib):
    from deeploopcloser_amd import _lib
    for name in ("dlc_fuse_rows", "dlc_fuse_rows_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dlc_abi_version() == 20 and _lib.DLC_ABI_VERSION == 20
    header = open(os.path.join(ROOT, "include", "dlc.h")).read()
    assert "#define DLC_MAX_FUSE %d\n" % _lib.DLC_MAX_FUSE in header and _lib.DLC_MAX_FUSE == 8
    assert "enum { DLC_FUSE_NONE = %d, DLC_FUSE_ZSCORE = %d, DLC_FUSE_MINMAX = %d };" % (
        _lib.DLC_FUSE_NONE, _lib.DLC_FUSE_ZSCORE, _lib.DLC_FUSE_MINMAX) in header
    assert "enum { DLC_FUSE_PLAN_AUTO = %d, DLC_FUSE_PLAN_ROW = %d, DLC_FUSE_PLAN_SLAB = %d };" % (
        _lib.DLC_FUSE_PLAN_AUTO, _lib.DLC_FUSE_PLAN_ROW, _lib.DLC_FUSE_PLAN_SLAB) in header


def test_a_null_context_is_a_bad_argument(lib):
    from deeploopcloser_amd import _lib
    buf = (C.c_double * 8)()
    out = (C.c_double * 8)()
    src = (C.c_void_p * 1)(C.addressof(buf))
    rc = lib.dlc_fuse_rows(None, 1, (C.c_int * 1)(_lib.DLC_F64), src, (C.c_int64 * 1)(8), (C.c_double * 1)(1.0), (C.c_int * 1)(0),
                           1, 8, 8, 0, _lib.DLC_FUSE_ZSCORE, _lib.DLC_FUSE_PLAN_AUTO, out, 8, None, 0, None)
    assert rc == _lib.DLC_ERR_BAD_ARG and not any(out)


def test_workspace_bytes(lib):
    f = lib.dlc_fuse_rows_workspace_bytes
    assert f(32, 100000, 3) >= 2 * 8 * 3 * 32 * 25 and f(32, 100000, 3) % 16 == 0
    assert 0 < f(1, 1, 1) <= f(1, 4097, 1) <= f(2, 4097, 8)
    assert f(1, 2 ** 31 - 1, 8) > 0
    for rows, n, m in ((0, 10, 1), (-1, 10, 1), (10, 0, 1), (10, -5, 1), (1, 2 ** 31, 1), (1, 2 ** 40, 2), (4, 10, 0), (4, 10, 9),
                       (4, 10, -1)):
        assert f(rows, n, m) == 0, (rows, n, m)


def test_the_python_surface():
    import inspect
    import deeploopcloser_amd as dlc
    for name in ("fuse_scores", "FusedLoopClosureDetector"):
        assert name in dlc.__all__ and hasattr(dlc, name)
    p = inspect.signature(dlc.Engine.fuse_rows).parameters
    assert [k for k in p][1:] == ["sources", "weights", "lower_is_better", "norm", "n", "limit0", "limit_step", "out", "plan"]
    assert p["norm"].default == "zscore" and p["plan"].default is None and p["lower_is_better"].default is False
    p = inspect.signature(dlc.fuse_scores).parameters
    assert list(p) == ["matrices", "weights", "lower_is_better", "norm", "limit0", "limit_step"]
    p = inspect.signature(dlc.FusedLoopClosureDetector.__init__).parameters
    assert list(p)[1:] == ["members", "weights", "norm", "k", "threshold", "exclusion", "capacity", "device", "sequence", "slopes",
                           "contrast", "suppress", "steps", "chains"]
    assert p["k"].default == 5 and p["exclusion"].default == 30 and p["capacity"].default == 4096 and p["threshold"].default is None


# ---- 4. the CLI's argument rules ----------------------------------------------------------------------------------------------
def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


@pytest.mark.parametrize("args,message", [
    (("--fuse", "sad"), "--fuse takes two or three different members"),
    (("--fuse", "sad,sdav"), "--fuse takes two or three different members"),
    (("--fuse", "sad,sad"), "--fuse takes two or three different members"),
    (("--fuse", "sad,distance", "--fuse-weights", "1"), "--fuse-weights: 1 weights for 2 members"),
    (("--fuse", "sad,distance", "--fuse-weights", "1,x"), "--fuse-weights must be numbers"),
    (("--fuse", "sad,distance", "--fuse-weights", "1,inf"), "--fuse-weights must be finite"),
    (("--fuse", "sad,distance", "--fuse-weights", "nan,1"), "--fuse-weights must be finite"),
    (("--fuse-weights", "1,1"), "--fuse-weights and --fuse-norm need --fuse"),
    (("--fuse-norm", "minmax"), "--fuse-weights and --fuse-norm need --fuse"),
    (("--fuse", "sad,distance", "--fuse-norm", "softmax"), "argument --fuse-norm: invalid choice"),
    (("--fuse", "sad,distance", "--network", "seqslam", "--metric", "sad"), "--fuse chooses the descriptors and the measures itself: it excludes --network and --metric"),
    (("--fuse", "sad,distance", "--metric", "distance"), "--fuse chooses the descriptors and the measures itself: it excludes --network and --metric"),
    (("--fuse", "distance,cosine", "--shift", "2"), "--shift needs --network seqslam"),
    (("--fuse", "sad,distance", "--shift", "9"), "--shift must be 0..8"),
    (("--fuse", "sad,distance", "--contrast", "3"), "--contrast needs --sequence"),
    (("--fuse", "sad,distance", "--sequence", "65"), "--sequence must be 1..64"),
])
def test_cli_refuses(args, message):
    res = run_cli(*args)
    assert res.returncode == 2 and "usage:" in res.stderr and "error: " + message in res.stderr, res.stdout + res.stderr
    assert res.stdout == ""
