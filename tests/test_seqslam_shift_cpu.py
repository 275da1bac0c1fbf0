"""CPU checks of the lateral-shift tolerant SeqSLAM difference (dlc_sad_u8_shift_rows): the NumPy oracle's two forms
(tests/seqslam_shift_oracle.py: the definition of include/dlc.h, and a composition of the plain sad_rows oracle over cropped
copies) agree; ties, the largest sums, and the real-frame evidence the feature rests on; the C ABI's new symbol and the
CLI's argument rules.  No GPU is used."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import seqslam_oracle as sq
import seqslam_shift_oracle as ss
from conftest import GOLDEN, ROOT


# ---- 1. the oracle --------------------------------------------------------------------------------------------------------
def test_shift_order():
    assert ss.shift_order(0) == [0] and ss.shift_order(3) == [0, -1, 1, -2, 2, -3, 3]


@pytest.mark.parametrize("h,w,S", [(3, 5, 4), (1, 9, 8), (4, 16, 3), (32, 64, 8), (2, 70, 8)])
def test_the_two_forms_agree(h, w, S):
    rng = np.random.RandomState(h * 100 + w + S)
    q = rng.randint(0, 256, size=(5, h * w)).astype(np.uint8)
    db = rng.randint(0, 256, size=(7, h * w)).astype(np.uint8)
    db[3] = q[2]                                                       # an exact match: value 0 at shift 0
    v, s = ss.shift_rows(q, db, h, w, S)
    v2, s2 = ss.shift_rows_composed(q, db, h, w, S)
    assert v.dtype == np.int64 and s.dtype == np.int8 and v.shape == (5, 7)
    assert np.array_equal(v, v2) and np.array_equal(s, s2)
    assert v[2, 3] == 0 and s[2, 3] == 0
    assert (v <= sq.sad_rows(q, db)).all() and (np.abs(s) <= S).all() and len(np.unique(s)) > 1
    # S = 0 is the plain rows, shift 0 everywhere
    v0, s0 = ss.shift_rows(q, db, h, w, 0)
    assert np.array_equal(v0, sq.sad_rows(q, db)) and not s0.any()
    c0, cs0 = ss.shift_rows_composed(q, db, h, w, 0)
    assert np.array_equal(c0, v0) and not cs0.any()


def test_a_shifted_copy_is_found_with_its_sign():
    """The query's content is the key-frame's moved 2 columns to the left: shift +2, value 0."""
    rng = np.random.RandomState(5)
    a = rng.randint(0, 256, size=(4, 12)).astype(np.uint8)
    b = np.zeros_like(a)
    b[:, :10] = a[:, 2:]
    b[:, 10:] = rng.randint(0, 256, size=(4, 2))
    v, s = ss.shift_rows(b.reshape(1, -1), a.reshape(1, -1), 4, 12, 3)
    assert v[0, 0] == 0 and s[0, 0] == 2
    v, s = ss.shift_rows(a.reshape(1, -1), b.reshape(1, -1), 4, 12, 3)
    assert v[0, 0] == 0 and s[0, 0] == -2


def test_ties_go_to_the_first_in_the_order():
    flat = np.full((1, 24), 9, np.uint8)
    v, s = ss.shift_rows(flat, np.full((2, 24), 9, np.uint8), 3, 8, 4)
    assert not v.any() and not s.any()                                 # every shift gives 0: shift 0
    # v_-1 = v_+1 < v_0: one row, w = 3.  q = [0, 9, 0], d = [9, 0, 9]: shift 0 sums 27; shift -1 compares q[1], q[2] with
    # d[0], d[1]: 0 + 0; shift +1 compares q[0], q[1] with d[1], d[2]: 0 + 0 -- a tie of -1 and +1 below shift 0
    q, d = np.array([[0, 9, 0]], np.uint8), np.array([[9, 0, 9]], np.uint8)
    v, s = ss.shift_rows(q, d, 1, 3, 1)
    assert v[0, 0] == 0 and s[0, 0] == -1
    assert sq.sad_rows(q, d)[0, 0] == 27
    v2, s2 = ss.shift_rows_composed(q, d, 1, 3, 1)
    assert v2[0, 0] == 0 and s2[0, 0] == -1


@pytest.mark.parametrize("h", [1, 256])
def test_the_largest_sums(h):
    """All 0 against all 255 at h * w = 65536, S = 8: every v_s is floor(255 * h * (w - |s|) * w / (w - |s|)) = 255 * 65536 in
    Python's integers -- the rescaling of the largest sums of this size is exact and shift 0 wins the 17-fold tie."""
    w = 65536 // h
    q, d = np.zeros((1, 65536), np.uint8), np.full((1, 65536), 255, np.uint8)
    want = min((255 * h * (w - abs(s)) * w) // (w - abs(s)) for s in ss.shift_order(8))
    assert want == 255 * 65536
    for form in (ss.shift_rows, ss.shift_rows_composed):
        v, s = form(q, d, h, w, 8)
        assert int(v[0, 0]) == want and s[0, 0] == 0


def green_crops(dx, width=192):
    """(A, B): uint8 [20, 192, width] -- the green channel of the 20 real frames, columns 0 .. width-1 and dx .. dx+width-1."""
    from oracle import patches as opatch
    import real_frames
    g = np.stack([opatch.read_ppm(p)[:, :, 1] for p in real_frames.frame_paths()])
    assert g.shape == (20, 192, 240)
    return np.ascontiguousarray(g[:, :, :width]), np.ascontiguousarray(g[:, :, dx:dx + width])


def test_real_frames_revisited_an_eighth_of_the_width_to_the_side():
    """The revisit displaced by 24 source pixels = 8 thumbnail columns = one normalisation tile: the plain SAD of the true
    pair rises to the level of the wrong pairs and loses rows; the best of +-8 columns is exact."""
    a, b = green_crops(24)
    da, dq = sq.describe(a, (32, 64), 8, 32), sq.describe(b, (32, 64), 8, 32)
    v, s = ss.shift_rows(dq, da, 32, 64, 8)
    truth = np.arange(20)
    assert (np.diag(v) == 0).all() and (np.diag(s) == 8).all()
    assert np.array_equal(v.argmin(axis=1), truth)
    plain = sq.sad_rows(dq, da)
    wrong = int((plain.argmin(axis=1) != truth).sum())
    assert wrong >= 1
    assert wrong == 8 and np.diag(plain).min() == 50026 and np.diag(plain).max() == 60896     # as measured for the issue


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeploopcloser_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deeploopcloser_amd", "csrc"), "-j4"])
    return _lib.load()


def test_library_exports_the_shifted_rows(lib):
    from deeploopcloser_amd import _lib
    assert lib.dlc_abi_version() == 20 and _lib.DLC_ABI_VERSION == 20
    assert hasattr(lib, "dlc_sad_u8_shift_rows") and "dlc_sad_u8_shift_rows" in _lib.SIGNATURES
    assert _lib.DLC_MAX_SHIFT == 8
    header = open(os.path.join(ROOT, "include", "dlc.h")).read()
    assert "#define DLC_MAX_SHIFT %d\n" % _lib.DLC_MAX_SHIFT in header
    buf = (C.c_uint8 * 64)()
    out = (C.c_int64 * 4)()
    sh = (C.c_int8 * 4)()
    assert lib.dlc_sad_u8_shift_rows(None, buf, 1, 16, buf, 1, 16, 2, 8, 3, 1, 0, out, 1, sh, 1, None) == _lib.DLC_ERR_BAD_ARG
    assert lib.dlc_sad_u8_shift_rows(None, buf, 1, 16, buf, 1, 16, 2, 8, 3, 1, 0, out, 1, None, 0, None) == _lib.DLC_ERR_BAD_ARG


def test_python_surface_takes_the_shift():
    import inspect
    import deeploopcloser_amd as dlc
    from deeploopcloser_amd import drivers, pipeline
    for fn, names in ((dlc.Engine.sad_rows, ("shift", "width", "shift_out")),
                      (dlc.DifferenceCalculator.difference_rows, ("shift", "width", "return_shift")),
                      (dlc.DifferenceCalculator.difference_matrix, ("shift", "width", "return_shift")),
                      (dlc.SadKeyframeDatabase.differences, ("shift", "width", "return_shift")),
                      (dlc.SeqSlamLoopClosureDetector.__init__, ("shift", "width")),
                      (pipeline.seqslam_difference_matrix_from_frames, ("shift",)),
                      (drivers.create_difference_matrix, ("shift",))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params and params[name].default in (None, False), (fn, name)


# ---- 3. the CLI's argument rules ------------------------------------------------------------------------------------------
def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


SAD = ("--network", "seqslam", "--metric", "sad")


@pytest.mark.parametrize("args,message", [(("--shift", "2"), "--shift needs --network seqslam"),
                                          (("--network", "cnn_vtl", "--metric", "distance", "--shift", "2"),
                                           "--shift needs --network seqslam"),
                                          (SAD + ("--shift", "-1"), "--shift must be 0..8"),
                                          (SAD + ("--shift", "9"), "--shift must be 0..8"),
                                          (SAD + ("--size", "8x4", "--shift", "4"), "--shift must be 0..8")])
def test_cli_refuses(args, message):
    res = run_cli(*args)
    assert res.returncode == 2 and "usage:" in res.stderr and "error: " + message in res.stderr, res.stdout + res.stderr
