"""CPU checks of the SeqSLAM front-end: the NumPy oracle's own properties (tests/seqslam_oracle.py restates the two
definitions of include/dlc.h), the C ABI's new symbols, and the CLI's argument rules.  No GPU is used."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import seqslam_oracle as sq
from conftest import GOLDEN, ROOT


# ---- 1. the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out,n_in", [(1, 1), (3, 10), (5, 13), (7, 7), (24, 192), (64, 240), (32, 240)])
def test_weights_sum_to_the_source_length(n_out, n_in):
    w = sq.area_weights(n_out, n_in)
    assert w.shape == (n_out, n_in) and (w >= 0).all()
    assert (w.sum(axis=1) == n_in).all()              # over the source pixels of a cell: the cell's extent, n_in units
    assert (w.sum(axis=0) == n_out).all()             # over the cells: every source pixel is used up exactly


def test_resize_is_the_identity_at_full_size():
    rng = np.random.RandomState(0)
    g = rng.randint(0, 256, size=(3, 7, 9)).astype(np.uint8)
    assert np.array_equal(sq.resize(g, 7, 9), g)


def test_resize_is_the_rounded_block_mean_for_integer_ratios():
    rng = np.random.RandomState(1)
    g = rng.randint(0, 256, size=(12, 20)).astype(np.uint8)
    blocks = g.reshape(4, 3, 5, 4).astype(np.int64).sum(axis=(1, 3))         # 3 x 4 pixels per cell
    assert np.array_equal(sq.resize(g, 4, 5), (2 * blocks + 12) // 24)       # mean, rounded half up
    assert np.array_equal(sq.resize(np.full((10, 13), 255, np.uint8), 3, 5), np.full((3, 5), 255))
    assert np.array_equal(sq.resize(np.zeros((10, 13), np.uint8), 3, 5), np.zeros((3, 5), np.int64))


def test_flat_and_single_cell_tiles_are_128():
    g = np.full((1, 16, 16), 77, np.uint8)
    assert (sq.describe(g, (4, 4), 2, 32) == 128).all()                      # a constant image
    rng = np.random.RandomState(2)
    g = rng.randint(0, 256, size=(2, 10, 13)).astype(np.uint8)
    assert (sq.describe(g, (3, 5), 1, 127) == 128).all()                     # tiles of one cell
    d = sq.describe(g, (3, 5), 2, 32).reshape(2, 3, 5)
    assert (d[:, 2, 4] == 128).all()                                         # the clipped corner tile is one cell
    assert (d[:, :2, :4] != 128).any()


def test_normalisation_is_strength_times_the_z_score():
    t = np.array([[10, 20], [30, 40]], dtype=np.int64)
    z = (t - t.mean()) / t.std(ddof=1)
    assert np.array_equal(sq.normalise(t, 2, 32), np.rint(128 + 32 * z).astype(np.uint8))
    assert np.array_equal(sq.normalise(t, 64, 32), sq.normalise(t, 2, 32))   # one tile larger than the image
    checker = (np.indices((4, 4)).sum(axis=0) % 2 * 255).astype(np.int64)
    hi = sq.normalise(checker, 4, 127)
    assert set(np.unique(hi)) == {128 - 123, 128 + 123}                      # 127 * 15 / sqrt(240) = 122.97: inside the byte
    sharp = np.zeros((4, 4), np.int64)
    sharp[0, 0] = 255
    out = sq.normalise(sharp, 4, 127)
    assert out[0, 0] == 255 and (out[1:] == 128 - 32).all()                  # z = 3.75: 128 + 476 is clamped; the rest z = -0.25


def test_sad_properties():
    rng = np.random.RandomState(3)
    x = rng.randint(0, 256, size=(9, 37)).astype(np.uint8)
    m = sq.sad_rows(x, x)
    assert m.dtype == np.int64 and np.array_equal(m, m.T) and (np.diag(m) == 0).all()
    lo, hi = np.zeros((1, 5), np.uint8), np.full((1, 5), 255, np.uint8)
    assert sq.sad_rows(lo, hi)[0, 0] == 5 * 255 and sq.sad_rows(hi, lo)[0, 0] == 5 * 255     # 255, not 1: unsigned bytes
    assert np.array_equal(sq.offered(3, 4, 1, 1), np.array([[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0]], bool))
    assert not sq.offered(3, 4, 0, 0).any() and sq.offered(2, 4, 9, -1).all()


def test_golden_frames_give_ordinary_descriptors():
    """The real frames at 24 x 32: hardly any byte saturated, and most frames nearest to a neighbour in time."""
    from oracle import patches as opatch
    import real_frames
    gray = np.stack([opatch.bgr2gray_opencv(opatch.read_ppm(p)) for p in real_frames.frame_paths()])
    d = sq.describe(gray, (24, 32), 8, 32)
    assert d.shape == (20, 768) and ((d == 0) | (d == 255)).mean() < 0.01
    m = sq.sad_rows(d, d)
    off = m + np.eye(20, dtype=np.int64) * (1 << 40)
    assert m[~np.eye(20, dtype=bool)].min() > 0
    nearest = off.argmin(axis=1)
    assert (np.abs(nearest - np.arange(20)) == 1).mean() >= 0.75


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeploopcloser_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deeploopcloser_amd", "csrc"), "-j4"])
    return _lib.load()


def test_library_exports_the_front_end(lib):
    from deeploopcloser_amd import _lib
    assert lib.dlc_abi_version() == 20 and _lib.DLC_ABI_VERSION == 20
    assert hasattr(lib, "dlc_seqslam_describe_u8") and hasattr(lib, "dlc_sad_u8_rows")
    assert "dlc_seqslam_describe_u8" in _lib.SIGNATURES and "dlc_sad_u8_rows" in _lib.SIGNATURES
    buf = (C.c_uint8 * 64)()
    out = (C.c_int64 * 4)()
    assert lib.dlc_seqslam_describe_u8(None, buf, 1, 4, 4, 2, 2, 2, 32, buf, 4, None) == _lib.DLC_ERR_BAD_ARG
    assert lib.dlc_sad_u8_rows(None, buf, 1, 16, buf, 1, 16, 16, 1, 0, out, 1, None) == _lib.DLC_ERR_BAD_ARG


def test_package_exports_the_front_end():
    import deeploopcloser_amd as dlc
    for name in ("SeqSlam", "DifferenceCalculator", "SadKeyframeDatabase", "SeqSlamLoopClosureDetector"):
        assert hasattr(dlc, name) and name in dlc.__all__
    from deeploopcloser_amd import drivers, pipeline
    assert callable(drivers.create_difference_matrix) and callable(pipeline.seqslam_descriptors_from_frames)


# ---- 3. the CLI's argument rules ------------------------------------------------------------------------------------------
def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


SAD = ("--network", "seqslam", "--metric", "sad")


@pytest.mark.parametrize("args,message", [(("--network", "seqslam"), "--network seqslam and --metric sad need each other"),
                                          (("--metric", "sad", "--network", "cnn_vtl"), "--network seqslam and --metric sad need each other"),
                                          (SAD + ("--size", "24by32"), "--size must be HxW"),
                                          (SAD + ("--size", "0x32"), "--size must be HxW"),
                                          (SAD + ("--patch", "65"), "--patch must be 1..64"),
                                          (SAD + ("--contrast", "5"), "--contrast needs --sequence")])
def test_cli_refuses(args, message):
    """Each case is refused by the rule it names (not by argparse's choices: seqslam and sad are choices now)."""
    res = run_cli(*args)
    assert res.returncode == 2 and "usage:" in res.stderr and "error: " + message in res.stderr, res.stdout + res.stderr
