"""CPU checks of the binary place descriptor: the NumPy oracle's own properties (tests/ldb_oracle.py restates the two
definitions of include/dlc.h), the header's worked example, the C ABI's new symbols and host arithmetic, the package's
argument errors and the CLI's argument rules.  No GPU is used."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ldb_oracle as lo
from conftest import GOLDEN, ROOT


# ---- 1. the oracle --------------------------------------------------------------------------------------------------------
EXAMPLE = np.array([[1, 2, 5, 5], [3, 4, 5, 5], [9, 7, 0, 8], [9, 7, 8, 0]], dtype=np.uint8)


def test_worked_example_of_the_header():
    s, dx, dy = lo.cell_values(EXAMPLE.astype(np.int64), 2)
    assert s.tolist() == [10, 20, 32, 16] and dx.tolist() == [2, 0, -4, 0] and dy.tolist() == [4, 0, 0, 0]
    assert lo.n_bits((2,)) == 18 and lo.row_bytes((2,)) == 16
    row = lo.describe(EXAMPLE[None], (4, 4), (2,))
    assert row.shape == (1, 16) and row.dtype == np.uint8
    assert bytes(row[0]) == bytes([0xB6, 0x95, 0x00]) + bytes(13)
    header = open(os.path.join(ROOT, "include", "dlc.h")).read()
    assert "B6 95 00 followed by 13 zero bytes" in header


@pytest.mark.parametrize("levels,bits", [((2, 3, 4), 486), ((2, 4, 8), 6426), ((8,), 6048), ((5, 6, 7, 8), 12366)])
def test_bit_counts(levels, bits):
    assert lo.n_bits(levels) == bits
    assert lo.row_bytes(levels) == 16 * -(-bits // 128)


def test_pad_bits_are_zero():
    rng = np.random.RandomState(0)
    g = rng.randint(0, 256, size=(3, 48, 48)).astype(np.uint8)
    for levels in ((2, 3, 4), (3,), (2, 4)):
        rows = lo.describe(g, (48, 48), levels)
        bits = np.unpackbits(rows, axis=1, bitorder="little")
        assert rows.shape[1] == lo.row_bytes(levels) and bits[:, :lo.n_bits(levels)].any()
        assert not bits[:, lo.n_bits(levels):].any()


def test_constant_image_gives_zero_rows():
    for v in (0, 77, 255):
        assert not lo.describe(np.full((2, 37, 53), v, np.uint8), (12, 12), (2, 3)).any()


@pytest.mark.parametrize("a,b", [(1, 0), (1, 30), (2, 0), (3, 7), (5, 5)])
def test_gain_and_offset_change_no_bit(a, b):
    rng = np.random.RandomState(1)
    t = rng.randint(0, 51, size=(4, 24, 24))                         # 5 * 50 + 5 = 255: no clipping
    assert (a * t + b).max() <= 255
    same = lo.describe((a * t + b).astype(np.uint8), (24, 24), (2, 3, 4))
    assert np.array_equal(same, lo.describe(t.astype(np.uint8), (24, 24), (2, 3, 4)))
    assert np.array_equal(same, lo.describe_thumbs(a * t + b, (2, 3, 4)))


def test_hamming_rows_is_the_bit_count_of_the_xor():
    rng = np.random.RandomState(2)
    q = rng.randint(0, 256, size=(5, 37)).astype(np.uint8)
    db = rng.randint(0, 256, size=(9, 37)).astype(np.uint8)
    want = [[(int.from_bytes(bytes(a), "little") ^ int.from_bytes(bytes(b), "little")).bit_count() for b in db] for a in q]
    got = lo.hamming_rows(q, db)
    assert got.dtype == np.int64 and got.tolist() == want
    m = lo.hamming_rows(db, db)
    assert np.array_equal(m, m.T) and (np.diag(m) == 0).all()
    assert lo.hamming_rows(np.zeros((1, 816), np.uint8), np.full((1, 816), 255, np.uint8))[0, 0] == 6528


def test_real_frames_rolled_four_pixels_find_themselves():
    """The 20 real frames (the oracle's grey conversion) at 48 x 48, levels (2, 3, 4): every frame rolled 4 px to the right
    is nearest, of the 20 unrolled codes, to its own."""
    from oracle import patches as opatch
    import real_frames
    gray = np.stack([opatch.bgr2gray_opencv(opatch.read_ppm(p)) for p in real_frames.frame_paths()]).astype(np.uint8)
    assert gray.shape == (20, 192, 240)
    db = lo.describe(gray, (48, 48), (2, 3, 4))
    m = lo.hamming_rows(db, db)
    assert m[~np.eye(20, dtype=bool)].min() > 0                     # no two frames share a code
    rows = lo.hamming_rows(lo.describe(np.roll(gray, 4, axis=2), (48, 48), (2, 3, 4)), db)
    correct = int((rows.argmin(axis=1) == np.arange(20)).sum())
    true = np.diag(rows)
    wrong = np.where(np.eye(20, dtype=bool), 1 << 40, rows).min(axis=1)
    print("rolled 4 px: %d of 20 correct, median true %d, median best wrong %d" % (correct, np.median(true), np.median(wrong)))
    assert correct == 20


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeploopcloser_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deeploopcloser_amd", "csrc"), "-j4"])
    return _lib.load()


def test_library_exports_the_binary_descriptor(lib):
    from deeploopcloser_amd import _lib
    assert lib.dlc_abi_version() == 20 and _lib.DLC_ABI_VERSION == 20
    for name in ("dlc_ldb_row_bytes", "dlc_ldb_describe_u8", "dlc_hamming_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    buf = (C.c_uint8 * 64)()
    out = (C.c_int64 * 4)()
    lv = (C.c_int * 1)(2)
    assert lib.dlc_ldb_describe_u8(None, buf, 1, 4, 4, 4, 4, lv, 1, buf, 16, None) == _lib.DLC_ERR_BAD_ARG
    assert lib.dlc_hamming_rows(None, buf, 1, 16, buf, 1, 16, 16, 1, 0, out, 1, None) == _lib.DLC_ERR_BAD_ARG


def test_row_bytes_is_host_arithmetic(lib):
    def row_bytes(levels):
        return lib.dlc_ldb_row_bytes((C.c_int * max(1, len(levels)))(*levels), len(levels))
    assert row_bytes((2, 3, 4)) == 64
    for levels in ((2, 4, 8), (8,), (5, 6, 7, 8), (2,)):
        assert row_bytes(levels) == lo.row_bytes(levels)
    for bad in ((), (1,), (9,), (3, 2), (2, 2), (2, 3, 4, 5, 6)):
        assert row_bytes(bad) == 0, bad
    assert lib.dlc_ldb_row_bytes(None, 1) == 0


def test_package_exports_the_binary_descriptor():
    import deeploopcloser_amd as dlc
    for name in ("Ldb", "HammingCalculator", "HammingKeyframeDatabase", "LdbLoopClosureDetector"):
        assert hasattr(dlc, name) and name in dlc.__all__
    from deeploopcloser_amd import drivers, pipeline
    assert callable(drivers.create_hamming_matrix)
    assert callable(pipeline.ldb_descriptors_from_frames) and callable(pipeline.ldb_hamming_matrix_from_frames)
    assert hasattr(dlc.Engine, "ldb_describe") and hasattr(dlc.Engine, "hamming_rows")


# ---- 3. argument errors that need no GPU ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs", [dict(levels=()), dict(levels=(1,)), dict(levels=(9,)), dict(levels=(3, 2)),
                                    dict(levels=(2, 2)), dict(levels=(2, 3, 4, 5, 6)), dict(levels=(2.5,)), dict(levels=5),
                                    dict(size=(0, 48)), dict(size=(512, 256)), dict(size=(48, 50)),
                                    dict(size=(48, 48), levels=(5,))])
def test_ldb_refuses_before_it_needs_a_gpu(kwargs):
    import deeploopcloser_amd as dlc
    with pytest.raises(ValueError):
        dlc.Ldb(**kwargs)


def test_ldb_bits_of_the_package_agree_with_the_oracle():
    from deeploopcloser_amd.ldb import ldb_bits
    for levels in ((2, 3, 4), (2, 4, 8), (8,), (5, 6, 7, 8)):
        assert ldb_bits(levels) == lo.n_bits(levels)


@pytest.mark.parametrize("kwargs", [dict(k=0), dict(k=129), dict(exclusion=-1), dict(max_distance=-1), dict(dim=0),
                                    dict(capacity=0), dict(suppress=-1), dict(contrast=5), dict(sequence=4, steps=(3, 2))])
def test_detector_refuses_before_it_needs_a_gpu(kwargs):
    import deeploopcloser_amd as dlc
    args = dict(dim=64)
    args.update(kwargs)
    with pytest.raises(ValueError):
        dlc.LdbLoopClosureDetector(**args)


def test_detectors_share_one_body():
    import deeploopcloser_amd as dlc
    from deeploopcloser_amd import loop_closure
    base = loop_closure._ByteRowsLoopClosureDetector
    assert issubclass(dlc.LdbLoopClosureDetector, base) and issubclass(dlc.SeqSlamLoopClosureDetector, base)
    for cls in (dlc.LdbLoopClosureDetector, dlc.SeqSlamLoopClosureDetector):
        assert "query_and_insert" not in vars(cls) and "loops" not in vars(cls)
    # and all six stand on one base, which alone has loops and len(): the SDAV detector's loops adds its poison check
    root = loop_closure._StreamingDetector
    assert issubclass(base, root) and "loops" in vars(root) and "__len__" in vars(root)
    for cls in (dlc.LoopClosureDetector, dlc.SdavLoopClosureDetector, dlc.CnnVtlLoopClosureDetector,
                dlc.SeqSlamLoopClosureDetector, dlc.LdbLoopClosureDetector, dlc.FusedLoopClosureDetector):
        assert issubclass(cls, root)
        for c in cls.__mro__[:cls.__mro__.index(root)]:
            assert "__len__" not in vars(c)
            assert "loops" not in vars(c) or c is dlc.SdavLoopClosureDetector
    assert issubclass(dlc.CnnVtlLoopClosureDetector, base) and "query_and_insert" not in vars(dlc.CnnVtlLoopClosureDetector)


# ---- 4. the CLI's argument rules ------------------------------------------------------------------------------------------
def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


HAM = ("--network", "ldb", "--metric", "hamming")


@pytest.mark.parametrize("args,message", [(("--network", "ldb"), "--network ldb and --metric hamming need each other"),
                                          (("--metric", "hamming"), "--network ldb and --metric hamming need each other"),
                                          (HAM + ("--size", "48by48"), "--size must be HxW"),
                                          (HAM + ("--levels", "3,2"), "--levels must be 1 to 4 integers"),
                                          (HAM + ("--levels", "2,x"), "--levels must be 1 to 4 integers"),
                                          (HAM + ("--size", "32x64", "--levels", "2,3"), "--levels: twice every grid size"),
                                          (HAM + ("--max-distance", "1.5"), "--max-distance must be a non-negative integer"),
                                          (HAM + ("--contrast", "5"), "--contrast needs --sequence"),
                                          (("--levels", "2,3"), "--levels needs --network ldb")])
def test_cli_refuses(args, message):
    res = run_cli(*args)
    assert res.returncode == 2 and "usage:" in res.stderr and "error: " + message in res.stderr, res.stdout + res.stderr
