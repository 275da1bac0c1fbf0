"""The sign-random-projection hash without a GPU: tests/lsh_oracle.py (the NumPy restatement of include/dlc.h and of
lsh.lsh_planes) against per-element loops and the header's worked examples, the generator, the header's constants, the
CLI's refusals, and a planted stream through the oracle alone."""
import os
import re
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT
import lsh_oracle as lo


def test_worked_examples():
    q = lo.quantize(np.array([[0.5, -1.0, 0.25, 0.0]]))
    assert q.dtype == np.int8 and q.tolist() == [[64, -127, 32, 0]]              # 63.5 ties to the even 64
    pl = np.array([[1, 1, 1, 1], [-1, 1, 1, -1], [1, 1, -1, -1], [1, -1, 1, 1]], dtype=np.int8)
    qq = np.array([[3, -2, 0, 1]], dtype=np.int8)
    assert lo.sums(qq, pl).tolist() == [[2, -6, 0, 6]]
    row = lo.hash_rows(qq, pl)
    assert row.shape == (1, 16) and row.dtype == np.uint8 and row[0].tolist() == [0x09] + [0] * 15


def test_mix64_and_row_bytes():
    assert lo.mix64(0) == 0xE220A8397B1DCDAF
    assert [lo.row_bytes(b) for b in (0, 1, 128, 129, 1000, 8192, 8193)] == [0, 16, 16, 32, 128, 1024, 0]


def test_header_constants_equal_the_bindings():
    from deeploopcloser_amd import _lib
    header = open(os.path.join(ROOT, "include", "dlc.h")).read()
    for name in ("DLC_LSH_MAX_BITS", "DLC_LSH_MAX_D", "DLC_LSH_CHUNK", "DLC_LSH_SPLIT_MAX_ROWS"):
        (value,) = re.findall(r"#define %s (\d+)\b" % name, header)
        assert int(value) == getattr(_lib, name), name
    assert "enum { DLC_LSH_PLAN_AUTO = 0, DLC_LSH_PLAN_ONE_PASS = 1, DLC_LSH_PLAN_SPLIT = 2 };" in header
    assert (_lib.DLC_LSH_PLAN_AUTO, _lib.DLC_LSH_PLAN_ONE_PASS, _lib.DLC_LSH_PLAN_SPLIT) == (lo.AUTO, lo.ONE_PASS, lo.SPLIT) == (0, 1, 2)
    assert (_lib.DLC_LSH_MAX_BITS, _lib.DLC_LSH_MAX_D, _lib.DLC_LSH_CHUNK, _lib.DLC_LSH_SPLIT_MAX_ROWS) == \
        (lo.MAX_BITS, lo.MAX_D, lo.CHUNK, lo.SPLIT_MAX_ROWS)
    assert 128 * 128 * _lib.DLC_LSH_MAX_D < 1 << 31 <= 128 * 128 * (_lib.DLC_LSH_MAX_D + 1)
    for name in ("dlc_lsh_quantize_i8", "dlc_lsh_row_bytes", "dlc_lsh_hash_workspace_bytes", "dlc_lsh_hash_i8"):
        assert name in _lib.SIGNATURES


def test_package_exports():
    import deeploopcloser_amd as dlc
    for name in ("Lsh", "lsh_planes", "HashedLoopClosureDetector"):
        assert hasattr(dlc, name) and name in dlc.__all__
    assert dlc.lsh.Lsh is dlc.Lsh and issubclass(dlc.HashedLoopClosureDetector, dlc.LdbLoopClosureDetector)


def test_quantize_oracle_against_a_loop():
    rng = np.random.RandomState(1)
    x = rng.standard_normal((6, 9))
    x[1] = 0.0
    x[2, 3] = np.nan
    x[3, 0] = -np.inf
    x[4] = [0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 127.0, 0.0]                     # m = 127, s = 1: ties of both parities
    mean = rng.standard_normal(9)
    for mu in (None, mean):
        got = lo.quantize(x, mu)
        for r in range(x.shape[0]):
            t = [float(x[r, d]) - (float(mu[d]) if mu is not None else 0.0) for d in range(x.shape[1])]
            m = max(abs(v) for v in t) if all(np.isfinite(t)) else None
            for d in range(x.shape[1]):
                want = 0 if (m is None or m == 0) else int(round(t[d] * (127.0 / m)))        # Python's round: ties to even
                assert got[r, d] == want, (r, d)
    assert lo.quantize(np.array([[0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 127.0, 0.0]]))[0].tolist() == [0, 2, 2, 4, 0, -2, -2, 127, 0]
    assert lo.quantize(np.array([[5e-324, -5e-324, 0.0]]))[0].tolist() == [127, -127, 0]      # 127 / m overflows: clamped


def test_hash_oracle_against_a_loop():
    rng = np.random.RandomState(2)
    for rows, bits, d in ((1, 1, 1), (3, 7, 5), (2, 9, 17), (4, 130, 3)):
        q = rng.randint(-128, 128, size=(rows, d)).astype(np.int8)
        pl = rng.randint(-128, 128, size=(bits, d)).astype(np.int8)
        got = lo.hash_rows(q, pl)
        assert got.shape == (rows, lo.row_bytes(bits))
        for r in range(rows):
            for t in range(8 * got.shape[1]):
                s = sum(int(q[r, c]) * int(pl[t, c]) for c in range(d)) if t < bits else 0
                assert (got[r, t >> 3] >> (t & 7)) & 1 == int(s > 0), (r, t)
    a = lo.hash_rows(q, pl)
    flipped = a.copy()
    flipped[0, 0] ^= 0x05
    assert lo.hamming(a, a).diagonal().tolist() == [0] * 4 and lo.hamming(flipped, a)[0, 0] == 2


def test_planes_are_the_stated_generator():
    from deeploopcloser_amd.lsh import lsh_planes, mix64
    assert int(mix64(0)[0]) == 0xE220A8397B1DCDAF
    assert [int(v) for v in mix64([1, 2 ** 64 - 1])] == [lo.mix64(1), lo.mix64(2 ** 64 - 1)]
    for n_bits, d, seed in ((3, 1, 0), (5, 63, 1), (4, 64, 2), (3, 65, 2 ** 64 - 1), (2, 200, 12345), (16, 4096, 0)):
        p = lsh_planes(n_bits, d, seed)
        assert p.dtype == np.int8 and p.shape == (n_bits, d) and p.flags.c_contiguous
        assert np.array_equal(p, lo.planes(n_bits, d, seed)), (n_bits, d, seed)
    p = lsh_planes(1024, 4096, 0)
    assert np.array_equal(np.abs(p), np.ones_like(p))
    assert np.abs(p.astype(np.int64).sum(axis=1)).max() <= 5 * np.sqrt(4096)
    assert np.array_equal(p[:16], lo.planes(16, 4096, 0))
    assert not np.array_equal(lsh_planes(4, 64, 0), lsh_planes(4, 64, 1))


def run_loop_closure(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_hash_argparse_errors():
    for args in (("--hash", "nothing.npz"), ("--network", "sdav", "--metric", "similarity", "--hash", "nothing.npz"),
                 ("--network", "ldb", "--metric", "hamming", "--hash", "nothing.npz")):
        r = run_loop_closure(*args)
        assert r.returncode == 2 and "--hash needs --network sdav --metric cosine" in r.stderr and r.stdout == "", args
    r = run_loop_closure("--network", "sdav", "--metric", "hamming")             # as before: hamming keeps needing ldb
    assert r.returncode == 2 and "--network ldb and --metric hamming need each other" in r.stderr
    r = run_loop_closure("--network", "sdav", "--metric", "cosine", "--sequence", "3")       # and --sequence its metrics
    assert r.returncode == 2 and "--sequence needs --metric similarity, sad or hamming (or --fuse)" in r.stderr
    r = run_loop_closure("--network", "sdav", "--metric", "cosine", "--hash", "nothing.npz")
    assert r.returncode == 2 and "--hash: " in r.stderr and r.stdout == ""       # a model that is not there


def test_planted_stream_through_the_oracle():
    """40 places, D = 200, 256 bits, a revisit = the place + uniform noise of amplitude 0.25, centred by the places' mean:
    every revisit's nearest code is its place, and the largest true distance lies below the smallest wrong one."""
    base, again = lo.planted_stream(places=40, d=200, amplitude=0.25, seed=0)
    mean = base.mean(axis=0)
    pl = lo.planes(256, 200, seed=0)
    a = lo.hash_rows(lo.quantize(base, mean), pl)
    b = lo.hash_rows(lo.quantize(again, mean), pl)
    dist = lo.hamming(b, a)                                                       # [revisit, place]
    true = dist.diagonal()
    wrong = dist + np.where(np.eye(40, dtype=bool), 1 << 20, 0)
    print("planted stream, centred: largest true distance %d, smallest wrong %d" % (true.max(), wrong.min()))
    assert (dist.argmin(axis=1) == np.arange(40)).all()
    assert true.max() < wrong.min()
