"""dlc_cnnvtl_distance_matrix (csrc/match_ref.hip) through the C ABI against oracle/distance.py, every cell equal, with both of
its loaders and rows the caller padded.

The kernel loads a row a word at a time when the base and the row pitch are 4-byte aligned (distance_matrix_kernel<true>:
the bytes of the last word past D are masked) and byte by byte otherwise (distance_matrix_kernel<false>).
Engine.cnnvtl_distance_matrix pads rows to 4-byte pitches with ZEROS, so the rest of the suite never runs the byte loader and
never shows the word loader's mask a non-zero byte.  Here the rows live in an int8 buffer whose bytes in [D, ldd) and whose
rows before and after are non-zero garbage, -128 included, and each (N, D) runs in three layouts:
  words   ldd % 4 == 0, base on a 4-byte boundary: the word loader, its tail mask facing garbage wherever D % 4 != 0;
  odd     ldd odd: the byte loader (every second row off any alignment);
  offset  ldd % 4 == 0, base + 1 byte: the byte loader.
N in {1, 63, 64, 65, 129}: below, at and above the 64 x 64 output tile, and three tile rows (only tiles on or above the
diagonal are computed, the others mirrored).  D in {1, 3, 63, 64, 65, 257, 1000, 2243}: below, at and above the word and the
64-byte step; 1000 and 2243 are cut into 4 and 9 chunks of 256 bytes over gridDim.z, the last with a tail of 232 and of
195, whose partial sums meet in 64-bit atomics.  Operands hold -128 and 127 and pairs whose XOR is -128 (|x| = 128: one bit).  out is
pre-filled with garbage inside a larger int64 buffer with sentinel bands: the bands stay untouched, the N x N block is the
oracle's.  Four cases go through Engine.cnnvtl_distance_matrix(desc, d=D) with garbage in the caller's padding.

The file runs in 3 s on an MI355X.  Mutation check (not committed): with the word loader's tail mask forced to all ones every
"words" case with D % 4 != 0 and N > 1 fails (N = 1 compares a row with itself: the garbage cancels) while every older test
of the distance kernels passes; with sa[r] ^ sb[c] replaced by sa[r] every case but N = D = 1 (one positive byte) fails."""
import functools

import numpy as np
import pytest
import torch

import distance_rows_oracle as dro

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 129]
DS = [1, 3, 63, 64, 65, 257, 1000, 2243]
BAND = 96                                        # int64 words on either side of out
LAYOUTS = ("words", "odd", "offset")


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()


def garbage(rng, shape):
    """Non-zero int8 bytes over the whole range, -128 planted."""
    g = rng.randint(1, 256, size=shape).astype(np.uint8).view(np.int8)           # 1 .. 127, -128 .. -1
    g.reshape(-1)[::7] = -128
    return g


@functools.lru_cache(maxsize=None)
def case(n, d):
    """Descriptors [n, d] with the edge values planted, and the oracle's matrix: computed once, shared by the layouts."""
    from oracle import distance as od
    rng = np.random.RandomState(n * 10007 + d)
    desc = dro.random_bytes(rng, (n, d))
    desc[0, 0], desc[n - 1, d - 1] = -128, 127
    if n > 1:                                                                   # pairs whose XOR is -128, in the first and last word
        desc[1, 0] = np.int8(-128) ^ desc[0, 0]                                 # 0 against -128
        desc[n - 2, d - 1] = np.int8(-128) ^ desc[n - 1, d - 1]                 # -1 against 127
        x = np.bitwise_xor(desc[0], desc[1])
        assert x[0] == -128 and np.bitwise_xor(desc[n - 2, d - 1], desc[n - 1, d - 1]) == -128
    assert desc.size == 1 or ((desc == -128).any() and (desc == 127).any())
    want = od.distance_matrix(desc)
    assert want.dtype == np.int64 and want.shape == (n, n)
    return desc, want


def pitch(d, layout):
    if layout == "odd":
        return d + 1 + (d & 1)
    return (d + 3) // 4 * 4 + 4                                                # words, offset: room for the offset byte and garbage


def rows_in_garbage(desc, layout, seed):
    """desc inside a garbage-filled [(n + 2) * ldd + 4] int8 device buffer, at row 1 (+ 1 byte for "offset").
    -> (buffer, byte offset of the first row, ldd, the buffer's host copy)."""
    n, d = desc.shape
    ldd = pitch(d, layout)
    host = garbage(np.random.RandomState(seed), (n + 2) * ldd + 4)
    start = ldd + (1 if layout == "offset" else 0)
    for r in range(n):
        host[start + r * ldd:start + r * ldd + d] = desc[r]
    assert (host != 0).sum() >= host.size - (desc == 0).sum()                   # nothing but the descriptors may be zero
    return torch.from_numpy(host).to("cuda"), start, ldd, host


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_every_cell_in_three_layouts(eng, n, d):
    desc, want = case(n, d)
    for li, layout in enumerate(LAYOUTS):
        buf, start, ldd, host = rows_in_garbage(desc, layout, n + 3 * d + li)
        ptr = buf.data_ptr() + start
        aligned = ptr % 4 == 0 and ldd % 4 == 0
        assert aligned == (layout == "words"), (layout, ptr % 4, ldd)          # the loader this layout is meant to reach
        # out: garbage in the block, a sentinel that differs from word to word around it
        total = n * n + 2 * BAND
        sentinel = -(np.arange(total, dtype=np.int64) * 2654435761 + 12345)
        out_host = sentinel.copy()
        out_host[BAND:BAND + n * n] = np.random.RandomState(d).randint(-2 ** 40, 2 ** 40, size=n * n)
        out = torch.from_numpy(out_host).to("cuda")
        eng._check(eng.lib.dlc_cnnvtl_distance_matrix(eng.ctx, ptr, n, d, ldd, out.data_ptr() + 8 * BAND, None))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:BAND], sentinel[:BAND]) and np.array_equal(got[BAND + n * n:], sentinel[BAND + n * n:]), layout
        block = got[BAND:BAND + n * n].reshape(n, n)
        assert np.array_equal(block, want), (layout, np.argwhere(block != want)[:4])
        assert np.array_equal(buf.cpu().numpy(), host), layout                 # the descriptors and the garbage are left alone


@pytest.mark.parametrize("n,d,width", [(65, 257, 260), (65, 257, 259), (129, 1000, 1001), (64, 63, 64)])
def test_engine_with_caller_padded_rows(eng, n, d, width):
    """Engine.cnnvtl_distance_matrix(desc, d=D) on rows the caller padded, the padding garbage: a 4-byte pitch (the word
    loader) and an odd one (the byte loader)."""
    desc, want = case(n, d)
    rows = garbage(np.random.RandomState(width), (n, width))
    rows[:, :d] = desc
    got = eng.cnnvtl_distance_matrix(torch.from_numpy(rows).to(eng.device), d=d)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    # ... and the same answer as the engine's own zero-padded copy of the bare rows
    assert torch.equal(got, eng.cnnvtl_distance_matrix(torch.from_numpy(desc).to(eng.device)))
