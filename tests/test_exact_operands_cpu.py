"""tests/exact_operands.py on the CPU: the premise (the fp64 product of the drawn operands IS the integer product), its
independence of the summation order, and that a NumPy emulation of a tiled / split-K GEMM with one modelled defect each
gives a result the exact comparison and the guard bands see.  The HIP kernels are held to the same checks in
tests/test_gpu_gemm_f64_operands.py."""
import numpy as np
import pytest
import torch

import exact_operands as xo

TK = 16                        # the K tile of both fp64 kernels


@pytest.mark.parametrize("m,n,k", [(70, 130, 4096), (257, 98, 8190), (1, 1, 1), (37, 53, 29)])
def test_premise_float_product_is_the_integer_product(m, n, k):
    ai, bi, ci = xo.draw_integers(np.random.RandomState(m + n + k), m, n, k)
    a, b, bias = xo.to_float(ai, bi, ci)
    assert np.abs(ai).max() <= 512 and np.abs(bi).max() <= 512 and ci.min() >= -2 ** 15 and ci.max() < 2 ** 15
    assert np.array_equal(a * 2.0 ** 9, ai) and np.array_equal(b * 2.0 ** 15, bi) and np.array_equal(bias * 2.0 ** 15, ci)
    assert np.abs(ai @ bi).max() < 2 ** 31
    assert np.array_equal(xo.product(a, b), xo.int_product(ai, bi))
    assert np.array_equal(xo.product(a, b, bias), xo.int_product(ai, bi, ci))


def test_premise_is_refused_where_it_breaks():
    xo.check_premise(8192)
    xo.check_premise(2 ** 35 - 1)
    for k in (0, 2 ** 35, 2 ** 40):
        with pytest.raises(ValueError):
            xo.check_premise(k)
    with pytest.raises(ValueError):
        xo.draw_integers(np.random.RandomState(0), 1, 1, 0)


@pytest.mark.parametrize("m,n,k", [(70, 130, 4096), (33, 50, 8192), (300, 250, 2500)])
def test_product_is_independent_of_the_k_order(m, n, k):
    a, b, bias = xo.draw(np.random.RandomState(m * n + k), m, n, k)
    z = xo.product(a, b)
    assert np.array_equal(a[:, ::-1] @ b[::-1], z)
    perm = np.random.RandomState(1).permutation(k)
    assert np.array_equal(a[:, perm] @ b[perm], z)
    for chunk in (16, 144, 512, 640):
        forward = np.zeros((m, n))
        for k0 in range(0, k, chunk):
            forward += a[:, k0:k0 + chunk] @ b[k0:k0 + chunk]
        backward = np.zeros((m, n))
        for k0 in reversed(range(0, k, chunk)):
            backward += a[:, k0:k0 + chunk] @ b[k0:k0 + chunk]
        assert np.array_equal(forward, z) and np.array_equal(backward, z), chunk
    # one k at a time, as an fma chain sums: still no rounding
    rows = a[:3]
    chain = np.zeros((3, n))
    for kk in range(k):
        chain += rows[:, kk:kk + 1] * b[kk:kk + 1]
    assert np.array_equal(chain, z[:3])
    assert 0.3 < (z + bias).std() < 1.0                               # a sigmoid behind it is not saturated


def test_sigmoid_reference_is_a_rounding_of_the_extended_value():
    z = np.linspace(-8, 8, 4001)
    s = xo.sigmoid_ref(z)
    plain = 1.0 / (1.0 + np.exp(-z))
    assert np.all(np.abs(s - plain) <= 2 * np.spacing(s)) and s[2000] == 0.5
    if np.finfo(np.longdouble).nmant > 52:
        exact = 1.0 / (1.0 + np.exp(-z.astype(np.longdouble)))
        assert np.all(np.abs(s.astype(np.longdouble) - exact) <= 0.5 * np.spacing(s) * (1 + 2.0 ** -9))


# ---- a NumPy emulation of the kernels' structure, with one defect at a time --------------------------------------------
def emulate(a_buf, b, bias, K, ldc, kchunk=None, defect=None, block=(16, 32, 16, 32)):
    """C = A . B + bias as a tiled kernel forms it, into a sentinel-banded [M + 2, ldc] buffer.  a_buf [M, lda] holds A in
    its first K columns and whatever the caller put behind them.  K is walked in tiles of 16, the tiles of a chunk of
    kchunk (a multiple of 16; None: one pass) summed in order and the chunks' partial sums added in chunk order.
    defect, in the output block rows r0:r1, columns c0:c1 given by `block` where it is local:
      "drop_last_k"     the last k element of the LAST K tile is left out
      "pad_k"           the last K tile's mask is one too wide on A: A's column K (padding) times a masked B (0.0)
      "chunk0_dropped"  the reduce starts at chunk 1
      "column_past_n"   column N of C is stored (a clamped column's value)"""
    M, N = a_buf.shape[0], b.shape[1]
    r0, r1, c0, c1 = block
    kchunk = kchunk or -(-K // TK) * TK
    assert kchunk % TK == 0
    parts = []
    for k_lo in range(0, K, kchunk):
        k_hi = min(K, k_lo + kchunk)
        acc = np.zeros((M, N))
        for t0 in range(k_lo, k_hi, TK):
            t1 = min(k_hi, t0 + TK)
            acc += a_buf[:, t0:t1] @ b[t0:t1]
            if t1 == K and defect == "drop_last_k":
                acc[r0:r1, c0:c1] -= a_buf[r0:r1, K - 1:K] * b[K - 1:K, c0:c1]
            if t1 == K and defect == "pad_k":
                acc[r0:r1, c0:c1] += a_buf[r0:r1, K:K + 1] * np.zeros((1, c1 - c0))
        parts.append(acc)
    z = np.zeros((M, N))
    for acc in parts[1 if defect == "chunk0_dropped" else 0:]:
        z += acc
    z = z + bias
    buf, view = xo.sentinel_output(M, N, ldc, False, "cpu")
    view.copy_(torch.from_numpy(z))
    if defect == "column_past_n":
        off = (view.data_ptr() - buf.data_ptr()) // 8 - ldc
        buf[1:M + 1, off + N] = view[:, N - 1]
    return buf, view


def padded(a, pad, fill):
    out = np.full((a.shape[0], a.shape[1] + pad), fill)
    out[:, :a.shape[1]] = a
    return out


CASES = [(70, 130, 258, 144), (70, 130, 100, None), (37, 53, 29, None), (60, 96, 4096, 144)]


@pytest.mark.parametrize("m,n,k,kchunk", CASES)
def test_emulation_without_a_defect_is_exact(m, n, k, kchunk):
    a, b, bias = xo.draw(np.random.RandomState(k), m, n, k)
    buf, view = emulate(padded(a, 3, np.nan), b, bias, k, n + 3, kchunk)
    assert np.array_equal(view.numpy(), xo.product(a, b, bias)) and xo.guard_intact(buf, view)


@pytest.mark.parametrize("m,n,k,kchunk", CASES)
@pytest.mark.parametrize("defect", ["drop_last_k", "pad_k", "chunk0_dropped", "column_past_n"])
def test_each_modelled_defect_is_seen(m, n, k, kchunk, defect):
    if defect == "chunk0_dropped" and kchunk is None:
        kchunk = 16                                                   # (a split of the one-pass cases, for this defect)
    a, b, bias = xo.draw(np.random.RandomState(k), m, n, k)
    z = xo.product(a, b, bias)
    buf, view = emulate(padded(a, 3, np.nan), b, bias, k, n + 3, kchunk, defect)
    same, guard = np.array_equal(view.numpy(), z), xo.guard_intact(buf, view)
    if defect == "column_past_n":
        assert same and not guard                                     # only the band shows it
    elif defect == "pad_k":
        assert not same and not guard and np.isnan(view.numpy()[16:32, 16:32]).all()
        # the same defect behind a ZERO pad column -- what the suite had -- changes nothing: 0 * 0
        buf0, view0 = emulate(padded(a, 3, 0.0), b, bias, k, n + 3, kchunk, defect)
        assert np.array_equal(view0.numpy(), z) and xo.guard_intact(buf0, view0)
    else:
        assert not same and guard
        wrong = view.numpy() != z
        if defect == "drop_last_k":                                   # confined to the block, and integers: far above any rounding
            assert wrong[16:32, 16:32].any() and not wrong[:16].any() and not wrong[:, :16].any()
            assert np.abs(view.numpy() - z)[wrong].min() >= 2.0 ** -24
        else:
            assert wrong.mean() > 0.9


def test_guard_bands():
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    for ld, mis in ((4, False), (6, False), (6, True), (7, False), (7, True), (5, True)):
        buf, view = xo.banded(x, ld, mis)
        assert buf.shape == (5, ld) and torch.equal(view, x)
        off = (view.data_ptr() - buf.data_ptr()) // 8 - ld
        assert off in (0, 1) and (ld + off) % 2 == int(mis)
        inside = torch.zeros_like(buf, dtype=torch.bool)
        inside[1:4, off:off + 4] = True
        assert torch.isnan(buf[~inside]).all() and not torch.isnan(buf[inside]).any()
    with pytest.raises(ValueError):
        xo.banded(x, 4, True)                                         # no room for the column offset
    vb, v = xo.banded_vector(x[0])
    assert torch.equal(v, x[0]) and torch.isnan(vb[0]) and torch.isnan(vb[-1])
    for ld, mis in ((4, False), (7, True), (6, True)):
        buf, view = xo.sentinel_output(3, 4, ld, mis, "cpu")
        assert not xo.guard_intact(buf, view)                         # unwritten: the sentinel is a NaN
        view.copy_(x)
        assert xo.guard_intact(buf, view)
        for r, c in ((0, 0), (4, ld - 1), (1, ld - 1) if ld > 4 else (0, 1)):
            was = buf[r, c].clone()
            buf[r, c] = 1.0
            inside_view = 1 <= r <= 3 and (view.data_ptr() - buf.data_ptr()) // 8 - ld <= c < (view.data_ptr() - buf.data_ptr()) // 8 - ld + 4
            assert xo.guard_intact(buf, view) == inside_view
            buf.view(torch.int64)[r, c] = was.view(torch.int64)
        assert xo.guard_intact(buf, view)
        view[1, 1] = float("nan")
        assert not xo.guard_intact(buf, view)
