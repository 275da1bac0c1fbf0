"""The reduced-precision routes element by element against fp64, within the bounds of tests/precision_bounds.py.

  * f16x2: dlc_sdav_encode_split (SDAV(dtype="f16x2")) -- single layers at the tile and slice edges, slice probes
    (rows non-zero in one 32-deep k-slice: the case that catches a stale ring slot or a product dropped in one slice),
    chains with the bound propagated layer by layer, and the input contract of include/dlc.h;
  * fp32: gemm_bias_act on every plan (one pass, split-K under latency_mode, both B layouts, every activation, bias or
    none, leading dimensions of A, B and C wider than the row), dlc_bias_act in fp32 and fp64, and their callers SDAV(dtype="float32")
    and TensorWrapper.
Every case prints its worst err / bound and asserts it is <= 1.  The bounds are derived, not fitted
(tests/test_precision_bounds_cpu.py shows they hold for an emulation and break for each modelled defect)."""
import numpy as np
import pytest
import torch

import precision_bounds as pb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def eng(dlc):
    return dlc.default_engine()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def report(what, r):
    print("%-70s worst err/bound %.3g" % (what, r))
    assert r <= 1.0, (what, r)
    return r


# --------------------------------------------------------------------------------------------------- f16x2 helpers
def weights(kind, K, N, rng):
    if kind == "fan_in":
        return rng.standard_normal((K, N)) / np.sqrt(K)
    if kind == "normal":
        return rng.standard_normal((K, N))
    if kind == "outlier":                  # second pieces of most weights are fp16 subnormals
        w = 1e-2 * rng.standard_normal((K, N))
        w[K // 2, N // 2] = 1e3
        return w
    if kind in ("max_one", "below_one"):   # the two sides of sp_scale_kernel's frexp boundary
        w = rng.uniform(-1, 1, (K, N)) * 0.999
        w[K // 3, N // 3] = 1.0 if kind == "max_one" else np.nextafter(1.0, 0.0)
        return w
    if kind == "zero":
        return np.zeros((K, N))
    raise ValueError(kind)


def inputs(kind, M, K, rng):
    if kind == "uniform":
        return rng.uniform(0, 1, (M, K))
    if kind == "tiny":                     # saturated-sigmoid magnitudes: first pieces are fp16 subnormals
        return 10.0 ** rng.uniform(-9, -6, (M, K))
    if kind == "zeros":
        x = rng.uniform(0, 1, (M, K))
        x[:, ::3] = 0.0
        x[::2, K // 2:] = 0.0
        x[0] = 0.0
        return x
    if kind == "edge":                     # +-16, the documented edge of the input range
        return rng.choice([-16.0, 16.0, 0.25], size=(M, K))
    raise ValueError(kind)


def split_encode(eng, x, ws, bs):
    dims = [x.shape[1]] + [w.shape[1] for w in ws]
    return eng.sdav_encode_split(x, dims, eng.sdav_split_panels(ws), bs)


def chain_ratio(eng, x, ws, bs):
    """Encode, then compare every element with the fp64 chain within the propagated bound; returns (ratio, output)."""
    got = split_encode(eng, x, ws, bs)
    (h, e), = pb.split_chain_bound(x, ws, bs)[-1:]
    return pb.ratio(got - h, e), got


# --------------------------------------------------------------------------------------------------- a. full rows
KS = [1, 31, 32, 33, 64, 65, 96, 97, 1681, 2500, 4096]
NS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2500]
ROWS = [1, 255, 256, 257, 1280, 31890]
WKINDS = ["fan_in", "normal", "outlier", "max_one", "below_one", "zero"]
XKINDS = ["uniform", "tiny", "zeros", "edge"]
# Every K, N, row count, weight and input kind appears; K and N walk their lists at co-prime strides so that each
# K meets several N.  31 890 rows (the reference's 1063 frames) only with N <= 257.
FULL_CASES = []
for i in range(22):
    K, N, rows = KS[i % 11], NS[(3 * i + 1) % 11], ROWS[i % 6]
    if rows == 31890 and N > 257:
        rows = 1280
    FULL_CASES.append((K, N, rows, WKINDS[i % 6], XKINDS[(i // 2) % 4], i % 2 == 0))
FULL_CASES += [(2500, 2500, 1280, "normal", "uniform", True), (4096, 257, 31890, "fan_in", "uniform", False),
               (1681, 2500, 257, "outlier", "tiny", True), (2500, 65, 31890, "below_one", "edge", True)]


@pytest.mark.parametrize("K,N,rows,wkind,xkind,bias", FULL_CASES)
def test_split_layer_full_rows_elementwise(eng, K, N, rows, wkind, xkind, bias):
    rng = np.random.RandomState(K * 31 + N * 7 + rows)
    x, w = dev(inputs(xkind, rows, K, rng)), dev(weights(wkind, K, N, rng))
    b = dev(0.3 * rng.standard_normal(N)) if bias else None
    r, got = chain_ratio(eng, x, [w], [b])
    if wkind == "zero":                    # W = 0: acc = 0 exactly, every row is sigma(b) from the fp32 epilogue alone
        assert torch.equal(got, got[:1].expand_as(got))
    report("split layer K %d N %d rows %d, %s weights, %s inputs, bias %s" % (K, N, rows, wkind, xkind, bias), r)


# --------------------------------------------------------------------------------------------------- b. slice probes
@pytest.mark.parametrize("K", [97, 1681, 2500])
@pytest.mark.parametrize("N", [257, 2500])
@pytest.mark.parametrize("wkind", ["fan_in", "normal"])
def test_split_layer_slice_probes(eng, K, N, wkind):
    """Rows non-zero in one k-slice (every slice, the tail included, at four row positions in two 256-row tiles): the
    bound counts that slice's three steps only, so a stale W2 / h2 slot or a product dropped in one slice exceeds it
    30-340x in the emulation (tests/test_precision_bounds_cpu.py)."""
    rng = np.random.RandomState(K + 3 * N)
    x = dev(pb.slice_probes(K, rng))
    w, b = dev(weights(wkind, K, N, rng)), dev(0.1 * rng.standard_normal(N))
    r, _ = chain_ratio(eng, x, [w], [b])
    report("split probes K %d N %d, %s weights" % (K, N, wkind), r)


# --------------------------------------------------------------------------------------------------- c. chains
CHAINS = [([1681] + [2500] * 5, "fan_in", 300), ([1681] + [2500] * 5, "normal", 300),
          ([1681, 2500, 2500, 2500, 2500, 4096], "fan_in", 257),
          ([97, 257, 65, 17, 300, 33], "fan_in", 513), ([97, 257, 65, 17, 300, 33], "normal", 513)]


@pytest.mark.parametrize("dims,wkind,rows", CHAINS)
def test_split_chain_elementwise(eng, dims, wkind, rows):
    """Hidden layers hand on fp16 pieces of the fp32 output; the ragged chain's widths end inside 16-, 64- and
    256-column blocks, so layer l's N tail is layer l+1's K tail.  Each row encoded alone equals its row in the batch."""
    rng = np.random.RandomState(len(dims) * 100 + rows)
    ws = [dev(weights(wkind, k, n, rng)) for k, n in zip(dims[:-1], dims[1:])]
    bs = [dev(0.1 * rng.standard_normal(n)) if l % 2 == 0 else None for l, n in enumerate(dims[1:])]
    x = dev(rng.uniform(0, 1, (rows, dims[0])))
    r, got = chain_ratio(eng, x, ws, bs)
    for i in (0, 17, rows // 2, rows - 1):
        assert torch.equal(split_encode(eng, x[i:i + 1], ws, bs)[0], got[i]), i
    report("split chain %s, %s weights, %d rows" % (dims, wkind, rows), r)


# --------------------------------------------------------------------------------------------------- d. input contract
def test_split_input_contract(eng):
    """include/dlc.h: x must lie in [-16, 16].  A row holding 40, 1e4, +inf or NaN (x 2^11 overflows fp16) is NaN in
    every output; every other row is bit for bit what it is in the batch without that row."""
    rng = np.random.RandomState(4)
    dims = [97, 300, 65]
    ws = [dev(weights("fan_in", k, n, rng)) for k, n in zip(dims[:-1], dims[1:])]
    bs = [dev(0.1 * rng.standard_normal(n)) for n in dims[1:]]
    x = rng.uniform(0, 1, (40, dims[0]))
    x[1, 5] = 16.0
    x[2, 90] = -16.0
    bad = {3: 40.0, 9: 1e4, 22: np.inf, 31: np.nan}
    for r_, v in bad.items():
        x[r_, (7 * r_) % dims[0]] = v
    got = split_encode(eng, dev(x), ws, bs)
    rows_ok = [r_ for r_ in range(40) if r_ not in bad]
    clean = split_encode(eng, dev(x[rows_ok]), ws, bs)
    for r_ in bad:
        assert torch.isnan(got[r_]).all(), r_
    assert torch.equal(got[rows_ok], clean)
    assert torch.isfinite(clean).all()


# --------------------------------------------------------------------------------------------------- f. fp32 gemm
GEMM_SHAPES = [(37, 53, 29), (128, 128, 16), (600, 2500, 1681), (1, 1, 1), (130, 384, 3456),
               (300, 2500, 2500), (300, 1681, 2500), (300, 2501, 2500), (77, 130, 4096), (200, 256, 8190),
               (1, 2500, 2502), (255, 1000, 644), (64, 128, 130), (320, 1024, 1682), (129, 98, 5000),
               (30, 2500, 2497), (60, 300, 1695), (7, 33, 17), (3, 5, 31)]   # K % 16 = 1 and 15


def _act_ref(act, z):
    return torch.sigmoid(z) if act == 1 else (torch.relu(z) if act == 2 else z)


@pytest.mark.parametrize("blayout", [0, 1])
def test_gemm_bias_act_f32_every_plan(eng, blayout):
    from deeploopcloser_amd import _lib as L
    worst, split_differs = 0.0, False
    for m, n, k in GEMM_SHAPES:
        rng = np.random.RandomState(m * 3 + n + k)
        a = rng.standard_normal((m, k)).astype(np.float32)
        b = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
        bias = rng.standard_normal(n).astype(np.float32)
        a64, b64, bias64 = dev(a), dev(b), dev(bias)
        ta, tbias = dev(a, torch.float32), dev(bias, torch.float32)
        tb = dev(b if blayout == 0 else b.T, torch.float32)
        abs_ab = a64.abs() @ b64.abs()
        for with_bias in (True, False):
            z = a64 @ b64 + (bias64 if with_bias else 0.0)
            for act in (L.DLC_ACT_NONE, L.DLC_ACT_SIGMOID, L.DLC_ACT_RELU):
                ref = _act_ref(act, z)
                tbb = tbias if with_bias else None
                one = eng.gemm_bias_act(ta, tb, tbb, act=act, blayout=blayout)
                bound1 = pb.act_bound(act, z, pb.gemm_dz(abs_ab, k, 1, bias64 if with_bias else None))
                worst = max(worst, pb.ratio(one.double() - ref, bound1))
                with eng.latency_mode():
                    split = eng.gemm_bias_act(ta, tb, tbb, act=act, blayout=blayout)
                    again = eng.gemm_bias_act(ta, tb, tbb, act=act, blayout=blayout)
                assert torch.equal(split, again), (m, n, k, act)
                split_differs |= not torch.equal(split, one)
                bound = pb.act_bound(act, z, pb.gemm_dz(abs_ab, k, pb.latency_chunks_max(k), bias64 if with_bias else None))
                worst = max(worst, pb.ratio(split.double() - ref, bound))
                assert worst <= 1.0, (m, n, k, act, with_bias, worst)
    assert split_differs                     # the split plan ran (its summation order is not the one-pass order)
    report("fp32 gemm_bias_act, %s, every shape / act / bias / plan" % ("KN" if blayout == 0 else "NK"), worst)


@pytest.mark.parametrize("m,n,k,blayout", [(300, 2500, 2500, 0), (37, 53, 29, 1), (60, 300, 1695, 1), (129, 98, 5000, 0)])
def test_gemm_bias_act_f32_wide_leading_dimensions(eng, m, n, k, blayout):
    """lda > K, ldb > B's row width and ldc > N through the C ABI: A's and B's padding is NaN (never read), C's padding a
    sentinel (never written).  B both tight and wide, in the layout of the case."""
    from deeploopcloser_amd import _lib as L
    rng = np.random.RandomState(m + n + k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    lda, ldc = k + 5, n + 3
    wide = torch.full((m, lda), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :k] = dev(a, torch.float32)
    tight_b = dev(b if blayout == 0 else b.T, torch.float32)
    wide_b = torch.full((tight_b.shape[0], tight_b.shape[1] + 7), float("nan"), dtype=torch.float32, device="cuda")
    wide_b[:, :tight_b.shape[1]] = tight_b
    tbias = dev(bias, torch.float32)
    z = dev(a) @ dev(b) + dev(bias)
    for tb in (tight_b, wide_b):
        assert tb.stride(0) == tight_b.shape[1] + (7 if tb is wide_b else 0)
        for scratch in (False, True):
            for act in (L.DLC_ACT_NONE, L.DLC_ACT_SIGMOID, L.DLC_ACT_RELU):
                out = torch.full((m, ldc), 12345.0, dtype=torch.float32, device="cuda")
                if scratch:
                    eng.set_scratch()
                try:
                    eng._check(eng.lib.dlc_gemm_bias_act(eng.ctx, L.DLC_F32, blayout, act, m, n, k, wide.data_ptr(), lda,
                                                          tb.data_ptr(), tb.stride(0), tbias.data_ptr(), out.data_ptr(), ldc, None))
                    torch.cuda.synchronize()
                finally:
                    if scratch:
                        eng.set_scratch(0)
                assert torch.all(out[:, n:] == 12345.0)
                bound = pb.act_bound(act, z, pb.gemm_dz(dev(a).abs() @ dev(b).abs(), k, pb.latency_chunks_max(k) if scratch else 1, dev(bias)))
                report("fp32 gemm lda %d ldb %d ldc %d, %dx%dx%d, act %d, latency %s" % (lda, tb.stride(0), ldc, m, n, k, act, scratch),
                       pb.ratio(out[:, :n].double() - _act_ref(act, z), bound))


# --------------------------------------------------------------------------------------------------- g. bias_act
def _ulps(got, ref, dt):
    """|got - ref| in units of the spacing of `dt` at ref."""
    return np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(dt)).astype(np.float64)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_bias_act_every_activation(eng, dtype):
    """dlc_bias_act with and without bias, one row, one column, M N past one grid pass of 8192 x 256 threads, strided
    lda / ldc with sentinels in the padding.  fp64 within 2 ulp of NumPy (none / relu: the same bits).  fp32: none and
    relu are the fp32 sum itself; sigmoid is within (1 - s)(|z| + 4) + 2 ulp of the fp64 formula on the fp32 inputs --
    (1 - s)|z| from rounding a + b (relative u |z| on z, times d log s / dz = 1 - s), 4 (1 - s) from expf's 2 ulp, 2 from
    the add and the division."""
    from deeploopcloser_amd import _lib as L
    from oracle import tensor_ops
    npdt, tdt, code = (np.float32, torch.float32, L.DLC_F32) if dtype == "f32" else (np.float64, torch.float64, L.DLC_F64)
    worst = 0.0
    for m, n, pad_a, pad_c in ((1, 300, 0, 0), (300, 1, 0, 0), (1500, 1501, 0, 0), (77, 130, 5, 3), (1, 1, 2, 1)):
        rng = np.random.RandomState(m + n)
        a = (3 * rng.standard_normal((m, n))).astype(npdt)
        bias = rng.standard_normal(n).astype(npdt)
        ta = torch.full((m, n + pad_a), float("nan"), dtype=tdt, device="cuda")
        ta[:, :n] = dev(a, tdt)
        tbias = dev(bias, tdt)
        for with_bias in (True, False):
            for act in (L.DLC_ACT_NONE, L.DLC_ACT_SIGMOID, L.DLC_ACT_RELU):
                out = torch.full((m, n + pad_c), -777.0, dtype=tdt, device="cuda")
                eng._check(eng.lib.dlc_bias_act(eng.ctx, code, act, m, n, ta.data_ptr(), ta.stride(0),
                                                 tbias.data_ptr() if with_bias else None, out.data_ptr(), out.stride(0), None))
                torch.cuda.synchronize()
                assert torch.all(out[:, n:] == -777.0)
                got = out[:, :n].cpu().numpy()
                zt = (a + bias) if with_bias else a                               # in the operand type: one rounding
                if act != L.DLC_ACT_SIGMOID:
                    assert np.array_equal(got, np.maximum(zt, 0) if act == L.DLC_ACT_RELU else zt), (m, n, act)
                    continue
                if dtype == "f64":
                    u = _ulps(got, tensor_ops.sigmoid(zt), np.float64)
                    assert u.max() <= 2.0, (m, n, u.max())
                    worst = max(worst, u.max() / 2.0)
                else:
                    z64 = a.astype(np.float64) + (bias.astype(np.float64) if with_bias else 0.0)
                    ref = tensor_ops.sigmoid(z64)
                    allow = (1 - ref) * (np.abs(z64) + 4) + 2
                    worst = max(worst, float((_ulps(got, ref, np.float32) / allow).max()))
                assert worst <= 1.0, (dtype, m, n, with_bias, worst)
    report("bias_act %s, sigmoid in ulps against the stated allowance" % dtype, worst)


# --------------------------------------------------------------------------------------------------- h. callers
@pytest.mark.parametrize("hu,frames,latency", [([300, 77, 1000], 4, False), ([2500] * 5, 1, True),
                                               ([2500, 2500, 2500, 2500, 4096], 2, False), ([300, 77, 1000], 1, True)])
def test_sdav_float32_elementwise(dlc, hu, frames, latency):
    """SDAV(dtype="float32") against oracle.sdav.transform on the fp32 operands, every element within the propagated
    bound; under latency_mode a frame's 30 rows take split-K (the chunk count bounded by plan_split's cap)."""
    from oracle import sdav as osdav
    rng = np.random.RandomState(len(hu) + frames)
    net = dlc.SDAV(seed=12, dtype="float32", weight_scale="fan_in", hidden_units=hu)
    ws, bs = net.get_weights()
    bs = [(0.1 * rng.standard_normal(b.shape)).astype(np.float32) for b in bs]
    net.set_weights(ws, bs)
    x = rng.uniform(0, 1, size=(frames, 30, 1681)).astype(np.float32).astype(np.float64)
    if latency:
        with net.engine.latency_mode():
            h = net.transform(x)
    else:
        h = net.transform(x)
    ws64 = [w.astype(np.float64) for w in ws]
    bs64 = [b.astype(np.float64) for b in bs]
    ref = osdav.transform(x, ws64, bs64)
    chunks = pb.latency_chunks_max if latency else (lambda K: 1)
    (h_ref, e), = pb.f32_chain_bound(dev(x.reshape(-1, 1681)), [dev(w) for w in ws64], [dev(b) for b in bs64], chunks)[-1:]
    assert np.abs(h_ref.cpu().numpy() - ref).max() < 1e-12          # the bound's chain is the oracle's
    report("SDAV float32 %s, %d frame(s), latency %s" % (hu, frames, latency), pb.ratio(dev(h) - dev(ref), e))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("rank3", [False, True])
def test_tensor_wrapper_matmul_add_sigmoid(dlc, dtype, rank3):
    """TensorWrapper x.matmul(w).add(b).sigmoid(): fused (one gemm_bias_act) and unfused (the product materialised
    first, then add and sigmoid through dlc_bias_act), 2-D and the 3-D x 2-D broadcast, against oracle.tensor_ops."""
    from deeploopcloser_amd.tensor_wrapper import TensorWrapper
    from oracle import tensor_ops
    fp64 = dtype == torch.float64
    npdt = np.float64 if fp64 else np.float32
    rng = np.random.RandomState(31 + rank3)
    shape = (3, 30, 401) if rank3 else (67, 401)
    x = rng.uniform(0, 1, shape).astype(npdt)
    w = (rng.standard_normal((401, 130)) / 20).astype(npdt)
    b = rng.standard_normal(130).astype(npdt)
    tx, tw, tb = dev(x, dtype), dev(w, dtype), dev(b, dtype)
    fused = TensorWrapper(tx).matmul(tw).add(tb).sigmoid().numpy()
    prod = TensorWrapper(tx).matmul(tw)
    prod.to_tf()                                                        # materialised: add and sigmoid are bias_act
    unfused = prod.add(tb).sigmoid().numpy()
    x64, w64, b64 = (v.astype(np.float64) for v in (x, w, b))
    ref = tensor_ops.sigmoid(tensor_ops.tw_matmul(x64, w64) + b64)
    z = dev(tensor_ops.tw_matmul(x64, w64) + b64).reshape(-1, 130)
    abs_ab = dev(np.abs(x64).reshape(-1, 401)) @ dev(np.abs(w64))
    u = pb.U64 if fp64 else pb.U
    for name, got, extra in (("fused", fused, 0), ("unfused", unfused, 1)):
        assert got.shape == ref.shape and got.dtype == npdt
        bound = pb.act_bound(1, z, pb.gemm_dz(abs_ab, 401 + extra, 1, dev(b64), u=u), fp64=fp64)
        report("TensorWrapper %s %s %s" % (name, "3-D" if rank3 else "2-D", dtype), pb.ratio(dev(got.reshape(-1, 130)) - dev(ref.reshape(-1, 130)), bound))
