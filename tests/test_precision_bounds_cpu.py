"""The bounds of tests/precision_bounds.py have teeth: a NumPy emulation of the kernels' arithmetic stays inside them, and
every defect of the kind these kernels tend to have breaks them on at least one element.  CPU only.

The split-layer emulation follows csrc/gemm_split_f16.hip step by step: fp16 pieces of x 2^11 and W 2^s, per 32-deep
k-slice the three products P1 = h1.W1, P2 = h2.W1, P3 = h1.W2 each added to an fp32 accumulator with one rounding, then
the fp32 epilogue (one fma, exp2, reciprocal) and, for a hidden layer, the fp16 pieces of the fp32 output.  The fp32
emulation is the k-ordered fmaf chain of v_mfma_f32_16x16x4_f32, split-K partials summed in fp32 chunk by chunk, the bias
added once, sigmoid as 1 / (1 + expf(-z)).  The GPU tests (tests/test_gpu_reduced_precision.py) hold the kernels
themselves to the same bounds."""
import numpy as np
import pytest
import torch

import precision_bounds as pb

T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
F32, F16 = np.float32, np.float16


# --------------------------------------------------------------------------------------------------- emulation
def _pieces(v, wide):
    """Two fp16 pieces of v (v - piece 1 computed exactly in `wide`)."""
    a = v.astype(F16)
    return a, (v - a.astype(wide)).astype(F16)


def emulate_split_layer(xs, w, b, final, mutant=None, j0=None):
    """One layer of dlc_sdav_encode_split.  xs: the layer's scaled input, x 2^11 (fp64 for layer 0, the previous layer's
    fp32 output otherwise).  Returns the fp64 output (final) or the fp32 h 2^11 (hidden).

    mutant: None (faithful), "p2_drop" (P2 skipped in slice j0), "p3_drop_tail" (P3 skipped in the tail slice),
    "stale_w2" (slice j0 uses W2 of slice j0 - 2), "h2_tail_zero" (h2 of the tail slice read as zeros)."""
    K, N = w.shape
    s = pb.split_scale_exponent(T(w))
    x1, x2 = _pieces(xs, np.float64 if xs.dtype == np.float64 else F32)
    w1, w2 = _pieces(w * 2.0 ** s, np.float64)
    ns = (K + 31) // 32
    acc = np.zeros((xs.shape[0], N), dtype=F32)
    step = lambda acc, p: (acc.astype(np.float64) + p).astype(F32)       # 32 exact products + acc, one rounding
    for j in range(ns):
        ks = slice(32 * j, min(K, 32 * (j + 1)))
        a1, a2 = x1[:, ks].astype(np.float64), x2[:, ks].astype(np.float64)
        b1, b2 = w1[ks].astype(np.float64), w2[ks].astype(np.float64)
        if mutant == "stale_w2" and j == j0:
            b2 = w2[32 * (j - 2):32 * (j - 1)].astype(np.float64)
        if mutant == "h2_tail_zero" and j == ns - 1:
            a2 = np.zeros_like(a2)
        acc = step(acc, a1 @ b1)
        if not (mutant == "p2_drop" and j == j0):
            acc = step(acc, a2 @ b1)
        if not (mutant == "p3_drop_tail" and j == ns - 1):
            acc = step(acc, a1 @ b2)
    ninv = F32(-F32(pb.LOG2E) / F32(2.0 ** (pb.SP_X_SHIFT + s)))
    bias = np.zeros(N) if b is None else b
    bv = (-pb.LOG2E * bias - (0.0 if final else pb.SP_X_SHIFT)).astype(F32)
    zl = (acc.astype(np.float64) * np.float64(ninv) + bv).astype(F32)
    with np.errstate(over="ignore"):
        e = np.exp2(zl)
    one = F32(1.0 if final else 2.0 ** -pb.SP_X_SHIFT)
    hv = F32(1.0) / (one + e)
    return hv.astype(np.float64) if final else hv


def emulate_split_chain(x, ws, bs, mutant=None, layer=None, j0=None):
    h = x * 2.0 ** pb.SP_X_SHIFT
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = emulate_split_layer(h, w, b, l == len(ws) - 1, mutant if l == layer else None, j0)
    return h


def emulate_gemm_f32(a, b, bias, chunks, act, mutant=None):
    """gemm_bias_act in fp32: a [M,K], b [K,N] fp32.  mutant: "bias_every_chunk", "chunk_twice"."""
    M, K = a.shape
    kchunk = -(-K // chunks)
    parts = []
    for c in range(chunks):
        acc = np.zeros((M, b.shape[1]), dtype=F32)
        for k in range(c * kchunk, min(K, (c + 1) * kchunk)):
            acc = (acc.astype(np.float64) + np.outer(a[:, k], b[k]).astype(np.float64)).astype(F32)
        if mutant == "bias_every_chunk" and bias is not None and c < chunks - 1:
            acc = acc + bias
        parts.append(acc)
    if mutant == "chunk_twice":
        parts.insert(1, parts[1])
    z = parts[0]
    for p in parts[1:]:
        z = z + p
    if bias is not None:
        z = z + bias
    if act == 1:
        with np.errstate(over="ignore"):
            return F32(1.0) / (F32(1.0) + np.exp(-z))
    return np.maximum(z, F32(0)) if act == 2 else z


# --------------------------------------------------------------------------------------------------- helpers
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
        w[0, 0] = 1.0 if kind == "max_one" else np.nextafter(1.0, 0.0)
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
        x[0] = 0.0
        return x
    if kind == "edge":                     # +-16, the documented input range
        return rng.choice([-16.0, 16.0, 0.5], size=(M, K))
    raise ValueError(kind)


def layer_ratio(x, w, b, got):
    z = T(x) @ T(w) + (0.0 if b is None else T(b))
    bound, _ = pb.split_layer_bound(T(x), torch.zeros(x.shape, dtype=torch.float64), T(w), None if b is None else T(b),
                                    z, final=True)
    return pb.ratio(T(got) - torch.sigmoid(z), bound)


# --------------------------------------------------------------------------------------------------- split layer
@pytest.mark.parametrize("wkind", ["fan_in", "normal", "outlier", "max_one", "below_one", "zero"])
@pytest.mark.parametrize("xkind", ["uniform", "tiny", "zeros", "edge"])
def test_split_emulation_within_bound_full_rows(wkind, xkind):
    rng = np.random.RandomState(len(wkind) * 7 + len(xkind))
    for M, K, N, bias in ((40, 97, 65, True), (17, 1681, 257, False)):
        x, w = inputs(xkind, M, K, rng), weights(wkind, K, N, rng)
        b = 0.3 * rng.standard_normal(N) if bias else None
        got = emulate_split_layer(x * 2.0 ** pb.SP_X_SHIFT, w, b, True)
        r = layer_ratio(x, w, b, got)
        assert r <= 1.0, (wkind, xkind, M, K, N, r)


@pytest.mark.parametrize("K,N", [(97, 2500), (1681, 257), (2500, 257)])
@pytest.mark.parametrize("wkind", ["fan_in", "normal"])
def test_split_probes_faithful_within_and_mutants_beyond(K, N, wkind):
    """On slice probes the faithful emulation is well inside the bound, and each of the four one-slice defects
    exceeds it on at least one element."""
    rng = np.random.RandomState(K + N)
    x = pb.slice_probes(K, rng)
    w = weights(wkind, K, N, rng)
    b = 0.1 * rng.standard_normal(N)
    ns = (K + 31) // 32
    j0 = ns // 2 if ns > 2 else 2
    faithful = layer_ratio(x, w, b, emulate_split_layer(x * 2.0 ** pb.SP_X_SHIFT, w, b, True))
    line = ["faithful %.3g" % faithful]
    assert faithful <= 1.0
    for mutant in ("p2_drop", "p3_drop_tail", "stale_w2", "h2_tail_zero"):
        if mutant == "stale_w2" and ns < 3:
            continue
        r = layer_ratio(x, w, b, emulate_split_layer(x * 2.0 ** pb.SP_X_SHIFT, w, b, True, mutant, j0))
        line.append("%s %.3g" % (mutant, r))
        assert r > 1.0, (mutant, r)
    print("K %d N %d %s weights: err / bound %s" % (K, N, wkind, ", ".join(line)))


def test_split_all_zero_layer_is_sigmoid_of_bias():
    rng = np.random.RandomState(3)
    x, b = rng.uniform(0, 1, (5, 70)), 3 * rng.standard_normal(33)
    got = emulate_split_layer(x * 2.0 ** pb.SP_X_SHIFT, np.zeros((70, 33)), b, True)
    assert np.all(got == got[0]) and layer_ratio(x, np.zeros((70, 33)), b, got) <= 1.0


@pytest.mark.parametrize("scale", ["fan_in", "normal"])
def test_split_chain_emulation_within_propagated_bound(scale):
    """The reference chain 1681 -> 2500 x 5 and a ragged chain whose widths end inside 16-, 64- and 256-column
    blocks: the emulated hidden layers (fp32 output -> fp16 pieces) within the propagated bound at every layer."""
    rng = np.random.RandomState(11)
    for dims, M in (([1681] + [2500] * 5, 6), ([97, 257, 65, 17, 300], 33)):
        ws = [weights(scale, k, n, rng) for k, n in zip(dims[:-1], dims[1:])]
        bs = [0.1 * rng.standard_normal(n) for n in dims[1:]]
        x = rng.uniform(0, 1, (M, dims[0]))
        got = emulate_split_chain(x, ws, bs)
        (h, e), = pb.split_chain_bound(T(x), [T(w) for w in ws], [T(b) for b in bs])[-1:]
        r = pb.ratio(T(got) - h, e)
        print("chain %s, %s weights: err / bound %.3g" % (dims, scale, r))
        assert r <= 1.0


def test_split_chain_mutant_in_a_hidden_layer_trips():
    """A one-slice defect in a hidden layer of a chain still shows at the chain's output (probe rows, 1/sqrt(K))."""
    rng = np.random.RandomState(12)
    dims = [97, 257, 129]
    ws = [weights("fan_in", k, n, rng) for k, n in zip(dims[:-1], dims[1:])]
    bs = [None, None]
    x = pb.slice_probes(dims[0], rng)
    (h, e), = pb.split_chain_bound(T(x), [T(w) for w in ws], bs)[-1:]
    assert pb.ratio(T(emulate_split_chain(x, ws, bs)) - h, e) <= 1.0
    assert pb.ratio(T(emulate_split_chain(x, ws, bs, "p2_drop", 0, 1)) - h, e) > 1.0


# --------------------------------------------------------------------------------------------------- fp32 route
@pytest.mark.parametrize("act", [0, 1, 2])
def test_f32_gemm_emulation_within_bound_and_split_mutants_beyond(act):
    rng = np.random.RandomState(act)
    M, K, N, chunks = 30, 401, 90, 4
    a = rng.standard_normal((M, K)).astype(F32)
    b = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(F32)
    bias = rng.standard_normal(N).astype(F32)
    a64, b64, bias64 = T(a), T(b), T(bias)
    z = a64 @ b64 + bias64
    ref = torch.sigmoid(z) if act == 1 else (torch.relu(z) if act == 2 else z)
    for c in (1, chunks):
        bound = pb.act_bound(act, z, pb.gemm_dz(a64.abs() @ b64.abs(), K, c, bias64))
        assert pb.ratio(T(emulate_gemm_f32(a, b, bias, c, act)) - ref, bound) <= 0.5
    bound = pb.act_bound(act, z, pb.gemm_dz(a64.abs() @ b64.abs(), K, chunks, bias64))
    for mutant in ("bias_every_chunk", "chunk_twice"):
        r = pb.ratio(T(emulate_gemm_f32(a, b, bias, chunks, act, mutant)) - ref, bound)
        assert r > 1.0, (mutant, r)


def test_f32_chain_emulation_within_propagated_bound():
    rng = np.random.RandomState(5)
    dims = [1681, 300, 77, 257]
    x = rng.uniform(0, 1, (30, dims[0])).astype(F32)
    for scale in ("fan_in", "normal"):
        ws = [weights(scale, k, n, rng).astype(F32) for k, n in zip(dims[:-1], dims[1:])]
        bs = [(0.1 * rng.standard_normal(n)).astype(F32) for n in dims[1:]]
        for chunks in (1, 5):
            h = x
            for w, b in zip(ws, bs):
                h = emulate_gemm_f32(h, w, b, chunks if w.shape[0] > 256 else 1, 1)
            (ref, e), = pb.f32_chain_bound(T(x), [T(w) for w in ws], [T(b) for b in bs],
                                            chunks=lambda K: chunks if K > 256 else 1)[-1:]
            assert pb.ratio(T(h) - ref, e) <= 1.0, (scale, chunks)


def test_bounds_are_not_vacuous():
    """The bounds are far below the quantities they guard: a 1/sqrt(K) split layer's bound is ~1e-6 or less, not the
    1e-4 of the row-L2 tests, and sigmoid's slope is taken where the output sits, not the global 1/4."""
    rng = np.random.RandomState(9)
    x, w = rng.uniform(0, 1, (8, 2500)), weights("fan_in", 2500, 2500, rng)
    z = T(x) @ T(w)
    bound, dz = pb.split_layer_bound(T(x), torch.zeros(8, 2500, dtype=torch.float64), T(w), None, z, final=True)
    assert float(bound.max()) < 2e-5
    zs = torch.tensor([0.0, 10.0, 40.0], dtype=torch.float64)
    out = pb.sigmoid_out_bound(zs, torch.full_like(zs, 1e-3), 0.0, 0.0)
    assert float(out[0]) < 2.6e-4 and float(out[1]) < 5e-8 and float(out[2]) < 1e-19
