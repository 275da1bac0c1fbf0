"""Elementwise error bounds for the two reduced-precision routes, derived from the arithmetic the kernels perform.

Shared by tests/test_precision_bounds_cpu.py (which shows that the bounds hold for a NumPy emulation of the kernels and
that each modelled defect breaks them) and tests/test_gpu_reduced_precision.py (which holds the HIP kernels to them).
Nothing here is fitted to a measurement: every constant is a unit roundoff, an accuracy the instruction set or the math
library states, or a factor that covers a second-order term.  Test infrastructure only.

All functions take torch float64 tensors (CPU or GPU) and return float64 tensors of the output's shape.  u = 2^-24 is
fp32's unit roundoff; "z" is a pre-activation, "h" an activation.

Routes:
  * f16x2 -- dlc_sdav_encode_split (csrc/gemm_split_f16.hip): split_layer_bound, split_chain_bound;
  * fp32  -- gemm_bias_act_kernel<float> / splitk_bias_act_kernel<float> (csrc/gemm_dense.hip): gemm_dz, act_bound,
             f32_chain_bound; the same with u = 2^-53 for the fp64 kernels behind TensorWrapper's float64 path.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                    # fp32 unit roundoff
U64 = 2.0 ** -53                  # fp64 unit roundoff
LOG2E = 1.4426950408889634
# fp32's underflow: below 2^-126 a result is subnormal or flushed, and for zl >= 128 v_exp_f32 returns +inf so that the
# reciprocal returns 0 where sigmoid is below 2^-127.  Either way the absolute error stays under 2^-125.
UNDERFLOW = 2.0 ** -125

# Relative accuracies the epilogues are built from.
SPLIT_EXP_REL = 2 * U             # v_exp_f32: 1 ulp, at most 2^-23 of the result
SPLIT_REST_REL = 3 * U            # one + E rounded (u) and v_rcp_f32 (1 ulp, 2u)
EXPF_REL = 4 * U                  # expf (ocml): at most 2 ulp, the math library's documented maximum
F32_REST_REL = 2 * U              # 1 + E rounded, then the IEEE division rounded
EXP64_REL = 4 * U64               # exp in fp64: at most 2 ulp
F64_REST_REL = 2 * U64

SP_X_SHIFT = 11                   # activations are carried as h * 2^11
SP_KS = 32                        # k per slice: one v_mfma_f32_16x16x32_f16


def gamma(n, u=U):
    """gamma_n = n u / (1 - n u): the classical bound on n successive roundings."""
    return n * u / (1.0 - n * u)


def sigmoid(z):
    return torch.sigmoid(z)


def sigmoid_out_bound(z, dz, rel_exp, rel_rest):
    """|computed sigmoid - sigmoid(z)| when the kernel evaluates 1 / (1 + E) at a z~ with |z~ - z| <= dz.

    Input error: sigmoid is evaluated at z~, not z.  By the mean value theorem the change is at most max sigma' on
    [z - dz, z + dz] times dz.  sigma' decreases in |t|, so the maximum sits at |t| = max(|z| - dz, 0).  The global 1/4
    is not used: in saturated layers sigma' is tiny, and that is where the N(0,1) weights put most outputs.

    Evaluation error: with E = exp(-z~) carried with relative error e_exp, 1 + E rounded and the reciprocal rounded,
    1 / ((1 + E (1 + e_exp))(1 + e_add)) (1 + e_rcp) = sigma(z~) (1 + eta) with
    |eta| <= (1 - sigma) |e_exp| + |e_add| + |e_rcp| to first order; E / (1 + E) = 1 - sigma is the factor on the exp
    error.  rel_rest is |e_add| + |e_rcp|.  The second-order terms are covered by eta (1 + eta).
    Plus UNDERFLOW for fp32's underflow range."""
    lo = (z.abs() - dz).clamp_min(0.0)
    slope = sigmoid(lo) * sigmoid(-lo)              # sigma (1 - sigma) without the cancellation of 1 - sigma
    dsig = torch.clamp(slope * dz, max=1.0)
    s_hi = torch.clamp(sigmoid(z) + dsig, max=1.0)
    one_minus_hi = torch.clamp(sigmoid(-z) + dsig, max=1.0)
    eta = rel_exp * one_minus_hi + rel_rest
    return dsig + s_hi * eta * (1.0 + eta) + UNDERFLOW


# ----------------------------------------------------------------------------------------------------- f16x2 (split)
def split_scale_exponent(w):
    """s with max|W| 2^s in [2048, 4096), as sp_scale_kernel picks it (0 for an all-zero layer)."""
    m = float(w.abs().max()) if w.numel() else 0.0
    if not (m > 0.0 and math.isfinite(m)):
        return 0
    _, e = math.frexp(m)                       # m = f 2^e, f in [0.5, 1)
    return max(-100, min(100, 12 - e))


def _slice_step_weights(x_nz, K):
    """3 x the number of non-zero k-slices j' >= j of each row, expanded over the k of slice j: [M, K].

    The accumulator of output (m, n) takes three MFMA steps (P1, P2, P3) per k-slice.  A step whose products are all
    exact zeros adds nothing and rounds nothing, so only slices where row m holds a non-zero input count (zeros in W
    only make the count an over-estimate)."""
    M = x_nz.shape[0]
    ns = (K + SP_KS - 1) // SP_KS
    pad = ns * SP_KS - K
    nz = torch.nn.functional.pad(x_nz.to(torch.float64), (0, pad)).reshape(M, ns, SP_KS).amax(dim=2)
    later = torch.flip(torch.cumsum(torch.flip(nz, [1]), 1), [1])          # non-zero slices j' >= j
    return (3.0 * later).repeat_interleave(SP_KS, dim=1)[:, :K]


def split_layer_bound(h, e_in, w, b, z, final):
    """Bound on |kernel output - sigmoid(z)| for one layer of dlc_sdav_encode_split.

    h [M, K]: the fp64 reference input of the layer; e_in [M, K]: a bound on the error of the input the kernel holds
    (0 for layer 0, whose input is x itself); w [K, N]; b [N] or None; z = h @ w + b [M, N] in fp64; final: the last
    layer (fp64 output) or a hidden one (its output goes on as fp16 pieces of h 2^11).  Returns (bound, dz), dz being the
    bound on the error of the pre-activation.

    Scaled domain (the file header of gemm_split_f16.hip): X = h~ 2^11 and W^ = W 2^s, s from split_scale_exponent.
    Each operand v is carried as two fp16 pieces v1 + v2:
      * |v - v1 - v2| <= 2^-22 |v| + 2^-25.  v1 is v rounded to 11 bits (|v - v1| <= 2^-11 |v|), the remainder is exact
        in the wider type and rounded to 11 bits again, 2^-23 |v|; another 2^-23 |v| covers a double -> fp16
        conversion that goes through fp32.  The 2^-25 is half the spacing of fp16 subnormals: a second piece (or a
        first one) below 2^-14 is subnormal and carries an absolute, not a relative, error.  Exact zeros stay exact.
      * |v2| <= 2^-11 (1 + 2^-10) |v| + 2^-25, and |v1| + |v2| <= (1 + 2^-9) |v| + 2^-24.
    The kernel computes x1.w1 + x2.w1 + x1.w2 = (X - rx)(W^ - rw) - x2 w2: the representation errors rx, rw, their
    product and the dropped x2 w2 term are the REPRESENTATION part (products of fp16 values are exact in fp32).

    ACCUMULATION: one MFMA step (32 exact products added to the fp32 accumulator) errs by at most
    2^-23 (|acc| + sum |products|) -- the model cosine_topk.hip states for the same instruction family, held on the
    device by tests/test_gpu_parity.py::test_score_error_bound_holds.  |acc| after slice j is at most C_j, the sum of
    |products| of slices <= j, so the three steps of slice j err by at most 3 * 2^-23 C_j, and the sum over the non-zero
    slices is 2^-23 sum_j' S_j' * 3 #{non-zero j >= j'} (_slice_step_weights).  (1 + 2^-10) covers errors in |acc|.
    A tighter form of the same model bounds |acc| by the fp64 partial sum in front of the slice (see the code).

    EPILOGUE (z units): zl = fmaf(acc, ninv, bv) with ninv = fp32(-log2 e) / 2^(11+s) (relative error u) and
    bv = fp32(-b log2 e - 11 [hidden]) (u |b log2 e + 11|), and the fma's own rounding u |zl|; with
    |acc ninv| / log2 e <= |z - b| + e_in.|W| + dz_product this is at most
    (2u + 2^-50) (|z - b| + e_in.|W| + dz_product + |b| + 11 / log2 e [hidden]).  Then v_exp_f32 (1 ulp), the
    add (u) and v_rcp_f32 (1 ulp): sigmoid_out_bound.  A hidden layer's output is h 2^11 in fp32 with the same relative
    error; its rounding to fp16 pieces is the next layer's representation error.

    INPUT ERROR: |(h~ - h).W| <= e_in.|W|, carried into dz with the factor (1 + u) of ninv's rounding."""
    K, N = w.shape
    s = split_scale_exponent(w)
    sx, sw = 2.0 ** SP_X_SHIFT, 2.0 ** s
    X = (h.abs() + e_in) * sx
    nzx = (X > 0).to(torch.float64)
    Wh = w.abs() * sw
    nzw = (w != 0).to(torch.float64)
    rho_x = 2.0 ** -22 * X + 2.0 ** -25 * nzx
    x2b = 2.0 ** -11 * (1 + 2.0 ** -10) * X + 2.0 ** -25 * nzx
    # rx |W^| + |X| rw + rx rw + |x2| |w2|, with rw = 2^-22 |W^| + 2^-25 [W != 0] and |w2| <= 2^-11 (1 + 2^-10) |W^| + 2^-25 [W != 0]
    rep = (rho_x * (1 + 2.0 ** -22) + 2.0 ** -22 * X + 2.0 ** -11 * (1 + 2.0 ** -10) * x2b) @ Wh \
        + 2.0 ** -25 * ((X + rho_x + x2b) @ nzw)
    A = (1 + 2.0 ** -9) * X + 2.0 ** -24 * nzx
    B = (1 + 2.0 ** -9) * Wh + 2.0 ** -24 * nzw
    AB = A @ B
    acc = 2.0 ** -23 * (1 + 2.0 ** -10) * ((A * _slice_step_weights(X > 0, K)) @ B)
    ew = e_in @ w.abs()
    # The same model with |acc| taken from the fp64 partial sums: in front of slice j the accumulator is within
    # D = (input error + representation + accumulation so far) of the exact partial sum over the slices before j, and
    # inside the slice it grows by at most S_j.  The three steps of a non-zero slice j err by at most
    # 2^-23 (3 (|partial_(j-1)| + D) + 3 S_j).  Both forms are bounds; the smaller one is taken.
    hs, ws_ = h * sx, w * sw
    partial = torch.zeros_like(AB)
    psum = torch.zeros_like(AB)
    cnt = torch.zeros((X.shape[0], 1), dtype=torch.float64, device=X.device)
    for j in range(0, K, SP_KS):
        nzj = (X[:, j:j + SP_KS] > 0).any(dim=1, keepdim=True).to(torch.float64)
        psum += nzj * partial.abs()
        cnt += nzj
        partial += hs[:, j:j + SP_KS] @ ws_[j:j + SP_KS]
    D = ew * (sx * sw) + rep + acc
    acc = torch.minimum(acc, 2.0 ** -23 * (1 + 2.0 ** -10) * 3.0 * (psum + cnt * D + AB))
    dz_prod = (rep + acc) / (sx * sw)
    babs = b.abs() if b is not None else torch.zeros(N, dtype=torch.float64, device=w.device)
    shift = 0.0 if final else SP_X_SHIFT / LOG2E
    zb = (z - (b if b is not None else 0.0)).abs()
    dz = (dz_prod + ew) * (1 + U) + (2 * U + 2.0 ** -50) * (zb + ew + dz_prod + babs + shift)
    return sigmoid_out_bound(z, dz, SPLIT_EXP_REL, SPLIT_REST_REL), dz


def split_chain_bound(x, ws, bs):
    """The fp64 reference chain h_l = sigmoid(h_{l-1} W_l + b_l) and the propagated bound of each layer:
    [(h_l, bound_l)].  Layer l + 1 sees layer l's bound as its e_in: it enters z as e_l.|W_{l+1}| and, through
    sigmoid_out_bound, with the slope of the next activation."""
    h, e, out = x, torch.zeros_like(x), []
    for l, (w, b) in enumerate(zip(ws, bs)):
        z = h @ w + (b if b is not None else 0.0)
        bound, _ = split_layer_bound(h, e, w, b, z, final=(l == len(ws) - 1))
        h, e = sigmoid(z), bound
        out.append((h, e))
    return out


# ---------------------------------------------------------------------------------------------- fp32 gemm_bias_act
def gemm_dz(abs_ab, K, chunks, bias=None, u=U):
    """|z - z64| for z = A.B + b computed by gemm_bias_act_kernel (and splitk_bias_act_kernel when chunks > 1), z64
    the fp64 value for the same operands.  abs_ab = |A|.|B| in fp64.

    v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain, one rounding per product (the CDNA4 notes), so a
    chunk of k products errs like K roundings.  Split-K sums the chunks' partial results in fp32, chunk by chunk
    (chunks - 1 roundings), and the bias add rounds once: (K + chunks + 1) roundings in all on partial sums bounded by
    |A|.|B| (+ |b| for the last), i.e. gamma_(K+chunks+1) |A|.|B| + u |b|.  The fp64 kernels have the same structure,
    with u = 2^-53 (any summation order of K products within K + chunks roundings)."""
    dz = gamma(K + chunks + 1, u) * abs_ab
    if bias is not None:
        dz = dz + u * bias.abs()
    return dz


def act_bound(act, z, dz, fp64=False):
    """Bound on |act(z~) as the kernel evaluates it - act(z)| for |z~ - z| <= dz.  none and relu are exact and
    1-Lipschitz; sigmoid: sigmoid_out_bound with expf (or exp) and the two roundings of 1 / (1 + E)."""
    if act == 0 or act == 2:
        return dz.clone()
    if fp64:
        return sigmoid_out_bound(z, dz, EXP64_REL, F64_REST_REL) - UNDERFLOW
    return sigmoid_out_bound(z, dz, EXPF_REL, F32_REST_REL)


def f32_chain_bound(x, ws, bs, chunks=lambda K: 1):
    """SDAV(dtype="float32"): the fp64 chain on the fp32 operands (x and the weights as the network holds them) and
    the bound of each layer, [(h_l, bound_l)].  The kernel's input to layer l + 1 is layer l's fp32 output, within e_l:
    the product then sees |h~| <= |h| + e and (h~ - h).W <= e.|W|.  chunks(K): the split-K chunk count of a layer (1
    for one pass)."""
    h, e, out = x, torch.zeros_like(x), []
    for w, b in zip(ws, bs):
        K = w.shape[0]
        z = h @ w + (b if b is not None else 0.0)
        dz = gemm_dz((h.abs() + e) @ w.abs(), K, chunks(K), b) + (e @ w.abs()) * (1 + gamma(K + 1))
        h, e = sigmoid(z), act_bound(1, z, dz)
        out.append((h, e))
    return out


def latency_chunks_max(K):
    """An upper bound on plan_split's chunk count for a K (csrc/gemm_dense.hip): at most ksteps / 8 and at most 64
    chunks, none for fewer than 16 K steps of 16."""
    ksteps = (K + 15) // 16
    return 1 if ksteps < 16 else max(1, min(64, ksteps // 8))


def slice_probes(K, rng):
    """Rows that are non-zero in exactly ONE 32-wide k-slice: [rows, K] fp64 numpy, U(0, 1) in the slice.

    Every slice, the tail slice included, appears in four rows: two in the first 256-row tile and two in the second,
    at row positions (mod 16) that differ from copy to copy.  The rows in between are exact zeros.  A defect that stays
    inside one slice (a stale ring slot, a product dropped in one slice) changes a probe row's output by the size of
    that slice's products, while the bound counts that slice's three steps only."""
    ns = (K + SP_KS - 1) // SP_KS
    rows = 256 + 2 * ns
    x = np.zeros((rows, K))
    for c in range(4):
        for j in range(ns):
            r = (c // 2) * 256 + (c % 2) * ns + (j + 5 * c) % ns
            lo, hi = j * SP_KS, min(K, (j + 1) * SP_KS)
            x[r, lo:hi] = rng.uniform(0, 1, hi - lo)
    return x


def ratio(err, bound):
    """The worst err / bound (the tests assert <= 1); an exact result under a zero bound counts 0."""
    err = err.abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())
