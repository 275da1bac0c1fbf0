"""Elementwise error bound for ONE convolution layer of the CnnVtl tolerance mode (dlc_cnnvtl_encode_split,
csrc/gemm_split_f16.hip: gemm_split_f16_kernel<SP_CONV> behind cs_im2col_split_kernel), and a NumPy / torch emulation of
that layer.  Built from the terms of precision_bounds.split_layer_bound; nothing here is fitted to a measurement.
Test infrastructure only: shared by tests/test_conv_precision_bounds_cpu.py (the emulation stays under the bound, modelled
defects exceed it) and tests/test_gpu_cnn_vtl_f16x2.py (which holds the HIP kernels to it at every element).

The layer: y = act(conv(x, W) + b), act = ReLU or none, on an input x the kernel receives exactly (fp32-representable).
  * x of frame f is carried as two fp16 pieces of x 2^sx_f, sx_f from that frame's own max |x| (the largest scaled
    magnitude in [1024, 2048); 0 for an all-zero frame); W as two pieces of W 2^sw (largest in [2048, 4096));
  * per 32-deep k-slice of the im2col row three MFMA steps x1.W1, x2.W1, x1.W2 into one fp32 accumulator;
  * y = fma(acc 2^-sx_f, 2^-sw, fp32(b)), ReLU / none.

geometry = (kh, kw, stride, pad_top, pad_left, oh, ow); x [n, h, w, c]; w [kh, kw, c, cout] (or [kh*kw*c, cout]).
All functions take and return torch float64 tensors (CPU or GPU)."""
import math

import torch

from precision_bounds import SP_KS, U, UNDERFLOW, _slice_step_weights, split_scale_exponent

ACT_NONE, ACT_RELU = 0, 2                  # include/dlc.h: DLC_ACT_NONE, DLC_ACT_RELU
SP_X_TOP = 11                              # a frame's largest |x| 2^sx lies in [2^10, 2^11)


def im2col(x, geometry):
    """x [n, h, w, c] -> [n * oh * ow, kh * kw * c], column order (ky, kx, c): the HWIO kernel viewed as [kh*kw*c, cout].
    Taps outside the image are zeros (TF's SAME padding: pad_top / pad_left in front, whatever is needed behind)."""
    kh, kw, s, pt, pl, oh, ow = geometry
    n, h, w, c = x.shape
    hp = max((oh - 1) * s + kh, pt + h)
    wp = max((ow - 1) * s + kw, pl + w)
    xp = torch.zeros((n, hp, wp, c), dtype=x.dtype, device=x.device)
    xp[:, pt:pt + h, pl:pl + w] = x
    cols = torch.empty((n, oh, ow, kh, kw, c), dtype=x.dtype, device=x.device)
    for i in range(kh):
        for j in range(kw):
            cols[:, :, :, i, j] = xp[:, i:i + (oh - 1) * s + 1:s, j:j + (ow - 1) * s + 1:s]
    return cols.reshape(n * oh * ow, kh * kw * c)


def frame_exponents(x):
    """sx per frame as cs_frame_scale_kernel picks it: max |x| 2^sx in [1024, 2048), 0 for a zero frame, |sx| <= 100."""
    out = []
    for f in range(x.shape[0]):
        m = float(x[f].abs().max()) if x[f].numel() else 0.0
        if not (m > 0.0 and math.isfinite(m)):
            out.append(0)
            continue
        _, e = math.frexp(m)
        out.append(max(-100, min(100, SP_X_TOP - e)))
    return out


def conv_reference(x, w, b, geometry, act):
    """The fp64 convolution of the same input: [n, oh, ow, cout]."""
    kh, kw, s, pt, pl, oh, ow = geometry
    w2 = w.reshape(-1, w.shape[-1])
    z = im2col(x, geometry) @ w2 + (b if b is not None else 0.0)
    if act == ACT_RELU:
        z = z.clamp_min(0.0)
    return z.reshape(x.shape[0], oh, ow, w2.shape[1])


def conv_split_layer_bound(x, w, b, geometry, act):
    """Bound on |kernel output - fp64 conv| at every element: [n, oh, ow, cout].

    Scaled domain, per im2col row m of frame f: X = x 2^sx_f, W^ = W 2^sw.
    REPRESENTATION (as split_layer_bound): an operand v is carried as v1 + v2 with |v - v1 - v2| <= 2^-22 |v| + 2^-25
    (x 2^sx is exact in fp32: a power-of-two multiple of an fp32 value below 2^11), exact zeros stay exact (the zero
    padding and the zero k-tail are zeros), and the kernel drops x2.w2 with |v2| <= 2^-11 (1 + 2^-10) |v| + 2^-25.
    ACCUMULATION: one MFMA step errs by at most 2^-23 (|acc| + sum |products|); three steps per slice in which the row
    holds a non-zero input, |acc| bounded by the sum of |products| so far (_slice_step_weights) or by the fp64 partial
    sum in front of the slice plus the error so far -- both are bounds, the smaller is taken.
    EPILOGUE: acc 2^-sx is exact (a power of two), the fma rounds once (u |y|), fp32(b) is within u |b|; UNDERFLOW covers
    fp32's subnormal range.  ReLU and none are exact and 1-Lipschitz."""
    kh, kw, s, pt, pl, oh, ow = geometry
    n = x.shape[0]
    w2 = w.reshape(-1, w.shape[-1])
    K, N = w2.shape
    sw = 2.0 ** split_scale_exponent(w2)
    sx = torch.tensor([2.0 ** e for e in frame_exponents(x)], dtype=torch.float64, device=x.device)
    sx = sx.repeat_interleave(oh * ow).reshape(-1, 1)                    # per im2col row
    a = im2col(x, geometry)
    z = a @ w2 + (b if b is not None else 0.0)
    X = a.abs() * sx
    nzx = (X > 0).to(torch.float64)
    Wh = w2.abs() * sw
    nzw = (w2 != 0).to(torch.float64)
    rho_x = 2.0 ** -22 * X + 2.0 ** -25 * nzx
    x2b = 2.0 ** -11 * (1 + 2.0 ** -10) * X + 2.0 ** -25 * nzx
    rep = (rho_x * (1 + 2.0 ** -22) + 2.0 ** -22 * X + 2.0 ** -11 * (1 + 2.0 ** -10) * x2b) @ Wh \
        + 2.0 ** -25 * ((X + rho_x + x2b) @ nzw)
    A = (1 + 2.0 ** -9) * X + 2.0 ** -24 * nzx
    B = (1 + 2.0 ** -9) * Wh + 2.0 ** -24 * nzw
    AB = A @ B
    acc = 2.0 ** -23 * (1 + 2.0 ** -10) * ((A * _slice_step_weights(X > 0, K)) @ B)
    hs, ws_ = a * sx, w2 * sw
    partial = torch.zeros_like(AB)
    psum = torch.zeros_like(AB)
    cnt = torch.zeros((X.shape[0], 1), dtype=torch.float64, device=X.device)
    for j in range(0, K, SP_KS):
        nzj = (X[:, j:j + SP_KS] > 0).any(dim=1, keepdim=True).to(torch.float64)
        psum += nzj * partial.abs()
        cnt += nzj
        partial += hs[:, j:j + SP_KS] @ ws_[j:j + SP_KS]
    acc = torch.minimum(acc, 2.0 ** -23 * (1 + 2.0 ** -10) * 3.0 * (psum + cnt * (rep + acc) + AB))
    dz_prod = (rep + acc) / (sx * sw)
    babs = b.abs() if b is not None else torch.zeros(N, dtype=torch.float64, device=x.device)
    dz = dz_prod + U * (z.abs() + dz_prod) + U * babs + UNDERFLOW
    return dz.reshape(n, oh, ow, N)


def _pieces(v):
    """Two fp16 pieces of fp64 / fp32 values already scaled: (v1, v2) as float32."""
    v1 = v.to(torch.float16)
    v2 = (v - v1.to(v.dtype)).to(torch.float16)
    return v1.to(torch.float32), v2.to(torch.float32)


def emulate_conv_split(x, w, b, geometry, act, drop_slice=None, drop_x2w1=False, frame_exponent_of=None):
    """The layer as the kernel computes it, in torch on the CPU: fp16 pieces, three fp32 products per 32-deep slice
    added in slice order (BLAS sums the 32 products of a slice in another order than the MFMA), fp32 epilogue.
    Modelled defects: drop_slice = j (slice j never added), drop_x2w1 (the x2.W1 product missing), frame_exponent_of =
    {f: g} (frame f's rows descaled with frame g's exponent: a tile that spans two frames read one exponent for both).
    -> [n, oh, ow, cout] float64."""
    kh, kw, s, pt, pl, oh, ow = geometry
    n = x.shape[0]
    w2 = w.reshape(-1, w.shape[-1])
    K, N = w2.shape
    sw = split_scale_exponent(w2)
    es = frame_exponents(x)
    sx = torch.tensor([2.0 ** e for e in es], dtype=torch.float32).reshape(n, 1, 1, 1)
    xs = x.to(torch.float32) * sx                                           # exact: power of two
    x1, x2 = _pieces(xs)
    w1, w2p = _pieces(w2 * 2.0 ** sw)
    c1, c2 = im2col(x1, geometry), im2col(x2, geometry)
    acc = torch.zeros((c1.shape[0], N), dtype=torch.float32)
    for j, k0 in enumerate(range(0, K, SP_KS)):
        if drop_slice == j:
            continue
        sl = slice(k0, k0 + SP_KS)
        acc = acc + c1[:, sl] @ w1[sl]
        if not drop_x2w1:
            acc = acc + c2[:, sl] @ w1[sl]
        acc = acc + c1[:, sl] @ w2p[sl]
    des = list(es)
    for f, g in (frame_exponent_of or {}).items():
        des[f] = es[g]
    xinv = torch.tensor([2.0 ** -e for e in des], dtype=torch.float32).repeat_interleave(oh * ow).reshape(-1, 1)
    bv = b.to(torch.float32) if b is not None else torch.zeros(N, dtype=torch.float32)
    # fma(acc * xinv, winv, bv): the product is exact, one rounding in the sum
    y = ((acc * xinv).to(torch.float64) * 2.0 ** -sw + bv.to(torch.float64)).to(torch.float32)
    if act == ACT_RELU:
        y = y.clamp_min(0.0)
    return y.to(torch.float64).reshape(n, oh, ow, N)


def same_geometry(h, w, k, s):
    """(kh, kw, stride, pad_top, pad_left, oh, ow) of a k x k SAME convolution (TF: the extra pad goes behind)."""
    oh, ow = -(-h // s), -(-w // s)
    ph, pw = max((oh - 1) * s + k - h, 0), max((ow - 1) * s + k - w, 0)
    return (k, k, s, ph // 2, pw // 2, oh, ow)


def valid_geometry(h, w, k, s):
    return (k, k, s, 0, 0, (h - k) // s + 1, (w - k) // s + 1)
