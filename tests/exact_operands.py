"""fp64 GEMM operands whose product is EXACT in fp64 in any summation order, and the guard bands the operand tests put
around A, B, bias and C.  Test infrastructure only (tests/test_exact_operands_cpu.py shows the premise and that each
modelled defect is seen; tests/test_gpu_gemm_f64_operands.py holds the HIP kernels to it).

  A    integers in [-512, 512]      times 2^-9        |A| <= 1
  B    integers in [-512, 512]      times 2^-15       |B| <= 2^-6
  bias integers in [-2^15, 2^15)    times 2^-15       |bias| <= 1

A product a b is an integer of at most 2^18 in magnitude times 2^-24; a sum of K of them, in any order and over any
subset (a split-K chunk, a tile's partial sum), is an integer below K 2^18 times 2^-24, and so is that sum plus the bias (a
multiple of 2^-15 = 2^9 quanta).  While K 2^18 < 2^53 every such integer is a double: no addition rounds, a fused
multiply-add rounds nothing either, and z = A . B + bias is the same double whatever order a kernel sums in.  For K <= 8192
the integers stay below 2^31.  z has a standard deviation of about 0.65 at K = 4096 (0.58 from the bias alone): a sigmoid
behind it is nowhere saturated.

What a result is compared with is therefore ONE array, at zero tolerance for act none / relu: a dropped, doubled or
misplaced k element, a chunk left out of a split-K sum, a k read from padding -- each changes integers, not roundings.
"""
import numpy as np
import torch

A_SHIFT, B_SHIFT, BIAS_SHIFT = 9, 15, 15
Z_SHIFT = A_SHIFT + B_SHIFT                       # z is an integer times 2^-24
A_MAX = B_MAX = 512
# C's pre-fill: a quiet NaN with a payload -- a word the kernels cannot produce (a cell left unwritten inside C is then a NaN
# as well as a mismatch); compared as int64
SENTINEL = 0x7FF8C0DEC0DE0001


def check_premise(K):
    """Refuses a K at which a sum of K products could leave the integers a double holds exactly."""
    if K < 1 or K * (A_MAX * B_MAX) >= 2 ** 53:
        raise ValueError("exact_operands: K = %d breaks the premise K * 2^18 < 2^53" % K)


def draw_integers(rng, M, N, K):
    """(ai [M, K], bi [K, N], ci [N]) int64: the operands as integers."""
    check_premise(K)
    ai = rng.randint(-A_MAX, A_MAX + 1, size=(M, K)).astype(np.int64)
    bi = rng.randint(-B_MAX, B_MAX + 1, size=(K, N)).astype(np.int64)
    ci = rng.randint(-2 ** BIAS_SHIFT, 2 ** BIAS_SHIFT, size=N).astype(np.int64)
    return ai, bi, ci


def to_float(ai, bi, ci):
    """The fp64 operands (a [M, K], b [K, N], bias [N]) of the integers: exact scalings by powers of two."""
    return ai * 2.0 ** -A_SHIFT, bi * 2.0 ** -B_SHIFT, ci * 2.0 ** -BIAS_SHIFT


def draw(rng, M, N, K):
    """(a [M, K], b [K, N], bias [N]) float64 NumPy arrays."""
    return to_float(*draw_integers(rng, M, N, K))


def int_product(ai, bi, ci=None):
    """z = A . B (+ bias) from int64 arithmetic: the integer quanta scaled by 2^-24 (exact)."""
    q = ai @ bi
    if ci is not None:
        q = q + ci * 2 ** (Z_SHIFT - BIAS_SHIFT)
    assert np.abs(q).max() < 2 ** 53
    return q * 2.0 ** -Z_SHIFT


def product(a, b, bias=None):
    """z in fp64 on the host: by the premise, the true z with no rounding."""
    z = a @ b
    return z + bias if bias is not None else z


def sigmoid_ref(z):
    """sigmoid(z) rounded once to fp64: evaluated in the host's extended precision (64-bit significand) where NumPy has
    one, so that the reference's own error is a rounding to double and no more."""
    zl = np.asarray(z, dtype=np.longdouble)
    return (1.0 / (1.0 + np.exp(-zl))).astype(np.float64)


# ---- guard bands -------------------------------------------------------------------------------------------------------
def _column_offset(ld, misaligned):
    """Column (0 or 1) of row 1 of a pitch-ld buffer of 8-byte words that is / is not on a 16-byte boundary."""
    return 0 if misaligned is None else (int(bool(misaligned)) - ld) & 1


def _view(buf, R, W, ld, misaligned):
    off = _column_offset(ld, misaligned)
    if ld < W + off:
        raise ValueError("a pitch of %d cannot hold %d columns at column offset %d" % (ld, W, off))
    view = buf[1:R + 1, off:off + W]
    if misaligned is not None and buf.element_size() == 8 and buf.data_ptr() % 16 == 0:
        assert view.data_ptr() % 16 == (8 if misaligned else 0)
    return view


def banded(x, ld, misaligned, fill=float("nan")):
    """x [R, W] (a 2-D torch tensor) inside a `fill`-filled buffer of R + 2 rows of pitch ld: a row of fill before it and one
    after, fill in the columns it does not cover.  The view starts at row 1 and at column 0 or 1, whichever puts its first
    element on a 16-byte boundary (misaligned False) or 8 bytes off one (True) for an 8-byte type and a 16-byte-aligned
    allocation; None: column 0, wherever that falls (a tight pitch).  -> (buffer [R + 2, ld], view [R, W] of it holding x)."""
    R, W = x.shape
    buf = torch.full((R + 2, ld), fill, dtype=x.dtype, device=x.device)
    view = _view(buf, R, W, ld, misaligned)
    view.copy_(x)
    return buf, view


def banded_vector(v, fill=float("nan")):
    """v [N] with one `fill` element on either side.  -> (buffer [N + 2], view)."""
    buf = torch.full((v.numel() + 2,), fill, dtype=v.dtype, device=v.device)
    buf[1:-1] = v
    return buf, buf[1:-1]


def sentinel_output(M, N, ld, misaligned, device):
    """C [M, N] inside a SENTINEL-filled fp64 buffer, laid out as banded().  -> (buffer, view)."""
    buf = torch.full((M + 2, ld), SENTINEL, dtype=torch.int64, device=device).view(torch.float64)
    return buf, _view(buf, M, N, ld, misaligned)


def guard_intact(buf, view):
    """Every word of the fp64 buffer outside the view still holds SENTINEL (compared as int64) and no word inside is a NaN."""
    words = buf.view(torch.int64).clone()
    M, N = view.shape
    off = (view.data_ptr() - buf.data_ptr()) // 8 - buf.shape[1]
    words[1:M + 1, off:off + N] = SENTINEL
    return bool((words == SENTINEL).all()) and not bool(torch.isnan(view).any())
