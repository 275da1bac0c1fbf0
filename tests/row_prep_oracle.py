"""An exact oracle for the stored bits of dlc_l2_normalize_rows, and fp64 references for the two reductions behind tau_scale
(dlc_max_row_norm, dlc_cosine_tau_scale).  NumPy only: no torch.cuda.

The normalised row.  With m = mean(x) when centring and 0 otherwise, element e of the result is

    r_e = (x_e - m) / ||x - m||

evaluated here in np.longdouble (a 64-bit mantissa).  The kernel forms the same value in fp64 in SOME summation order
(a lane's chain, a butterfly, four partial sums), then rounds fp64 -> fp32 -> bf16 / fp16, both round-to-nearest-even.  An
fp64 evaluation in any order lies within

    beta_e = 2 * (d + 8) * 2^-53 * (|r_e| + [center] mean|x| / ||x - m||)

of r_e: a sum of d terms in any order errs by at most (d - 1) u times the sum of the magnitudes (u = 2^-53), the norm
carries half the relative error of the sum of squares (all terms positive: relative (d + 1) u with the squares' own
rounding), and the subtraction, the reciprocal, the square root and the product add one u each -- d + 8 covers the lot.
When centring, the mean's error (d u mean|x| at most) passes through x_e - m unchanged and is divided by the norm.
Doubled for safety.  The double rounding R is monotone, so a stored value g_e is right iff

    R(r_e - beta_e) <= g_e <= R(r_e + beta_e)          (compared as VALUES)

and where the two ends agree that is bit equality.  Elements whose ends differ are "ambiguous": either neighbour is a
correct result of some order.  tests/test_row_prep_cpu.py proves the argument on four emulated orders and shows that five
modelled defects are seen; tests/test_gpu_row_prep.py holds the kernels to it.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the oracle needs an extended-precision long double"
U53 = 2.0 ** -53

KINDS = ("bf16", "f16")


# --------------------------------------------------------------------------- the stored formats
def decode(bits, kind):
    """uint16 words of the stored format -> their values as float64 (exact)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if kind == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float16).astype(np.float64)


def f32_to_bits(f, kind):
    """float32 -> the stored format's words, round-to-nearest-even (NaN stays a NaN)."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32)
    r = ((u + np.uint32(0x7fff) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(0x7fc0), r)


def round_twice(z, kind):
    """The kernel's contract R: fp64 -> fp32 -> stored format, both to nearest even.  Returns the words."""
    with np.errstate(over="ignore"):
        return f32_to_bits(np.asarray(z, dtype=np.float64).astype(np.float32), kind)


def round_once(z, kind):
    """fp64 -> stored format in ONE rounding to nearest even (not what the kernel does: a modelled defect).  Returns the
    words.  Finite values inside the format's range only."""
    z = np.asarray(z, dtype=np.float64)
    mant, emin = (8, -126) if kind == "bf16" else (11, -14)
    _, e = np.frexp(z)                                        # |z| in [2^(e-1), 2^e)
    q = np.exp2(np.maximum(e - mant, emin + 1 - mant).astype(np.float64))    # the spacing at z (subnormal floor)
    v = np.rint(z / q) * q                                    # both scalings exact: q is a power of two
    return f32_to_bits(v.astype(np.float32), kind)            # v is representable: this conversion is exact


# --------------------------------------------------------------------------- the normalised row
def reference(x, center):
    """x [n, d] (float32 / float64) -> (r, beta) in long double: the normalised rows and each element's radius.  A row
    whose norm is zero gives r = 0, beta = 0 (the kernel stores zeros) -- except a centred row of d > 1 equal elements,
    whose radius is infinite (see below)."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    d = x.shape[1]
    xl = x.astype(LD)
    m = xl.mean(axis=1, keepdims=True) if center else LD(0)
    y = xl - m
    nrm = np.sqrt((y * y).sum(axis=1, keepdims=True))
    safe = np.where(nrm > 0, nrm, LD(1))
    r = y / safe
    u = LD((d + 8) * U53)
    beta = u * np.abs(r)
    if center:
        beta = beta + u * np.abs(xl).mean(axis=1, keepdims=True) / safe
        # a centred row of one repeated value: the exact result is 0 / 0.  With d = 1 the mean is exact and the kernel stores
        # zero; otherwise the fp64 mean may miss by a rounding, x - mean is that noise, normalised -- no statement here
        beta = np.where(nrm > 0, beta, LD(0) if d == 1 else LD(np.inf))
    return r, 2 * beta


def interval(x, center, kind):
    """(lo, hi) float64 [n, d]: the values between which every stored element must lie (ends included)."""
    r, beta = reference(x, center)
    lo = decode(round_twice((r - beta).astype(np.float64), kind), kind)
    hi = decode(round_twice((r + beta).astype(np.float64), kind), kind)
    return lo, hi


def verdict(bits, lo, hi, kind):
    """Stored words against their interval: (outside, ambiguous), two boolean arrays.  NaN is outside."""
    g = decode(bits, kind)
    with np.errstate(invalid="ignore"):
        inside = (lo <= g) & (g <= hi)
    return ~inside, lo != hi


def first_outside(outside, lo, hi, bits, kind):
    """A line for an assertion message: the coordinates and values of the first element outside its interval."""
    where = np.argwhere(outside)
    if where.size == 0:
        return "none outside"
    i, e = (int(v) for v in where[0])
    return "%d outside, first at row %d column %d: stored %r, interval [%r, %r]" % (
        len(where), i, e, float(decode(bits, kind)[i, e]), float(lo[i, e]), float(hi[i, e]))


# --------------------------------------------------------------------------- fp64 emulations of a kernel
ORDERS = ("forward", "reverse", "pairwise", "lanes256")
DEFECTS = ("skip_last_square", "mean_over_ldd", "tail_prev_inv", "odd_last_zero", "single_rounding")


def ordered_sum(v, order):
    """Row sums of v [n, d] in fp64 in the named order."""
    v = np.asarray(v, dtype=np.float64)
    if order == "forward":
        return np.cumsum(v, axis=1)[:, -1]                    # cumsum adds one element at a time
    if order == "reverse":
        return np.cumsum(v[:, ::-1], axis=1)[:, -1]
    if order == "pairwise":
        return v.sum(axis=1)
    if order == "lanes256":                                   # 256 chains with stride 256, then the chains in turn
        n, d = v.shape
        pad = np.zeros((n, (d + 255) // 256 * 256))
        pad[:, :d] = v
        lanes = np.cumsum(pad.reshape(n, -1, 256), axis=1)[:, -1, :]
        return np.cumsum(lanes, axis=1)[:, -1]
    raise ValueError(order)


def emulate(x, center, kind, order, defect=None):
    """The kernel's arithmetic in fp64 with the sums in `order`: mean, centred sum of squares, (x - mean) * (1 / norm), two
    roundings.  `defect` injects one modelled fault.  Returns the stored words [n, d]."""
    assert defect is None or defect in DEFECTS
    x64 = np.asarray(x).astype(np.float64)
    n, d = x64.shape
    vw = 16 // np.asarray(x).dtype.itemsize
    mean = np.zeros((n, 1))
    if center:
        div = (d + 63) // 64 * 64 if defect == "mean_over_ldd" else d
        mean = (ordered_sum(x64, order) / div)[:, None]
    c = x64 - mean
    sq = c * c
    if defect == "skip_last_square":
        sq = sq[:, :-1] if d > 1 else sq * 0.0
    nrm = np.sqrt(ordered_sum(sq, order)) if sq.shape[1] else np.zeros(n)
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 1.0)[:, None]
    z = c * inv
    if defect == "tail_prev_inv" and d % vw:
        z[:, d - d % vw:] = c[:, d - d % vw:] * np.roll(inv, 1, axis=0)
    bits = round_once(z, kind) if defect == "single_rounding" else round_twice(z, kind)
    if defect == "odd_last_zero" and d % 2:
        bits[:, -1] = 0
    return bits


# --------------------------------------------------------------------------- data
def draw(rng, kind, n, d, dtype):
    """Rows of the named kind: 'n01' N(0, 1); 'n100' N(100, 1) (the cancellation in the centred sums); 'spiky' N(0, 1) with
    one element of 1e4 per row (the rest of an fp16 row is subnormal)."""
    x = rng.standard_normal((n, d))
    if kind == "n100":
        x += 100.0
    elif kind == "spiky":
        x[np.arange(n), rng.randint(0, d, n)] = 1e4
    elif kind != "n01":
        raise ValueError(kind)
    return x.astype(dtype)


def equal_row_widths(kind, dmax=4096):
    """Two widths d <= dmax for an all-equal row, whose every element is 1 / sqrt(d): the one that lies closest ABOVE a
    midpoint of two neighbouring values of the stored format (in spacings: every element rounds up by almost half a
    spacing), and the one whose rounding gains the most relative to the value -- the largest stored norm a normalised row
    of up to dmax elements has."""
    d = np.arange(1, dmax + 1)
    v = 1.0 / np.sqrt(d.astype(np.float64))
    mant = 8 if kind == "bf16" else 11
    _, e = np.frexp(v)
    q = np.exp2((e - mant).astype(np.float64))                # the spacing at v
    frac = v / q - np.floor(v / q)                            # position between the two neighbours, in spacings
    closest = int(d[np.argmin(np.where(frac > 0.5, frac - 0.5, np.inf))])
    gain = decode(round_twice(v, kind), kind) / v
    return closest, int(d[np.argmax(gain)])


# --------------------------------------------------------------------------- the reductions behind tau_scale
def stored_norms(bits, kind):
    """fp64 norms of stored rows [n, d] (uint16 words)."""
    v = decode(bits, kind)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt((v * v).sum(axis=1))


def tau_scale_reference(qnorms, R):
    """s_i = max(1, |q_i| R / 1.01); R = None is the 1.005 of rows dlc_l2_normalize_rows wrote."""
    R = 1.005 if R is None else float(R)
    with np.errstate(invalid="ignore"):
        return np.maximum(1.0, np.asarray(qnorms, dtype=np.float64) * R / 1.01)
