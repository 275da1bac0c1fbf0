"""The decision of the SDAV similarity's int8 arg-min filter in exact integers (NumPy, no library code).

Restated from the definitions in csrc/gram_i8.hip (sim_keys_init_kernel, sim_stream_keys_kernel, sim_rows_kernel, the epilogue
of gram_i8_kernel), csrc/gemm_internal.h (dlc_sim_window) and csrc/match_ref.hip (drop_copies, decided,
pair_score_amin_kernel, stream_argmin_kernel, strip_resolve_kernel):

  quantisation   matrix call: lo / hi = the column extremes, c = lo + 0.5 (hi - lo), s = the largest column range;
                 stream: s = hi - lo, c = centre + (lo + 0.5 (hi - lo)).  inv = 2 * 0.498 / s (= 0.996 / s: the doubling is
                 exact), v = clip((x - c) inv, +-0.498), q = rint(v 2^24)
  digits         q = s1 2^16 + s2 2^8 + s3, s_i in [-128, 127]: the signed low byte, then (q + 128) >> 8, twice
  nb             rint(|v|^2 2^15); sv = the largest row sum of |v| (a stream: over the rows appended so far)
  window         W = ceil((2 Ed + 1e-8) 32768) + 2, Ed = bound_ed(sv, H)
  d2[a, b]       nb[b] - acc[a, b], acc = C2 + ((C3 + (C4 >> 8)) >> 8) (arithmetic shifts: floors), C2 = s1.s1',
                 C3 = s2.s1' + s1.s2', C4 = s3.s1' + s2.s2' + s1.s3'
  a cell         (row patch a of frame i, column frame j > i): best = the FIRST minimum of d2 over the P patches of frame
                 j, the candidates are the patches with d2 - best <= W, later bit-identical copies of an earlier member
                 are dropped (equal content hashes in the library), and the cell is UNDECIDED -- one direct fp64 evaluation,
                 one count in stats[0], its frame pair marked in direct_pairs -- when two or more members remain.

The kernels form |v|^2 and sum |v| as fp64 sums in an order of their own; the model takes the exact sums (math.fsum) and
assert_unambiguous() refuses data on which the order could matter to nb or to W.
"""
import math

import numpy as np

VMAX = 0.498
VARIANTS = (None, "no_s3s1", "c4_last_kstep", "round", "trunc", "skip_last_kstep")


def digits(q):
    """q = s1 2^16 + s2 2^8 + s3 with s_i in [-128, 127] (sim_rows_kernel: the signed low byte, then (q + 128) >> 8)."""
    s3 = ((q + 128) & 255) - 128
    q1 = (q - s3) >> 8
    s2 = ((q1 + 128) & 255) - 128
    s1 = (q1 - s2) >> 8
    assert np.all(s1 * 65536 + s2 * 256 + s3 == q) and s1.min() >= -128 and s1.max() <= 127
    return s1, s2, s3


def bound_ed(sv, h):
    return 2.0 ** -23 * sv + h * (2.0 ** -24 + 2.0 ** -33 + 2.0 ** -46) + 1.004 * 2.0 ** -15 + 2.0 ** -16


def window_arg(sv, h):
    """The argument of the ceil in dlc_sim_window."""
    return (2.0 * bound_ed(sv, h) + 1e-8) * 32768.0


def window(sv, h):
    return int(math.ceil(window_arg(sv, h))) + 2


def centre_scale_matrix(x2):
    """(c [H], inv) of the matrix call for the rows x2 [rows, H]: sim_keys_init_kernel, sim_rows_kernel."""
    lo, hi = x2.min(axis=0), x2.max(axis=0)
    s = float((hi - lo).max())
    return lo + 0.5 * (hi - lo), (2.0 * VMAX / s if s > 0.0 else 0.0)


def centre_scale_stream(h, lo, hi, centre=None):
    """(c [H], inv) of a stream created over the fixed range [lo, hi]: sim_stream_keys_kernel."""
    s = hi - lo
    return (np.zeros(h) if centre is None else np.asarray(centre, dtype=np.float64)) + (lo + 0.5 * (hi - lo)), 2.0 * VMAX / s


def quantise(x2, c, inv):
    """(v fp64, q int64) [rows, H]: sim_centred and the fixed-point value of sim_rows_kernel."""
    v = np.clip((x2 - c) * inv, -VMAX, VMAX)
    return v, np.rint(v * 16777216.0).astype(np.int64)


def row_sums(v):
    """Exact (correctly rounded) |v|^2 and sum |v| of every row."""
    n2 = np.array([math.fsum((r * r).tolist()) for r in v])           # (r * r rounds each square once: see sum_margin)
    sa = np.array([math.fsum(np.abs(r).tolist()) for r in v])
    return n2, sa


def sum_margin(total, h):
    """How far an fp64 sum of h non-negative terms (squares formed by fma or rounded first) can lie from the exact sum
    `total`, in ANY order: h 2^-52 total.  (Higham: |error| <= gamma_{h-1} sum |terms| for every summation order,
    gamma_n = n u / (1 - n u), u = 2^-53; one more u per term for a square rounded before it is added: below
    (h + 1) 2^-53 (1 + 1e-12) total < h 2^-52 total for h >= 2, and for h = 1 the single rounding is 2^-53 total.)"""
    return h * 2.0 ** -52 * total


class Ambiguous(AssertionError):
    pass


def ambiguous_rows(v):
    """Rows whose nb = rint(|v|^2 2^15) could depend on the summation order: |v|^2 2^15 within sum_margin of a half-integer."""
    h = v.shape[1]
    n2, _ = row_sums(v)
    t = n2 * 32768.0
    dist = np.abs(t - np.floor(t) - 0.5)
    return np.nonzero(dist <= sum_margin(n2, h) * 32768.0 + 2.0 ** -30)[0]     # (2^-30: the roundings of t and dist themselves)


def assert_unambiguous(v):
    """Raises unless (1) every row's |v|^2 2^15 is farther from a half-integer than h 2^-52 |v|^2 2^15 (sum_margin, scaled),
    so that any fp64 summation order rounds to the same nb, and (2) the argument of the ceil in W is farther from an
    integer than the same bound on sv = max row sum of |v| carried through Ed: 2 * 2^-23 * 32768 * h 2^-52 sv."""
    h = v.shape[1]
    bad = ambiguous_rows(v)
    if len(bad):
        raise Ambiguous("rows %s: |v|^2 2^15 too close to a half-integer" % bad[:8].tolist())
    _, sa = row_sums(v)
    sv = float(sa.max())
    arg = window_arg(sv, h)
    dist = min(arg - math.floor(arg), math.ceil(arg) - arg)
    slack = 2.0 * 2.0 ** -23 * 32768.0 * sum_margin(sv, h) + 2.0 ** -40 * max(arg, 1.0)   # (+ the fp64 evaluation of arg itself)
    if dist <= slack:
        raise Ambiguous("the window's ceil argument %.17g is too close to an integer" % arg)


def _matmul_exact(a, b):
    """a @ b.T for integer matrices through fp64 BLAS: every product is below 2^14 and every sum below 2^14 H <= 2^29, far
    below 2^53 -- exact."""
    return np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


def _shift8(x, variant):
    if variant == "round":
        return (x + 128) >> 8
    if variant == "trunc":
        return np.where(x >= 0, x >> 8, -((-x) >> 8))
    return x >> 8                                                     # arithmetic: floor


def digit_products(q):
    """The six kept digit products of all row pairs, each split into the k-steps in front of the last 64-column k-step that
    holds data ("cut") and that k-step ("last") -- what every variant of acc_matrix is assembled from:
    (C2, C3, C4 without s3[a] . s1[b], s3[a] . s1[b]) x (cut, last)."""
    s1, s2, s3 = digits(q)
    k_last = 64 * ((q.shape[1] - 1) // 64)
    out = []
    for part in (slice(0, k_last), slice(k_last, None)):
        a1, a2, a3 = s1[:, part], s2[:, part], s3[:, part]
        if a1.shape[1] == 0:
            z = np.zeros((q.shape[0], q.shape[0]), dtype=np.int64)
            out.append((z, z, z, z))
            continue
        m21 = _matmul_exact(a2, a1)
        m31 = _matmul_exact(a3, a1)
        out.append((_matmul_exact(a1, a1), m21 + m21.T, _matmul_exact(a2, a2) + m31.T, m31))
    return out


def acc_matrix(q, variant=None, products=None):
    """acc[a, b] of all row pairs.  variant: None (the kernels'), or one of the subtly WRONG forms the tests must notice:
    no_s3s1 (C4 lacks s3[a] . s1[b]), c4_last_kstep (C4 without the last 64-column k-step that holds data),
    round / trunc (rounding shifts / truncation toward zero for the two floors), skip_last_kstep (all three classes
    without that k-step).  (K-steps behind the last column are zero padding and cannot matter.)"""
    assert variant in VARIANTS, variant
    (c2a, c3a, c4a, xa), (c2b, c3b, c4b, xb) = products if products is not None else digit_products(q)
    if variant == "skip_last_kstep":
        c2, c3, c4 = c2a, c3a, c4a + xa
    elif variant == "c4_last_kstep":
        c2, c3, c4 = c2a + c2b, c3a + c3b, c4a + xa
    elif variant == "no_s3s1":
        c2, c3, c4 = c2a + c2b, c3a + c3b, c4a + c4b
    else:
        c2, c3, c4 = c2a + c2b, c3a + c3b, c4a + c4b + xa + xb
    assert max(np.abs(c2).max(), np.abs(c3).max(), np.abs(c4).max()) < 2 ** 31
    return c2 + _shift8(c3 + _shift8(c4, variant), variant)


def copy_mask(x):
    """[N, P] bool: patch b of frame j is a bit-identical copy of an EARLIER patch of the same frame (drop_copies never keeps
    it: it has that patch's distance to everything and a later index)."""
    n, p, _ = x.shape
    bits = np.ascontiguousarray(x).view(np.uint64)
    out = np.zeros((n, p), dtype=bool)
    for j in range(n):
        for b in range(1, p):
            out[j, b] = any(np.array_equal(bits[j, e], bits[j, b]) for e in range(b))
    return out


class Verdicts:
    """What filter_verdicts() returns.  undecided [N, N, P] bool ([i, j, a]: row patch a of frame i against frame j > i),
    pair_count [N, N] int64 (undecided cells per frame pair, 0 on and under the diagonal), pair_map [N, N] uint8 (the
    pairs with one), total, gap [N, N, P] int64 (runner-up - best of d2, all P patches of frame j; -1 where j <= i or
    P == 1), bi [N, N, P] (the first minimum), d2 [N P, N P], W, sv, v, q."""


class FilterModel:
    """The quantised data set and what every verdict rests on: v, q, nb, sv, W, the copies, the digit products (formed once;
    verdicts(variant=) assembles each variant's acc from them)."""

    def __init__(self, x, c=None, inv=None, check=True):
        n, p, h = x.shape
        x = np.ascontiguousarray(x, dtype=np.float64)
        x2 = x.reshape(n * p, h)
        if c is None:
            c, inv = centre_scale_matrix(x2)
        self.shape = (n, p, h)
        self.flat = not (inv > 0.0)                                   # every column constant: all patches the same row
        self.v, self.q = quantise(x2, c, inv)
        if check and not self.flat:
            assert_unambiguous(self.v)
        n2, sa = row_sums(self.v)
        self.sv = float(sa.max())
        self.W = window(self.sv, h)
        self.nb = np.rint(n2 * 32768.0).astype(np.int64)
        self.copy = copy_mask(x)
        self.products = digit_products(self.q)

    def verdicts(self, variant=None, copies=True):
        n, p, h = self.shape
        r = Verdicts()
        r.shape, r.W, r.sv, r.v, r.q, r.nb = self.shape, self.W, self.sv, self.v, self.q, self.nb
        r.d2 = self.nb[None, :] - acc_matrix(self.q, variant, self.products)        # [a, b]
        d3 = r.d2.reshape(n, p, n, p).transpose(0, 2, 1, 3)           # [i, j, a, b]
        upper = np.triu(np.ones((n, n), dtype=bool), 1)[:, :, None]
        best = d3.min(axis=3)
        r.bi = d3.argmin(axis=3)                                      # the first minimum
        if p > 1:
            second = np.partition(d3, 1, axis=3)[..., 1]
            r.gap = np.where(upper, second - best, -1)
        else:
            r.gap = np.full((n, n, p), -1, dtype=np.int64)
        cand = (d3 - best[..., None]) <= r.W
        if copies:
            cand &= ~self.copy[None, :, None, :]
        r.undecided = (cand.sum(axis=3) >= 2) & upper & (not self.flat)
        r.pair_count = r.undecided.sum(axis=2).astype(np.int64)
        r.pair_map = (r.pair_count > 0).astype(np.uint8)
        r.total = int(r.pair_count.sum())
        r.cells = n * (n - 1) // 2 * p
        r.at_w = int((r.gap == r.W).sum())
        r.at_w1 = int((r.gap == r.W + 1).sum())
        return r


def filter_verdicts(x, c=None, inv=None, variant=None, copies=True, check=True):
    """The filter's verdicts on x [N, P, H] fp64.  c / inv: the stream's centre and scale (centre_scale_stream); default: the
    matrix call's (centre_scale_matrix).  copies=False: without the copy rule.  check: assert_unambiguous first."""
    return FilterModel(x, c, inv, check).verdicts(variant, copies)


def summary_line(r, what=""):
    n, p, h = r.shape
    return "filter verdicts %s(N, P, H) = (%d, %d, %d): W = %d, undecided %d / %d cells, %d at gap W, %d at W + 1" % (
        what + " " if what else "", n, p, h, r.W, r.total, r.cells, r.at_w, r.at_w1)


def stream_query_counts(r):
    """[N]: what stats[0] of the stream query of frame f holds -- the undecided cells of the pairs (j, f), j < f."""
    return r.pair_count.sum(axis=0)


# ---- data on which the verdicts are sharp ---------------------------------------------------------------------------------
UNIT = 2.0 ** -20


def sharp_data(n, p, h, amp, ncol, seed):
    """[N, P, H] fp64, every value a multiple of 2^-20 in [0, 1]: one random base row per frame, every patch the base with
    `ncol` columns (min(ncol, H)) moved by integers in [-amp, amp] -- so the nearest patch and the runner-up of a cell lie
    a few window widths apart.  The sentinels -- frame 0's patch 0 all 0.0 and patch 1 all 1.0; with P == 1 the frames 0
    and 1 -- pin every column's range to [0, 1]: c = 0.5, inv = 0.996 and sv = 0.498 H for the data set and for every
    subset that holds the sentinel frame(s), and for a stream over (0, 1).  A row that fails the unambiguity check is
    drawn again (the same generator: deterministic)."""
    rng = np.random.RandomState(seed)
    amp = int(amp)
    assert 0 < amp < 2 ** 19
    k = min(ncol, h)
    base = rng.randint(amp, 2 ** 20 - amp + 1, size=(n, h))

    def patch(f):
        row = base[f].copy()
        cols = rng.choice(h, k, replace=False)
        row[cols] += rng.randint(-amp, amp + 1, size=k)
        return row

    xi = np.stack([np.stack([patch(f) for _ in range(p)]) for f in range(n)]).astype(np.int64)
    sentinels = [(0, 0), (0, 1)] if p > 1 else [(0, 0), (1, 0)]
    xi[sentinels[0]] = 0
    xi[sentinels[1]] = 2 ** 20
    c, inv = np.full(h, 0.5), 2.0 * VMAX
    for _ in range(64):
        x = xi.astype(np.float64) * UNIT
        v, _q = quantise(x.reshape(n * p, h), c, inv)
        bad = ambiguous_rows(v)
        if not len(bad):
            break
        for r_ in bad:
            f, b = divmod(int(r_), p)
            assert (f, b) not in sentinels, "a sentinel row is ambiguous at this width"
            xi[f, b] = patch(f)
    else:
        raise Ambiguous("rows stayed ambiguous")
    x = xi.astype(np.float64) * UNIT
    assert x.min() == 0.0 and x.max() == 1.0
    assert_unambiguous(quantise(x.reshape(n * p, h), c, inv)[0])
    return x


def with_copies(x):
    """Twins inside every frame (patch 1 = patch 0, patch 5 = patch 4) and one repeated frame (the last = frame 2); the
    sentinel rows move to frame 0's patches 2 and 3 so that the range stays pinned."""
    x = x.copy()
    n, p, h = x.shape
    assert p >= 6 and n >= 4
    x[:, 1] = x[:, 0]
    x[:, 5] = x[:, 4]
    x[n - 1] = x[2]
    x[0, 2] = 0.0
    x[0, 3] = 1.0
    return x


# (N, P, H): amp, ncol, seed -- chosen on the CPU so that the sharpness and the mutation conditions of
# test_filter_oracle_cpu.py hold; the GPU tests (test_gpu_filter_verdicts.py) use exactly these
#   N above the smallest that reaches the seam where a condition needed it: (16, 30, 1) for 9 frames, (16, 32, 64) for 10,
#   (60, 2, 255) for 30; H = 2500 takes 8 columns per patch (with 2, every row patch of a frame pair sits at the same gap
#   and the truncation variant moved fewer than 3 pairs even at 48 frames)
SHAPES = {
    (16, 30, 1): (14000, 1, 3),
    (20, 16, 63): (3000, 2, 1),
    (16, 32, 64): (3000, 2, 1),
    (40, 7, 65): (3000, 2, 1),
    (60, 2, 255): (1500, 2, 2),
    (44, 30, 256): (3000, 2, 1),
    (24, 13, 257): (2500, 2, 1),
    (24, 30, 2500): (3000, 8, 1),
    (300, 1, 64): (3000, 2, 1),
}
SHARP_SHAPES = tuple(k for k in SHAPES if k[1] >= 2)
PAIR_SHAPES = ((44, 30, 256), (24, 13, 257), (16, 32, 64))            # frame-pair resolution: three-frame calls
STREAM_SHAPES = ((24, 13, 257), (16, 32, 64), (20, 16, 63), (24, 30, 2500))
MAX_PAIRS = 60


def boundary_pairs(r, cap=MAX_PAIRS):
    """The frame pairs (i, j) with a cell at gap W or W + 1, in row-major order; more than `cap`: every
    ceil(count / cap)-th of them."""
    ii, jj = np.nonzero(((r.gap == r.W) | (r.gap == r.W + 1)).any(axis=2))
    pairs = list(zip(ii.tolist(), jj.tolist()))
    step = -(-len(pairs) // cap) if pairs else 1
    return pairs[::step][:cap]


def subset_frames(i, j):
    """The three-frame data set of a pair: the sentinel frame 0, i, j (two frames when i is the sentinel frame)."""
    return sorted({0, i, j})


def subset_count(r, frames):
    """The undecided cells of the data set made of `frames` (ascending, the sentinel frame among them): the range, the
    scale and sv are the whole set's, so every cell keeps its d2 and W and the count is the sum over the subset's pairs."""
    return int(sum(r.pair_count[a, b] for k, a in enumerate(frames) for b in frames[k + 1:]))


_CACHE = {}


def shape_model(key):
    """(x, FilterModel, Verdicts) of a shape of SHAPES, or of ("copies", N, P, H) = with_copies() of that shape's data;
    formed once per process and shared by the tests (nobody writes to them)."""
    if key not in _CACHE:
        base = key[1:] if key[0] == "copies" else key
        n, p, h = base
        amp, ncol, seed = SHAPES[base]
        x = sharp_data(n, p, h, amp, ncol, seed)
        if key[0] == "copies":
            x = with_copies(x)
        x.setflags(write=False)
        m = FilterModel(x)
        _CACHE[key] = (x, m, m.verdicts())
    return _CACHE[key]
