"""Host helpers for the stages BETWEEN the GEMMs of the CnnVtl tolerance mode (dlc_cnnvtl_encode_split,
csrc/gemm_split_f16.hip: cs_input_kernel, cs_maxpool_kernel, the per-frame min / max fold of the SP_CONV epilogue,
cs_quant_gather_kernel, conv_run_layers) and for their fp64 twins in csrc/cnnvtl.hip.  NumPy only, test infrastructure
only; shared by tests/test_cnn_vtl_chain_cpu.py and tests/test_gpu_cnn_vtl_f16x2_chain.py, which walk the SAME case tables
(every copy-network case the GPU file runs is first held to exactness on the CPU).

COPY NETWORKS.  A convolution whose kernel is a one-hot tap times the identity (w[ky, kx] = I, every other tap zero; or
a 1x1 kernel with w = I) copies its input.  With integer inputs |x| <= 255 and an integer bias the f16x2 mode computes
it EXACTLY: x 2^sx is an integer below 2048 (its first fp16 piece holds it, the second is 0), W 2^sw is 2048, every
output has one non-zero product, the descale is a power of two and the fma with an integer bias is exact.  Every stage
behind such a GEMM can therefore be compared with ==.

expected_bytes() is oracle.cnn_vtl.quantize_int8's formula, (d - min) * (255 / (max - min)), truncation, wrap modulo 256,
on the per-frame concatenation, with three cases that formula leaves to NumPy's cast of NaN / inf and that are THIS
REPOSITORY'S definitions (quant_gather_kernel, cs_quant_gather_kernel: a scaled value that is NaN or not below 9e18 in
magnitude gives 0):
  * a column outside [0, width) gives byte 0;
  * a frame with max == min gives all bytes 0;
  * a frame whose 255 / (max - min) overflows fp64 (a range below ~1.4e-306: subnormal rows) gives all bytes 0.
None of them is reached through a cast of NaN here: they are written out."""
import functools
from collections import namedtuple

import numpy as np

from oracle import cnn_vtl as ocnn

ACT_NONE, ACT_RELU = 0, 2                      # include/dlc.h: DLC_ACT_NONE, DLC_ACT_RELU
GRID_WRAP_F32 = 256 * 32 * 256                 # elements one sweep of the fp32 element-wise kernels' largest grid covers
GRID_WRAP_F64 = 256 * 64 * 256                 # ... of the fp64 ones (cnnvtl.hip)
BRANCHES = ("wave", "block", "row")

# k x k kernel, w[tap] = I (stride `stride`, SAME padding), integer bias [c], ReLU or none, pool: 3x3 / 2 VALID behind it
CopyLayer = namedtuple("CopyLayer", "k tap stride bias relu pool")


def same_geometry(h, w, k, s):
    """(pad_top, pad_left, oh, ow) of a k x k SAME convolution (TF: the extra pad goes behind)."""
    oh, ow = -(-h // s), -(-w // s)
    ph, pw = max((oh - 1) * s + k - h, 0), max((ow - 1) * s + k - w, 0)
    return ph // 2, pw // 2, oh, ow


def identity_layer(bias, relu=False, pool=0):
    return CopyLayer(1, (0, 0), 1, np.asarray(bias, dtype=np.float64), relu, pool)


def layer_geometry(layers, h, w):
    """The engine's geometry rows (kh, kw, cin, cout, stride, pad_top, pad_left, oh, ow, act, pool) of a copy network
    whose first layer reads [h, w, c]."""
    geom = []
    for L in layers:
        c = L.bias.size
        pt, pl, oh, ow = same_geometry(h, w, L.k, L.stride)
        geom.append((L.k, L.k, c, c, L.stride, pt, pl, oh, ow, ACT_RELU if L.relu else ACT_NONE, int(L.pool)))
        h, w = oh, ow
        if L.pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return geom


def layer_weights(layers):
    """HWIO kernels [k, k, c, c] of the copy layers."""
    ws = []
    for L in layers:
        c = L.bias.size
        w = np.zeros((L.k, L.k, c, c), dtype=np.float64)
        w[L.tap[0], L.tap[1]] = np.eye(c)
        ws.append(w)
    return ws


def copy_layer(x, L):
    """One copy layer in plain NumPy: out[oy, ox] = x[oy s - pad_top + ky, ox s - pad_left + kx] (0 outside) + bias."""
    n, h, w, c = x.shape
    pt, pl, oh, ow = same_geometry(h, w, L.k, L.stride)
    out = np.zeros((n, oh, ow, c), dtype=np.float64)
    iy = np.arange(oh) * L.stride - pt + L.tap[0]
    ix = np.arange(ow) * L.stride - pl + L.tap[1]
    oky, okx = (iy >= 0) & (iy < h), (ix >= 0) & (ix < w)
    out[np.ix_(np.arange(n), np.nonzero(oky)[0], np.nonzero(okx)[0])] = x[np.ix_(np.arange(n), iy[oky], ix[okx])]
    out = out + L.bias
    return np.maximum(out, 0.0) if L.relu else out


def layer_inputs(x, layers, feats=None):
    """Each layer's input: x, then the previous layer's output (feats[l - 1], default: the expected one), max-pooled on
    the host where that layer pools."""
    feats = expected_features(x, layers) if feats is None else feats
    ins = [np.asarray(x, dtype=np.float64)]
    for l in range(1, len(layers)):
        f = np.asarray(feats[l - 1], dtype=np.float64)
        ins.append(ocnn.maxpool3x3s2(f) if layers[l - 1].pool else f)
    return ins


def expected_features(x, layers):
    """The per-layer outputs [n, oh, ow, c] of a copy network on integer frames x [n, h, w, c], fp64 (exact integers).
    The pool of the LAST layer feeds nothing: the features are the layers' own outputs."""
    h = np.asarray(x, dtype=np.float64)
    outs = []
    for L in layers:
        y = copy_layer(h, L)
        outs.append(y)
        h = ocnn.maxpool3x3s2(y) if L.pool and min(y.shape[1:3]) >= 3 else y
    return outs


def space_to_depth(x, s):
    n, h, w, c = x.shape
    return x.reshape(n, h // s, s, w // s, s, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // s, w // s, s * s * c)


def concat_features(features_per_layer):
    n = features_per_layer[0].shape[0]
    return np.concatenate([np.asarray(f, dtype=np.float64).reshape(n, -1) for f in features_per_layer], axis=1)


def expected_bytes(features_per_layer, cols, minmax=None):
    """int8 [n, len(cols)] (the file header).  minmax = (min [n], max [n]): a range other than the frames' own -- what a
    modelled defect of the fold left in the keys."""
    d = concat_features(features_per_layer)
    n, width = d.shape
    cols = np.asarray(cols, dtype=np.int64)
    mn, mx = (d.min(axis=1), d.max(axis=1)) if minmax is None else (np.asarray(minmax[0]), np.asarray(minmax[1]))
    inside = (cols >= 0) & (cols < width)
    g = d[:, np.where(inside, cols, 0)]
    with np.errstate(divide="ignore", over="ignore"):
        scale = np.float64(255) / (mx - mn)
    live = (mx != mn) & np.isfinite(scale) & np.isfinite(mx - mn)      # the two all-zero frame cases, written out
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.where(live.reshape(-1, 1), (g - mn.reshape(-1, 1)) * scale.reshape(-1, 1), 0.0)
    assert np.isfinite(scaled).all()
    out = (np.trunc(scaled).astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8)
    out[~live] = 0
    out[:, ~inside] = 0                                        # the out-of-range column case, written out
    return out


# ---- the fold of the SP_CONV epilogue ------------------------------------------------------------------------------
def fold_branch(m, rows_per_frame, M):
    """Which of the epilogue's three wave-uniform branches folds output row m of an [M, N] layer output into the keys:
    'wave' (the wave's 64 rows, clipped to M, lie in one frame), 'block' (the 16-row block does), 'row'."""
    w0 = 64 * (m // 64)
    wl = min(w0 + 63, M - 1)
    if w0 // rows_per_frame == wl // rows_per_frame:
        return "wave"
    m0 = 16 * (m // 16)
    ml = min(m0 + 15, M - 1)
    if m0 // rows_per_frame == ml // rows_per_frame:
        return "block"
    return "row"


def fold_branches(rows_per_frame, M):
    """fold_branch of every row, as indices into BRANCHES."""
    m = np.arange(M)
    w0, m0 = m // 64 * 64, m // 16 * 16
    wave = w0 // rows_per_frame == np.minimum(w0 + 63, M - 1) // rows_per_frame
    block = m0 // rows_per_frame == np.minimum(m0 + 15, M - 1) // rows_per_frame
    return np.where(wave, 0, np.where(block, 1, 2))


def fold_model(features_per_layer, drop=None, whole_column_groups_only=False):
    """(min [n], max [n]) the keys hold after every layer folded its outputs: per layer one per-frame min / max in three
    passes, each over the rows fold_branch assigns to it.  Modelled defects: drop = a branch whose pass never runs;
    whole_column_groups_only: columns >= 64 * (N // 64) are not looked at (layers narrower than 64 are left alone)."""
    n = features_per_layer[0].shape[0]
    mn, mx = np.full(n, np.inf), np.full(n, -np.inf)
    for f in features_per_layer:
        N = f.shape[-1]
        y = np.asarray(f, dtype=np.float64).reshape(-1, N)
        M = y.shape[0]
        rpf = M // n
        if whole_column_groups_only and N >= 64:
            y = y[:, :64 * (N // 64)]
        rmn, rmx = y.min(axis=1), y.max(axis=1)
        br = fold_branches(rpf, M)
        frame = np.arange(M) // rpf
        for b in range(3):
            if BRANCHES[b] == drop:
                continue
            sel = br == b
            np.minimum.at(mn, frame[sel], rmn[sel])
            np.maximum.at(mx, frame[sel], rmx[sel])
    return mn, mx


def lonely(m, rows_per_frame, M):
    """Row m is the only row of its frame inside its 16-row block."""
    f = m // rows_per_frame
    lo, hi = max(f * rows_per_frame, 16 * (m // 16)), min((f + 1) * rows_per_frame - 1, 16 * (m // 16) + 15, M - 1)
    return lo == hi


# ---- case tables -----------------------------------------------------------------------------------------------------
def _bias(rng, c, lo=-40, hi=40):
    return rng.randint(lo, hi, size=c).astype(np.float64)


# A1: (n, h, w, c, s2d, dtype name); the last one sweeps cs_input_kernel's grid more than once
A1_SHAPES = ((3, 8, 12, 3), (2, 12, 20, 1), (5, 4, 4, 5))
A1_CASES = tuple((n, h, w, c, s, dt) for (n, h, w, c) in A1_SHAPES for s in (1, 2, 4) for dt in ("uint8", "float32", "float64")) \
    + ((16, 192, 240, 3, 4, "uint8"),)
assert 16 * 192 * 240 * 3 > GRID_WRAP_F32


def a1_case(case):
    """-> (frames [n, h, w, c] of the case's dtype, [the one 1x1 identity layer over c s^2 channels])."""
    n, h, w, c, s, dt = case
    rng = np.random.RandomState(1000 + 7 * n + 3 * h + s + len(dt))
    x = rng.randint(0, 256, size=(n, h, w, c)) if dt == "uint8" else rng.randint(-255, 256, size=(n, h, w, c))
    return x.astype(dt), [identity_layer(_bias(rng, c * s * s))]


# A2: two identity layers, the first one pools
A2_SHAPES = ((3, 3), (7, 8), (8, 7), (23, 31), (4, 9))
A2_CHANNELS = (5, 16, 70)
A2_KINDS = ("negative", "ties", "last_corner")
A2_BIG = (64, 47, 47, 64)                      # pooled: 64 x 23 x 23 x 64 elements
assert 64 * 23 * 23 * 64 > GRID_WRAP_F32


def a2_frames(kind, n, h, w, c, seed):
    rng = np.random.RandomState(seed)
    if kind == "negative":                                      # every window's maximum is negative
        return rng.randint(-200, 0, size=(n, h, w, c)).astype(np.float64)
    if kind == "ties":                                          # five values: most windows hold their maximum more than once
        return rng.randint(-2, 3, size=(n, h, w, c)).astype(np.float64)
    if kind == "last_corner":                                   # strictly increasing down and to the right
        i, j = np.arange(h).reshape(1, h, 1, 1), np.arange(w).reshape(1, 1, w, 1)
        return (i + j - 150 + rng.randint(-20, 20, size=(n, 1, 1, c))).astype(np.float64)
    return rng.randint(-200, 201, size=(n, h, w, c)).astype(np.float64)


def a2_case(kind, h, w, c, n=3, last_pool=0):
    seed = 2000 + 31 * h + 7 * w + c + len(kind)
    rng = np.random.RandomState(seed)
    lo, hi = (-40, 0) if kind == "negative" else (-40, 40)      # "negative": layer 0's output stays negative too
    layers = [identity_layer(_bias(rng, c, lo, hi), pool=1), identity_layer(_bias(rng, c), pool=last_pool)]
    return a2_frames(kind, n, h, w, c, seed + 1), layers


def all_columns(rng, width):
    """Every column, unsorted, some twice, and the two nearest out-of-range ones."""
    cols = np.concatenate([np.arange(width), rng.randint(0, width, size=max(3, width // 50)), [-1, width]])
    return rng.permutation(cols).astype(np.int64)


def _pick_rows(rng, f, n, rpf, M, reachable=None):
    """Local rows (min_row, max_row) of frame f for its planted extrema: frame 0 first / last row, the last frame first
    row / row M - 1, a frame with a lonely row (the only row of its frame in a 16-row block) gets one there, the others
    rows of the branch the rotation wants where the frame has one."""
    rows = [r for r in range(rpf) if reachable is None or reachable(r)]
    assert rows
    br = {r: fold_branch(f * rpf + r, rpf, M) for r in rows}
    order = [r for r in (0, rpf - 1) if r in br] + [int(r) for r in rng.permutation(rows)]

    def pick(want, avoid):
        for strict in (True, False):
            for r in order:
                if (br[r] == want or not strict) and (r != avoid or len(rows) == 1):
                    return r
        return order[0]

    lone = [r for r in rows if lonely(f * rpf + r, rpf, M)]
    wmin, wmax = BRANCHES[f % 3], BRANCHES[(f + 1 + f // 3) % 3]
    if f == 0 or f == n - 1:
        rmin, rmax = (0 if 0 in br else pick(wmin, None)), (rpf - 1 if rpf - 1 in br else pick(wmax, None))
    elif lone and rpf > 1:
        if f & 1:
            rmin = lone[0]
            rmax = pick(wmax, rmin)
        else:
            rmax = lone[-1]
            rmin = pick(wmin, rmax)
    else:
        rmin = pick(wmin, None)
        rmax = pick(wmax, rmin)
    return rmin, rmax


# A3, one layer: (name, n, h, w, c, layer kind, |base| limit, |bias| limit); the plants are +-255, so |base| + |bias| stays
# below 255 - |bias|.  The dense case fills the range up to the plants (every byte value occurs); in the others a lost
# plant moves the range by a fifth and more.
A3_SINGLE = (
    ("1 row per frame", 600, 1, 1, 70, "1x1", 100, 40),
    ("9 rows per frame", 70, 3, 3, 70, "1x1", 170, 40),
    ("9 rows per frame, dense range", 70, 3, 3, 70, "1x1", 250, 2),
    ("42 rows per frame, 300 columns", 13, 6, 7, 300, "1x1", 100, 40),
    ("130 rows per frame", 5, 10, 13, 70, "1x1", 100, 40),
    ("130 rows per frame, 300 columns", 7, 10, 13, 300, "1x1", 150, 40),
    ("616 rows per frame", 3, 22, 28, 70, "1x1", 100, 40),
    ("stride-2 tap with ReLU", 13, 12, 13, 5, "tap", 100, 40),
)
# A3, three layers: (name, n, h, w, tap of the middle layer); 70 channels
A3_TRIPLE = (
    ("three layers, 130 rows in the last", 9, 21, 27, (1, 2)),
    ("three layers, 42 rows in the last", 14, 13, 15, (1, 0)),
)
A3_NAMES = tuple(c[0] for c in A3_SINGLE + A3_TRIPLE)


def _a3_single(case, seed):
    name, n, h, w, c, kind, lim, blim = case
    assert lim + blim < 255 - blim
    rng = np.random.RandomState(seed)
    x = rng.randint(-lim, lim + 1, size=(n, h, w, c)).astype(np.float64)
    if kind == "1x1":
        L = identity_layer(_bias(rng, c, -blim, blim))
        oh, ow = h, w
        src = lambda r: (r // ow, r % ow)
    else:                                                       # 3x3, tap (2, 0), SAME, stride 2, ReLU: only the maximum survives
        L = CopyLayer(3, (2, 0), 2, _bias(rng, c, -blim, blim), True, 0)
        pt, pl, oh, ow = same_geometry(h, w, 3, 2)
        src = lambda r: ((r // ow) * 2 - pt + 2, (r % ow) * 2 - pl)
    rpf, M = oh * ow, n * oh * ow
    inside = lambda r: 0 <= src(r)[0] < h and 0 <= src(r)[1] < w
    for f in range(n):
        rmin, rmax = _pick_rows(rng, f, n, rpf, M, inside)
        ch = (0, c - 1, int(rng.randint(1, c - 1)))
        cmin, cmax = ch[(f + 1) % 3], ch[f % 3]
        x[(f,) + src(rmin) + (cmin,)] = -255.0
        x[(f,) + src(rmax) + (cmax,)] = 255.0
    return x, [L]


def _a3_triple(case, seed):
    """Layer 0: 1x1 identity, pool.  Layer 1: 3x3 one-hot tap, SAME.  Layer 2: 1x1 identity.  |base + biases| <= 80.
    Column 0 carries b1 + b2 = -30, column c - 1 carries + 30.  EVEN frames are decided by the LAST layer: + 200 at one
    odd input position of column c - 1 (one pooling window holds it) reaches the last layer as 230 + b0, and a 3x3
    window of - 200 in column 0 (one pooled element) as - 230 + b0.  ODD frames are decided by LAYER 0: + 200 in column
    0 (later layers see it 30 lower), - 200 in column c - 1 (no pooling window keeps it)."""
    name, n, h, w, tap = case
    c = 70
    rng = np.random.RandomState(seed)
    x = rng.randint(-60, 61, size=(n, h, w, c)).astype(np.float64)
    b0, b1, b2 = _bias(rng, c, -10, 10), _bias(rng, c, -5, 5), _bias(rng, c, -5, 5)
    b1[0], b2[0], b1[c - 1], b2[c - 1] = -10, -20, 10, 20
    layers = [identity_layer(b0, pool=1), CopyLayer(3, tap, 1, b1, False, 0), identity_layer(b2)]
    ph, pw = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    pooled = lambda r: (r // pw - 1 + tap[0], r % pw - 1 + tap[1])           # the pooled element a last-layer row copies
    reach = lambda r: 0 <= pooled(r)[0] < ph and 0 <= pooled(r)[1] < pw
    for f in range(n):
        if f % 2 == 0:
            rmin, rmax = _pick_rows(rng, f, n, ph * pw, n * ph * pw, reach)
            (py, px), (qy, qx) = pooled(rmax), pooled(rmin)
            x[f, 2 * py + 1, 2 * px + 1, c - 1] = 200.0
            x[f, 2 * qy:2 * qy + 3, 2 * qx:2 * qx + 3, 0] = -200.0
        else:
            rmin, rmax = _pick_rows(rng, f, n, h * w, n * h * w)
            x[f, rmax // w, rmax % w, 0] = 200.0
            x[f, rmin // w, rmin % w, c - 1] = -200.0
    return x, layers


@functools.lru_cache(maxsize=None)
def a3_case(name):
    """-> (frames, layers, columns, expected features per layer).  Read-only: shared between tests."""
    i = A3_NAMES.index(name)
    x, layers = _a3_single(A3_SINGLE[i], 3000 + i) if i < len(A3_SINGLE) else _a3_triple(A3_TRIPLE[i - len(A3_SINGLE)], 3100 + i)
    feats = expected_features(x, layers)
    cols = all_columns(np.random.RandomState(3200 + i), concat_features(feats).shape[1])
    for a in [x, cols] + feats:
        a.setflags(write=False)
    return x, layers, cols, feats


# A4: (rows per frame -> n, h, w); 1x1 identity over 70 channels
A4_INDEPENDENCE = ((9, 3, 3), (7, 10, 13))


def a4_zero_frame_case():
    rng = np.random.RandomState(4000)
    x = rng.randint(-200, 201, size=(5, 3, 5, 16)).astype(np.float64)
    x[2] = 0.0
    return x, [identity_layer(np.zeros(16))]


def a4_case(n, h, w):
    rng = np.random.RandomState(4100 + n)
    return rng.randint(-255, 256, size=(n, h, w, 70)).astype(np.float64), [identity_layer(_bias(rng, 70))]


def copy_cases():
    """(name, fp64 frames as layer 0 receives them, layers) of EVERY copy-network case the GPU file runs."""
    for case in A1_CASES:
        x, layers = a1_case(case)
        yield "A1 %s" % (case,), space_to_depth(x.astype(np.float64), case[4]), layers
    for kind in A2_KINDS:
        for (h, w) in A2_SHAPES:
            for c in A2_CHANNELS:
                yield ("A2 %s %dx%dx%d" % (kind, h, w, c),) + a2_case(kind, h, w, c)
    n, h, w, c = A2_BIG
    yield ("A2 big",) + a2_case("any", h, w, c, n=n)
    yield ("A2 last layer pools",) + a2_case("any", 23, 31, 16, last_pool=1)
    for name in A3_NAMES:
        yield ("A3 " + name,) + a3_case(name)[:2]
    yield ("A4 zero frame",) + a4_zero_frame_case()
    for n, h, w in A4_INDEPENDENCE:
        yield ("A4 independence %d" % (h * w),) + a4_case(n, h, w)


# ---- C: segments for the fp64 quantiser ----------------------------------------------------------------------------
C_WIDTHS = (1, 255, 257, 3 * 4096 + 5)
C_CASES = tuple((nseg, rows, first) for nseg in (1, 3, 8) for rows in (1, 300) for first in range(4)
                if rows == 1 or first in (0, 3))               # rows = 300: widths from 1 and from 12293 on


def c_case(nseg, rows, first):
    """-> (segments [rows, width_g] fp64, columns).  Segment g is C_WIDTHS[(first + g) % 4] wide.  Row r: magnitude
    1e-310 / 1 / 1e300 (r % 3), values within 0.4 of it, - magnitude and + magnitude planted at two of {first, last
    element of the first, of the last segment}, rotating with r; row 5 is constant."""
    rng = np.random.RandomState(5000 + 100 * nseg + rows + first)
    widths = [C_WIDTHS[(first + g) % 4] for g in range(nseg)]
    total = sum(widths)
    d = rng.uniform(-0.4, 0.4, size=(rows, total))
    spots = sorted({0, widths[0] - 1, total - widths[-1], total - 1})
    for r in range(rows):
        mag = (1e-310, 1.0, 1e300)[(r + first) % 3]
        d[r] *= mag
        if len(spots) > 1:
            a, b = spots[(r // 3) % len(spots)], spots[(r // 3 + 1 + r // 12) % len(spots)]
            b = b if b != a else spots[(spots.index(a) + 1) % len(spots)]
            d[r, a], d[r, b] = -mag, mag
    if rows > 5:
        d[5] = 7.0
    segs, o = [], 0
    for wd in widths:
        segs.append(np.ascontiguousarray(d[:, o:o + wd]))
        o += wd
    return segs, all_columns(rng, total)


# ---- what decides each A3 frame's range ------------------------------------------------------------------------------
Decision = namedtuple("Decision", "which frame layer m col branch count rows_per_frame M N")


def a3_decisions(name):
    """For both extrema of every frame of an A3 case, from the expected features alone: the layer, output row and column
    that hold it, the fold branch of that row, and how often the value occurs in the frame's whole descriptor."""
    _, layers, _, feats = a3_case(name)
    d = concat_features(feats)
    n = d.shape[0]
    starts = np.concatenate([[0], np.cumsum([f[0].size for f in feats])])
    out = []
    for which in ("min", "max"):
        idx = d.argmin(axis=1) if which == "min" else d.argmax(axis=1)
        for f in range(n):
            l = int(np.searchsorted(starts, idx[f], side="right") - 1)
            N = feats[l].shape[-1]
            rpf = feats[l][0].size // N
            m = f * rpf + int(idx[f] - starts[l]) // N
            out.append(Decision(which, f, l, m, int(idx[f] - starts[l]) % N, fold_branch(m, rpf, n * rpf),
                                int((d[f] == d[f, idx[f]]).sum()), rpf, n * rpf, N))
    return out


def a3_summary(name):
    """One line: how many frames' minimum / maximum each (layer, branch) decided."""
    parts = []
    for which in ("min", "max"):
        cnt = {}
        for q in a3_decisions(name):
            if q.which == which:
                cnt[(q.layer, q.branch)] = cnt.get((q.layer, q.branch), 0) + 1
        parts.append(which + ": " + ", ".join("layer %d %s x%d" % (l, b, k) for (l, b), k in sorted(cnt.items())))
    return "%s -- %s" % (name, "; ".join(parts))


def assert_a3_coverage():
    """The A3 case list reaches what it is there for (every fold branch, every plant position), judged from the expected features alone."""
    single = [q for c in A3_SINGLE for q in a3_decisions(c[0])]
    triple = [q for c in A3_TRIPLE for q in a3_decisions(c[0])]
    for c in A3_SINGLE:
        for q in a3_decisions(c[0]):
            assert q.count == 1 or (c[5] == "tap" and q.which == "min"), (c[0], q)      # (ReLU: the minimum is the zero class)
    for which in ("min", "max"):
        got = {q.branch for q in single if q.which == which and q.count == 1}
        assert got == set(BRANCHES), ("one layer", which, got)
        last = {q.branch for q in triple if q.which == which and q.count == 1 and q.layer == 2}
        assert last == set(BRANCHES), ("last of three layers", which, last)
    for c in A3_TRIPLE:
        by_frame = {}
        for q in a3_decisions(c[0]):
            assert q.count == 1, (c[0], q)
            by_frame.setdefault(q.frame, set()).add(q.layer)
        assert {0} in by_frame.values() and {2} in by_frame.values(), (c[0], by_frame)    # keys accumulate over layers
    plain = [q for q in single if q.count == 1]
    assert {q.rows_per_frame for q in plain} >= {1, 9, 42, 130, 616}
    for q in plain:
        assert q.M > 2 * 256 and q.M % 256 != 0, q
    assert any(q.M % 16 != 0 for q in plain)
    for what, hit in (("a frame's first row", lambda q: q.rows_per_frame > 1 and q.m % q.rows_per_frame == 0),
                      ("a frame's last row", lambda q: q.rows_per_frame > 1 and q.m % q.rows_per_frame == q.rows_per_frame - 1),
                      ("row M - 1", lambda q: q.m == q.M - 1),
                      ("the only row of its frame in a 16-row block", lambda q: q.rows_per_frame > 1 and lonely(q.m, q.rows_per_frame, q.M)),
                      ("column 69 of 70", lambda q: q.N == 70 and q.col == 69),
                      ("column 299 of 300", lambda q: q.N == 300 and q.col == 299),
                      ("column 0", lambda q: q.col == 0)):
        for which in ("min", "max"):
            assert any(hit(q) for q in plain if q.which == which), (what, which)
