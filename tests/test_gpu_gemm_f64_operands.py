"""dlc_gemm_bias_act(DLC_F64) -- the parity-mode arithmetic behind SDAV.transform, DA.transform, the CnnVtl convolutions and
both training steps -- at every pitch and alignment of its operands, on every route the planner takes.

The route of a call depends on properties of the OPERANDS, not only on the problem (plan_gemm / plan_dma_splitk / plan_split
in csrc/gemm_dense.hip, plan_dma_forms / plan_dma_launch in csrc/gemm_dma_f64.hip): lda & 1, ldb & 1, A & 15, B & 15, K & 1,
N & 1 for a [K,N] B, N <= 96, and whether a scratch is set.  Engine.gemm_bias_act makes every operand contiguous, so the rest
of the suite runs with lda == K, a tight ldb, ldc == N and bases at the allocator's alignment.  Here the raw C ABI is called
with operands behind guard bands (tests/exact_operands.py): A in a NaN-filled [M + 2, lda] buffer -- NaN rows before and
after, NaN in the columns it does not cover -- B the same in both layouts, bias inside a NaN-banded vector, C inside a buffer
pre-filled with a sentinel word.  A k read from padding is a NaN in the result; afterwards every word of C's buffer outside
[M, N] must still be the sentinel (as int64) and no NaN may be inside.

Variants, each per shape, B layout, mode (scratch off, scratch on = Engine.latency_mode) and activation:
  V0  tight, through Engine.gemm_bias_act          V4  A's base + 8 bytes, lda even
  V1  lda, ldb, ldc each wider by an even amount   V5  B's base + 8 bytes, ldb even
  V2  lda odd                                      V6  ldc odd, C's base 8 bytes off a 16-byte boundary
  V3  ldb odd                                      V7  bias NULL (compared with V0 run without a bias)

Routes, read from the plan code and checked with an emulation of it.  "DMA tm x tn" is the LDS-DMA kernel in one pass on
that tile, "staged" the register-staged kernel, "c x k" c chunks of k; off -> on is the scratch.  V1, V6 and V7 keep V0's
route (an even pitch and a 16-byte base stay eligible for the LDS-DMA kernel; ldc, C's base and the bias are never looked
at); V2 .. V5 are each refused by plan_dma_launch and take the staged column.  Both layouts alike except where noted.

 shape (M, N, K)     | V0, V1, V6, V7                                   | V2 .. V5
 --------------------+--------------------------------------------------+------------------------------------------
 (70, 130, 64)       | DMA 64 x 128, both modes: four whole K tiles     | staged, both modes (4 K steps < 16)
 (70, 130, 66)       |   ... a K tail of one 16-byte piece              |   ...
 (70, 130, 78)       |   ... a K tail of 14                             |   ...
 (70, 130, 100)      |   ... a K tail of 4                              |   ...
 (1, 130, 4096)      | DMA 64 x 128 -> DMA split-K 32 x 128             | staged -> staged split-K 29 x 144 (tail 64)
 (4000, 1024, 96)    | DMA 128 x 128, both modes                        | staged, both modes (6 K steps)
 (8000, 1024, 80)    | DMA 256 x 128, both modes                        | staged, both modes
 (3900, 96, 70)      | DMA 256 x 96 (the 96-column form), both modes    | staged, both modes
 (3900, 34, 64)      | DMA 256 x 96, one column tile a third full       | staged, both modes
 (37, 53, 29)        | staged by shape (odd K), both modes              | staged
 (64, 128, 48)       | staged by shape (K < 64), both modes             | staged
 (70, 131, 100)      | [K,N]: staged by shape (odd N); [N,K]: DMA 64 x  | staged
                     | 128, N may be odd there.  Both modes             |
 (1, 1, 1)           | staged by shape, both modes                      | staged
 (70, 130, 258)      | DMA 64 x 128 -> DMA split-K 2 x 144, the last    | staged -> staged split-K 2 x 144
                     | chunk 114 = 7 tiles + a tail of 2                |
 (300, 2500, 2500)   | DMA 64 x 128 -> DMA split-K 5 x 512 (last 452)    | staged -> staged split-K 4 x 640
 (60, 96, 4096)      | staged -> staged split-K 29 x 144: N <= 96       | staged -> staged split-K 29 x 144
                     | refuses the DMA split, and 1 tile of 256 rows    |
                     | the 96-column form                               |

ROUTE_DMA_TWO_PART is not here: for plain operands plan_dma_forms never chooses it.  Its cost 'split' is at least R + 0.51 +
0.05 for R whole rounds of 256-row tiles, the 64-row form's 'quarter' at most 0.248 (4 R + 2) + 0.02 whenever the rows left
over fit one round of 128-row tiles (and with two such rounds 'split' grows by another 0.51): split < quarter - 0.03 has no
solution, and a search of the emulation over 1 .. 599 column tiles and up to 179 200 rows found none.  The two-part form is
the convolutions' (0.27 instead of 0.248) and is left to their tests.

The ring of Engine.set_profiling counts launches of product kernels (not the split-K reduce) and gives no kernel's name:
every call here must record exactly one.  One pass against split is pinned by the bits of the N(0, 1) operands instead: the
scratch changes V0's bits for exactly the four shapes whose rows above say "->".

What is asserted.
  Exact operands (tests/exact_operands.py: integers times 2^-9 and 2^-15, every partial sum exact in fp64 in any order): with
  act none and relu the result EQUALS the host's fp64 product (then max(., 0)) bit for bit, on every route, variant and mode;
  with sigmoid it is within precision_bounds.act_bound(SIGMOID, z, dz = 0, fp64 = True) of the sigmoid evaluated in extended
  precision on the host.
  N(0, 1) x N(0, 1) / sqrt(K) operands, one shape per route, so that rounding and cancellation are real: against the fp64
  product on the device, elementwise within 2 * precision_bounds.gemm_dz(|A| |B|, K, chunks, bias, u = 2^-53) carried through
  act_bound -- 2 because the reference's own summation obeys the same bound; chunks = 1 for one pass, 64 (the cap both split
  planners share) where the scratch splits.
  Bit relations the code claims, on both kinds of operands: with the scratch off every variant equals V0 (all one-pass routes
  sum k in one order); with it on, the same call twice gives the same bits, and a variant that keeps V0's route (V1, V6, V7)
  equals V0; one that changes route is held to the oracle only.

Measured on an MI355X: every exact case bit-equal on every route, variant and mode; worst err / bound of the sigmoid over
the exact cases 0.25 (1 x 1 x 1) and 0.53 .. 0.58 (all others: the evaluation of 1 / (1 + exp(-z)) itself); of the N(0, 1)
cases 0.12 (70 x 130 x 100), 0.27 (4000 x 1024 x 96 and 3900 x 96 x 70), 0.47 (8000 x 1024 x 80), 0.17 (37 x 53 x 29), 0.0054
(300 x 2500 x 2500) and 0.00049 (60 x 96 x 4096), the same in both layouts.  The file runs in 6 s.  Mutation check (not
committed): with splitk_bias_act_kernel starting at chunk 1 all eight exact tests of the four shapes that split fail, and the
four N(0, 1) tests of the two split routes.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import exact_operands as xo
import precision_bounds as pb

pytestmark = pytest.mark.gpu

NONE, SIGMOID, RELU = 0, 1, 2
KN, NK = 0, 1

# (M, N, K) -> whether the scratch splits K (on every variant and in both layouts: the table above)
SHAPES = {
    (70, 130, 64): False, (70, 130, 66): False, (70, 130, 78): False, (70, 130, 100): False, (1, 130, 4096): True,
    (4000, 1024, 96): False, (8000, 1024, 80): False, (3900, 96, 70): False, (3900, 34, 64): False,
    (37, 53, 29): False, (64, 128, 48): False, (70, 131, 100): False, (1, 1, 1): False,
    (70, 130, 258): True, (300, 2500, 2500): True, (60, 96, 4096): True,
}
# one shape per route for the N(0, 1) operands: DMA on 64-, 128- and 256-row tiles, the 96-column form, staged, and the two
# split-K routes (scratch on)
ROUTE_SHAPES = [(70, 130, 100), (4000, 1024, 96), (8000, 1024, 80), (3900, 96, 70), (37, 53, 29), (300, 2500, 2500),
                (60, 96, 4096)]
SPLIT_CHUNKS = 64              # plan_split and plan_dma_splitk: at most 64 chunks
KEEPS_ROUTE = ("V1", "V6", "V7")


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def report(what, r):
    print("%-70s worst err/bound %.3g" % (what, r))
    assert r <= 1.0, (what, r)
    return r


def one_launch(eng, fn):
    """fn() with profiling on: its result, after asserting that it recorded exactly one ring entry (one launch of a
    product kernel; a split-K reduce is not one) of a positive duration."""
    eng.set_profiling(True)
    try:
        out = fn()
        ms = eng.profile_gemm_ms()
    finally:
        eng.set_profiling(False)
    assert len(ms) == 1 and ms[0] > 0, ms
    return out


def odd_pitch(w):
    return w + 3 - (w & 1)


def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))


class Operands:
    """The device operands of one (problem, layout) in every variant's layout, built once."""

    def __init__(self, a, b, bias, lay):
        self.M, self.K = a.shape
        self.N = b.shape[1]
        self.lay = lay
        self.a, self.bias = dev(a), dev(bias)
        self.b = dev(b if lay == KN else b.T)
        w = self.b.shape[1]                                       # B's row width: N for [K,N], K for [N,K]
        M, N, K = self.M, self.N, self.K
        # variant -> (lda, A misaligned, ldb, B misaligned, ldc, C misaligned); None: column 0 of a tight pitch
        self.layouts = {
            "V1": (K + 6, False, w + 4, False, N + 2, False),
            "V2": (odd_pitch(K), False, w, None, N, None),
            "V3": (K, None, odd_pitch(w), False, N, None),
            "V4": (K + 2 + (K & 1), True, w, None, N, None),
            "V5": (K, None, w + 2 + (w & 1), True, N, None),
            "V6": (K, None, w, None, odd_pitch(N), True),
            "V7": (K, None, w, None, N, None),
        }
        self.keep, self.views = [], {}
        self.bias_buf, self.bias_view = xo.banded_vector(self.bias)
        for v, (lda, a_mis, ldb, b_mis, _, _) in self.layouts.items():
            abuf, aview = xo.banded(self.a, lda, a_mis)
            bbuf, bview = xo.banded(self.b, ldb, b_mis)
            self.keep += [abuf, bbuf]
            self.views[v] = (aview, bview)
        for v, (lda, a_mis, ldb, b_mis, ldc, c_mis) in self.layouts.items():       # what each variant is there to vary
            aview, bview = self.views[v]
            assert aview.stride(0) == lda and bview.stride(0) == ldb
        assert self.layouts["V2"][0] & 1 and self.layouts["V3"][2] & 1 and self.layouts["V6"][4] & 1
        assert self.views["V4"][0].data_ptr() % 16 == 8 and self.views["V5"][1].data_ptr() % 16 == 8
        assert self.layouts["V4"][0] % 2 == 0 and self.layouts["V5"][2] % 2 == 0
        assert self.views["V1"][0].data_ptr() % 16 == 0 and self.views["V1"][1].data_ptr() % 16 == 0

    def engine_call(self, eng, act, with_bias=True):
        return one_launch(eng, lambda: eng.gemm_bias_act(self.a, self.b, self.bias if with_bias else None, act=act,
                                                         blayout=self.lay))

    def raw_call(self, eng, v, act):
        """Variant v through the C ABI into a fresh sentinel-banded C.  -> C's view, after the guard check."""
        from deeploopcloser_amd import _lib as L
        lda, _, ldb, _, ldc, c_mis = self.layouts[v]
        aview, bview = self.views[v]
        cbuf, cview = xo.sentinel_output(self.M, self.N, ldc, c_mis, "cuda")
        if v == "V6":
            assert cview.data_ptr() % 16 == 8
        bias_ptr = None if v == "V7" else self.bias_view.data_ptr()

        def call():
            eng._check(eng.lib.dlc_gemm_bias_act(eng.ctx, L.DLC_F64, self.lay, act, self.M, self.N, self.K, aview.data_ptr(),
                                                  lda, bview.data_ptr(), ldb, bias_ptr, cview.data_ptr(), ldc, None))
        one_launch(eng, call)
        torch.cuda.synchronize()
        assert xo.guard_intact(cbuf, cview), "%s act %d: a word outside C was written, or a NaN is inside" % (v, act)
        return cview


def sweep(eng, ops, check, split):
    """Every variant x mode x activation of one Operands, with the guard, launch-count and bit-relation assertions;
    check(variant, latency, act, got) holds each result to the caller's oracle.  split: the scratch splits this shape."""
    for latency in (False, True):
        with eng.latency_mode() if latency else contextlib.nullcontext():
            for act in (NONE, SIGMOID, RELU):
                v0 = ops.engine_call(eng, act)
                v0_nobias = ops.engine_call(eng, act, with_bias=False)
                assert not torch.isnan(v0).any() and not torch.isnan(v0_nobias).any()
                if latency:
                    assert same_bits(ops.engine_call(eng, act), v0), "V0 is not reproducible with the scratch on"
                check("V0", latency, act, v0)
                for v in ops.layouts:
                    got = ops.raw_call(eng, v, act)
                    base = v0_nobias if v == "V7" else v0
                    tag = "%s act %d latency %s" % (v, act, latency)
                    if not latency:
                        assert same_bits(got, base), tag + ": a one-pass route whose bits are not V0's"
                    else:
                        assert same_bits(ops.raw_call(eng, v, act), got), tag + ": not reproducible"
                        if v in KEEPS_ROUTE:
                            assert same_bits(got, base), tag + ": keeps V0's route but not its bits"
                    check(v, latency, act, got)
                if act == NONE:                                   # one pass against split, pinned by the bits (N(0, 1) operands)
                    if not latency:
                        plain = v0
                    elif split is not None:
                        assert same_bits(plain, v0) != split, "the scratch %s this shape" % ("no longer splits" if split else "now splits")


# ---- exact operands --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def exact_case(shape):
    """The host operands of a shape and their oracle, shared by the two layouts: (a, b, bias), then per bias / no bias the
    exact z, its extended-precision sigmoid and the sigmoid's bound, on the device."""
    m, n, k = shape
    a, b, bias = xo.draw(np.random.RandomState(m * 31 + n * 7 + k), m, n, k)
    oracle = {}
    for with_bias in (True, False):
        z = xo.product(a, b, bias if with_bias else None) + 0.0      # (+ 0.0: a host -0.0 -- a single product (-a) * 0 -- as the
        zd = dev(z)                                                   # +0.0 an accumulator that starts at +0.0 holds)
        oracle[with_bias] = (zd, dev(xo.sigmoid_ref(z)), pb.act_bound(SIGMOID, zd, torch.zeros_like(zd), fp64=True))
    return (a, b, bias), oracle


@pytest.mark.parametrize("lay", [KN, NK], ids=["kn", "nk"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "%dx%dx%d" % s)
def test_exact_operands_every_variant(eng, record_property, shape, lay):
    (a, b, bias), oracle = exact_case(shape)
    ops = Operands(a, b, bias, lay)
    worst = [0.0]

    def check(v, latency, act, got):
        z, sig, bound = oracle[v != "V7"]
        tag = "%s %s act %d latency %s" % (shape, v, act, latency)
        if act == NONE:
            assert same_bits(got, z), tag
        elif act == RELU:
            assert same_bits(got, z.clamp_min(0.0)), tag
        else:
            worst[0] = max(worst[0], pb.ratio(got - sig, bound))
            assert worst[0] <= 1.0, (tag, worst[0])

    # (exact operands give the same bits in any order: they cannot tell a split from one pass)
    sweep(eng, ops, check, split=None)
    record_property("sigmoid_worst_ratio", worst[0])
    report("exact %s %s: sigmoid, every variant and mode" % (shape, "KN" if lay == KN else "NK"), worst[0])


# ---- N(0, 1) operands, one shape per route ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def randn_case(shape):
    m, n, k = shape
    rng = np.random.RandomState(m + n * 3 + k * 5)
    a, b, bias = rng.standard_normal((m, k)), rng.standard_normal((k, n)) / np.sqrt(k), rng.standard_normal(n)
    ad, bd, biasd = dev(a), dev(b), dev(bias)
    abs_ab = ad.abs() @ bd.abs()
    oracle = {}
    for with_bias in (True, False):
        z = ad @ bd + (biasd if with_bias else 0.0)                # the reference: the fp64 product on the device
        oracle[with_bias] = (z, dev(xo.sigmoid_ref(z.cpu().numpy())), biasd if with_bias else None)
    return (a, b, bias), abs_ab, oracle


@pytest.mark.parametrize("lay", [KN, NK], ids=["kn", "nk"])
@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_randn_operands_within_the_summation_bound(eng, record_property, shape, lay):
    (a, b, bias), abs_ab, oracle = randn_case(shape)
    k, split = shape[2], SHAPES[shape]
    ops = Operands(a, b, bias, lay)
    worst = [0.0]

    def check(v, latency, act, got):
        z, sig, biasd = oracle[v != "V7"]
        chunks = SPLIT_CHUNKS if latency and split else 1
        bound = pb.act_bound(act, z, 2.0 * pb.gemm_dz(abs_ab, k, chunks, biasd, u=pb.U64), fp64=True)
        ref = z if act == NONE else (z.clamp_min(0.0) if act == RELU else sig)
        worst[0] = max(worst[0], pb.ratio(got - ref, bound))
        assert worst[0] <= 1.0, (shape, v, act, latency, worst[0])

    sweep(eng, ops, check, split=split)
    record_property("worst_ratio", worst[0])
    report("N(0, 1) %s %s: every variant, mode and activation" % (shape, "KN" if lay == KN else "NK"), worst[0])
