"""The DA training step (dlc_da_train_step, deeploopcloser_amd/csrc/train.hip; the DA / SDA classes and the train_sdav
command) against the fp64 oracle (tests/da_oracle.py) on every route its products and reductions take -- at the widths an
SDA stacks, in the latency mode every fit runs in, and at the edges of each dispatch rule.  The SDAV step has the same
treatment in test_gpu_train_routes.py; the checks are shared (train_route_checks.py).

What is compared is the STEP, not the parameters after it: for W, b_enc and b_dec the GPU's change (after - before, both
read back from the device) against -lr * gradient from da_oracle.loss_and_grads,

    max |dGPU - dREF| <= 1e-9 * max |dREF|        per tensor,

and {loss, cd, cs, cc} each within 1e-10 of the oracle's.  (A comparison of the updated parameters at 1e-9 of max |W|
holds a gradient only as tightly as one step moves the weights: with N(0, 1) weights an entry may be off by 1e-5 of its
size and pass.)  The step is driven through Engine.da_corrupt + Engine.da_train_step with masks built in NumPy -- exactly
int(rows * K * 0.3) zeros, salt on a seeded random half of them -- so that it does not depend on the mask generator; x~
is first compared bit for bit with zeros * x + ones.

What exists only on the DA side of train_step_impl: x~ is the caller's and holds salt (x~ = 1 where x is not), the
encoder and the x~^T dz1 half of the tied gradient read x~ while the cross entropy's labels are the clean x at another
pitch (K against even_pitch(K)); and cs_den = batch * patches where SDAV's layer 0 has batch * N.

Routes, read from the dispatch code (plan_gemm / plan_dma_splitk / plan_split in gemm_dense.hip, plan_dma_forms /
plan_dma_launch in gemm_dma_f64.hip, weight_step in train.hip).  rows = batch x P, Kp = even_pitch(K).  A step has four
products: fwd = x~ W ([rows, Kp] x [K, N], the shorter B when K is odd), dec = h W^T ([N, K] operand), dh = dz2 W (as
fwd) and dW = [dz2^T | x~^T] . [h ; dz1] ([K, 2 rows] x [2 rows, N]).  "DMA" is the LDS-DMA kernel on 64-row tiles
unless noted, "staged" the register-staged kernel; "fused" = dW stepped in the product's epilogue (gemm_axpy_dma_f64),
"ws" = dW into the workspace, stepped by update_kernel.  plain -> latency:

 case | (batch, P, K, N)       | routes
 -----+------------------------+------------------------------------------------------------------------------------
  A   | (10, 30, 1681, 2500)   | the first DA of the default stack; pad column (Kp = 1682, Kb = 1681).  fwd, dh: DMA ->
      |                        | DMA split-K with the shorter B, 5 chunks of 352; dec: DMA -> DMA split-K, 7 x 368;
      |                        | dW (K = 600): fused, both modes
  B   | (10, 30, 2500, 2500)   | every later DA of the stack; even K: no pad, labels pitch == x~ pitch.  fwd, dec, dh:
      |                        | DMA -> DMA split-K 5 x 512; dW: fused (256-row tiles)
  C   | (10, 30, 1681, 2499),  | odd N on the [K, N] operands, odd K on the [N, K] one: the LDS-DMA kernel refuses all
      | (10, 30, 2499, 2499)   | four products.  fwd, dec, dh: staged -> staged split by plan_split (4 / 5 / 4 chunks;
      |                        | 4 / 4 / 4) + splitk_bias_act_kernel; dW: ws + update_kernel, staged in one pass
  D   | (9, 29, 1681, 2500)    | odd rows (261): as A, the fused dW with K = 522
  E   | (2, 30, 1681, 2500)    | one frame pair, 60 rows: as A with 12 x 144 (fwd, dh) and 18 x 144 (dec) chunks
  F   | (260, 2, 64, 256)      | batch > 256: update_kernel's second frame pass, hidden_grad_kernel's 259 norms in LDS.
      |                        | fwd, dh: DMA (K = 64, the 4 x TK3 floor), no split; dec (N = 64 <= 96, 3 tiles of 256
      |                        | rows < 16): staged -> staged split-K 2; dW (K = 1040): fused
  G   | (3, 120, 64, 2500)     | frame_norm_kernel's slice count capped at FN_MAX_SLICES (P x N = 300 000 > 64 x 4096).
      |                        | fwd, dh: DMA; dec: staged -> staged split-K 16; dW (K = 720): fused
  H1  | (10, 30, 2500, 64)     | N <= 96 with few tiles: the 96-column form wants 16 tiles of 256 rows and refuses.
      |                        | fwd, dh: staged -> staged split-K 16; dec (K = 64): DMA; dW: ws, staged -> split-K 4
  H2  | (10, 30, 64, 32)       | dec has K = 32, below the LDS-DMA kernel's floor: everything staged, ws; latency
      |                        | splits dW alone (K = 600, 4 chunks)
  H3  | (4, 5, 37, 21)         | tiny, odd everywhere: staged, ws; plan_split declines (K steps < 16): latency == plain
  H4  | (2, 1, 2, 1)           | degenerate: one patch, one unit, two frames; as H3 (P == N: the one case that cannot
      |                        | tell cs_den = batch * patches from batch * N)
  H5  | (137, 30, 64, 64)      | N <= 96 with 4110 rows: fwd, dec, dh on the 96-column form of the LDS-DMA kernel
      |                        | (17 tiles of 256 rows); dW (64 x 64, K = 8220): ws, staged -> staged split-K
  I   | A's shape, lr 0.05,    | each loss term alone: (sparse, consecutive) penalty (0, 0), (1, 0), (0, 0.2); a wrong
      | sparse level 0.1       | cs_den shows in cs, and in the gradient of (1, 0) relative to the cross entropy's
 ref  | A and B, N(0, 1)       | the reference's initialisation (latency mode only)

The ring of Engine.set_profiling counts launches of product kernels, not the split-K reduce, and gives no kernel's name:
every case must record exactly four (a two-part LDS-DMA plan, or a tied gradient taken as two products, would be five).
Split against one pass is pinned by the bits instead: a step is deterministic (fixed summation orders), a one-pass
product gives the same bits in both modes and a split one sums in another order, so each latency case also runs the
plain step and asserts that W differs (A .. H2, H5, I, ref) or is bit for bit the same (H3, H4).  A later change of a
dispatch rule that merges two cases fails there.

The paths users call -- DA.train_steps (one eager step, the capture, replays, a re-capture after a new learning rate) and
SDA.fit_dataset (greedy, two layers of 2500) -- are compared with consecutive oracle steps on the masks the objects drew.

Preconditions, asserted on the oracle's values before the GPU is consulted (a near-tie would make the comparison
meaningless, not hide a bug): min |h - sparse_level| > 1e-9 (sign(h - s) is discontinuous), every consecutive-frame norm
> 0, max |dREF| > 0 per tensor (step_delta_ratio).  The seeds below were picked on the CPU so that all three hold.

Measured on an MI355X (max_delta_ratio, against the bound 1e-9): single steps 3.6e-15 .. 1.3e-14 (A .. H5), 1.5e-14 ..
3.6e-14 (I), 1.7e-13 and 1.9e-13 (ref A, B); train_steps 9.8e-14 / 1.2e-13 over the first four steps and 2.6e-13 /
2.8e-13 over the three after the new learning rate (A / B); SDA.fit_dataset 1.3e-13 (layer 0) and 1.4e-13 (layer 1, the
GPU's own layer 0 underneath: nothing of layer 0's difference shows).  The file runs in 7 s.
"""
import contextlib
import functools
import logging
import os

import numpy as np
import pytest
import torch

import da_oracle as od
from conftest import GOLDEN
from train_route_checks import assert_loss_parts, assert_step_delta

pytestmark = pytest.mark.gpu

DEFAULT_HP = dict(sparse_level=0.05, sparse_penalty=1.0, consecutive_penalty=0.2)
A_SHAPE, B_SHAPE = (10, 30, 1681, 2500), (10, 30, 2500, 2500)

# name -> (batch, P, K, N), seed, whether latency mode changes a summation order (see the table)
SHAPES = {
    "A": (A_SHAPE, 1100, True),
    "B": (B_SHAPE, 1200, True),
    "C-1681x2499": ((10, 30, 1681, 2499), 1300, True),
    "C-2499x2499": ((10, 30, 2499, 2499), 1301, True),
    "D": ((9, 29, 1681, 2500), 1400, True),
    "E": ((2, 30, 1681, 2500), 1500, True),
    "F": ((260, 2, 64, 256), 1600, True),
    "G": ((3, 120, 64, 2500), 1700, True),
    "H1-2500x64": ((10, 30, 2500, 64), 1800, True),
    "H2-64x32": ((10, 30, 64, 32), 1801, True),
    "H3-37x21": ((4, 5, 37, 21), 1802, False),
    "H4-2x1": ((2, 1, 2, 1), 1803, False),
    "H5-96col": ((137, 30, 64, 64), 1804, True),
}
PRODUCT_LAUNCHES = 4        # fwd, dec, dh, dW: one product kernel each on every route of the table


def np_masks(rng, rows, k, level=0.3):
    """(zeros, ones) [rows, k] as the reference draws them, in NumPy: exactly int(rows * k * level) zeros, every
    placement equally likely, and salt on a random half of them (rounded up: the one zero of the 2 x 2 case is salted)."""
    n = rows * k
    nz = int(n * level)
    at = rng.permutation(n)[:nz]
    zeros, ones = np.ones(n), np.zeros(n)
    zeros[at] = 0.0
    ones[at[:(nz + 1) // 2]] = 1.0
    return zeros.reshape(rows, k), ones.reshape(rows, k)


def problem(shape, seed, scale="fan_in"):
    """Frames in [0, 1), W N(0, 1) / sqrt(K) (or N(0, 1): the reference's), small random biases, NumPy masks."""
    batch, p, k, n = shape
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 1, size=(batch, p, k))
    w = rng.standard_normal((k, n)) / (np.sqrt(k) if scale == "fan_in" else 1.0)
    b0, b1 = rng.standard_normal(n) * 0.1, rng.standard_normal(k) * 0.1
    zeros, ones = np_masks(rng, batch * p, k)
    assert int((zeros == 0).sum()) == int(batch * p * k * 0.3) and np.all(ones <= 1 - zeros) and ones.sum() > 0
    return x, zeros, ones, w, b0, b1


def assert_preconditions(x, zeros, ones, w, b0, sparse_level):
    """No h within 1e-9 of the sparsity level, no two consecutive frames with the same code.  -> (gap, smallest norm)."""
    batch, p, k = x.shape
    h = od.sigmoid(od.corrupt(x.reshape(batch * p, k), zeros, ones) @ w + b0)
    gap = float(np.abs(h - sparse_level).min())
    hb = h.reshape(batch, -1)
    nrm = float(np.sqrt(((hb[:-1] - hb[1:]) ** 2).sum(axis=1)).min())
    assert gap > 1e-9, "an h within %.3g of the sparsity level: sign(h - s) is not defined well enough to compare" % gap
    assert nrm > 0.0, "two consecutive frames with the same code: the consecutive-frame gradient is 0 / 0"
    return gap, nrm


@functools.lru_cache(maxsize=2)
def oracle_case(shape, seed, scale, hp_items):
    """A case's problem and its oracle step, computed once per case and shared by its plain and latency runs."""
    hp = dict(hp_items)
    prob = problem(shape, seed, scale)
    x, zeros, ones, w, b0, b1 = prob
    assert_preconditions(x, zeros, ones, w, b0, hp["sparse_level"])
    parts, grads = od.loss_and_grads(x, zeros, ones, w, b0, b1, **hp)
    return prob, parts, grads


def gpu_step(eng, prob, lr, hp, latency, count_launches=False):
    """One Engine.da_corrupt + Engine.da_train_step on fresh device copies.  -> (loss[4], W, b_enc, b_dec) read back, and
    the number of product-kernel launches the step recorded when asked to count them."""
    x, zeros, ones, w, b0, b1 = prob
    batch, p, k = x.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    x2 = dev(x.reshape(batch * p, k))
    xt = eng.da_corrupt(x2, dev(zeros), dev(ones))
    want_xt = np.zeros((batch * p, eng.even_pitch(k)))
    want_xt[:, :k] = od.corrupt(x.reshape(batch * p, k), zeros, ones)
    assert np.array_equal(xt.cpu().numpy(), want_xt), "x~ is not zeros * x + ones with a zero pad column"
    W, BE, BD = dev(w), dev(b0), dev(b1)
    loss = torch.full((4,), float("nan"), dtype=torch.float64, device=eng.device)
    launches = None
    with eng.latency_mode() if latency else contextlib.nullcontext():
        if count_launches:
            eng.set_profiling(True)
        try:
            eng.da_train_step(x2, xt, batch, p, W, BE, BD, hp["sparse_level"], hp["sparse_penalty"],
                              hp["consecutive_penalty"], lr, loss_out=loss)
            if count_launches:
                ms = eng.profile_gemm_ms()
                assert all(t > 0 for t in ms), ms
                launches = len(ms)
        finally:
            if count_launches:
                eng.set_profiling(False)
        torch.cuda.synchronize()
    assert np.array_equal(x2.cpu().numpy(), x.reshape(batch * p, k)), "the step wrote into its clean batch"
    assert np.array_equal(xt.cpu().numpy(), want_xt), "the step wrote into x~"
    return loss.cpu().numpy(), W.cpu().numpy(), BE.cpu().numpy(), BD.cpu().numpy(), launches


def check_engine_step(record_property, shape, seed, latency, splits, scale="fan_in", lr=0.1, **hp):
    """One DA step against da_oracle.loss_and_grads; in latency mode also against the plain step's bits."""
    import deeploopcloser_amd as dlc
    hp = dict(DEFAULT_HP, **hp)
    (prob, parts, (g_w, g_b0, g_b1)) = oracle_case(shape, seed, scale, tuple(sorted(hp.items())))
    x, zeros, ones, w, b0, b1 = prob
    eng = dlc.default_engine()
    loss, w1, be1, bd1, launches = gpu_step(eng, prob, lr, hp, latency, count_launches=True)
    assert launches == PRODUCT_LAUNCHES, "%d product launches: this case no longer takes the route its row names" % launches
    assert_loss_parts(loss, parts)
    worst = max(assert_step_delta(w, w1, -lr * g_w, what="W"),
                assert_step_delta(b0, be1, -lr * g_b0, what="b_enc"),
                assert_step_delta(b1, bd1, -lr * g_b1, what="b_dec"))
    record_property("max_delta_ratio", worst)
    print("max_delta_ratio %.3g" % worst)
    if latency:
        _, w_plain, _, _, _ = gpu_step(eng, prob, lr, hp, False)
        if splits:
            assert not np.array_equal(w_plain, w1), "latency mode no longer splits any product of this case"
        else:
            assert np.array_equal(w_plain, w1), "latency mode now splits a product of this case"
    return parts


MODES = pytest.mark.parametrize("latency", [False, True], ids=["plain", "latency"])


@MODES
@pytest.mark.parametrize("case", list(SHAPES))
def test_case_shapes(record_property, case, latency):
    shape, seed, splits = SHAPES[case]
    check_engine_step(record_property, shape, seed, latency, splits)


@MODES
@pytest.mark.parametrize("sparse_penalty,consecutive_penalty", [(0.0, 0.0), (1.0, 0.0), (0.0, 0.2)])
def test_case_i_one_loss_term_at_a_time(record_property, sparse_penalty, consecutive_penalty, latency):
    parts = check_engine_step(record_property, A_SHAPE, 1900, latency, True, lr=0.05, sparse_level=0.1,
                              sparse_penalty=sparse_penalty, consecutive_penalty=consecutive_penalty)
    if sparse_penalty == 0.0 and consecutive_penalty == 0.0:
        # the oracle's cs (mean over batch * patches rows) is not what SDAV's layer-0 denominator (batch * N) gives: the
        # 1e-10 on cs above tells the two apart
        batch, p, _, n = A_SHAPE
        cs = parts[2]
        cs_sdav = cs * (batch * p) / (batch * n)
        assert abs(cs_sdav - cs) > 1e-3 * abs(cs)


@pytest.mark.parametrize("case", ["A", "B"])
def test_reference_initialisation(record_property, case):
    shape, seed, _ = SHAPES[case]
    check_engine_step(record_property, shape, seed + 50, True, True, scale="reference")


# ---- the paths users call: DA.train_steps (eager step + graph replays) and SDA.fit_dataset ---------------------------------
def cc_floor(p, n):
    """cc is a sum of distances between consecutive frames' codes; where steps have saturated the sigmoids the codes agree
    to many digits and cc is the difference of nearly equal numbers: its rounding error is that of the codes, a few eps
    times a frame's norm (<= sqrt(P x N) for codes in (0, 1)), not a few eps times cc (CC_FLOOR of
    test_gpu_train_routes.py, for this P x N)."""
    return 1e-15 * np.sqrt(p * n)


def oracle_steps(x, zeros, ones, w, b0, b1, n, lr, hp):
    """n consecutive da_oracle.sgd_step, the preconditions asserted before each.  -> the parameters after them and the
    loss parts of the last step (before its update)."""
    parts = None
    for _ in range(n):
        assert_preconditions(x, zeros, ones, w, b0, hp["sparse_level"])
        parts, (w, b0, b1) = od.sgd_step(x, zeros, ones, w, b0, b1, lr=lr, **hp)
    return (w, b0, b1), parts


def assert_same_run(record_property, before, after, ref_before, ref_after, bound=1e-9, name="max_delta_ratio"):
    """W, b_enc, b_dec moved over a run of steps as the oracle's steps moved them: the run's delta within `bound` of the
    oracle's largest delta, per tensor."""
    worst = max(assert_step_delta(b, a, r1 - r0, bound, what=what)
                for what, b, a, r0, r1 in zip(("W", "b_enc", "b_dec"), before, after, ref_before, ref_after))
    record_property(name, worst)
    print("%s %.3g" % (name, worst))
    return worst


@pytest.mark.parametrize("case", ["A", "B"])
def test_train_steps_replayed_vs_oracle(record_property, case):
    """DA.train_steps(x, 4) in latency mode (what DA._fit_batches runs): one eager step, the capture and three replays ==
    four consecutive oracle steps on the masks the DA drew; then, after a new learning rate, three more (train_steps
    captures from three steps on: an eager step, the re-capture, two replays) == the oracle's next three."""
    import deeploopcloser_amd as dlc
    batch, p, k, n = SHAPES[case][0]
    x = np.random.RandomState(2000 + k).uniform(0, 1, size=(batch, p, k))
    da = dlc.DA([p, k], n, batch_size=batch, seed=40 + (k & 1))
    hp = dict(sparse_level=da.sparse_level, sparse_penalty=da.sparse_penalty, consecutive_penalty=da.consecutive_penalty)
    zeros, ones = (m.cpu().numpy() for m in da.corruption_masks())
    assert zeros.shape == (batch * p, k) and int((zeros == 0).sum()) == int(batch * p * k * 0.3)
    before = da.get_weights()
    with da.engine.latency_mode():
        loss = da.train_steps(x, 4).cpu().numpy()
    torch.cuda.synchronize()
    after = da.get_weights()
    assert da.global_step == 4
    ref, parts = oracle_steps(x, zeros, ones, *before, 4, da.learning_rate, hp)
    assert_loss_parts(loss, parts, cc_floor=cc_floor(p, n))
    assert_same_run(record_property, before, after, before, ref)

    da.learning_rate = 0.05
    with da.engine.latency_mode():
        loss = da.train_steps(x, 3).cpu().numpy()
    torch.cuda.synchronize()
    assert da.global_step == 7
    ref2, parts = oracle_steps(x, zeros, ones, *ref, 3, 0.05, hp)
    assert_loss_parts(loss, parts, cc_floor=cc_floor(p, n))
    # (the second run's delta, from the GPU's own parameters after step 4, against the oracle's second run)
    assert_same_run(record_property, after, da.get_weights(), ref, ref2, name="max_delta_ratio_after_new_learning_rate")
    for m, m1 in zip((zeros, ones), da.corruption_masks()):
        assert np.array_equal(m, m1.cpu().numpy())              # the static masks are left as drawn


def test_sda_fit_vs_oracle_chain(record_property, caplog):
    """SDA([30, 1681], [2500, 2500], batch_size=10, epochs=3).fit_dataset on the 17 frames of the test dataset: one batch
    of 10 (the 7 left over are ignored with the reference's warning), three steps a layer, == the oracle chain: layer 0 is
    da_oracle.fit_batches, layer 1 is fit_batches on sigmoid(x W0 + b0) of the ORACLE's trained layer 0 -- so layer 1 is
    held to the chain, the GPU's own layer 0 included, not to another GPU run.  Both layers at the run-delta bound 1e-9."""
    import deeploopcloser_amd as dlc
    from deeploopcloser_amd.input import load_frames
    frames = load_frames(os.path.join(GOLDEN, "datasets_test", "*.ppm"), [30, 1681])
    assert len(frames) == 17
    sda = dlc.SDA([30, 1681], [2500, 2500], batch_size=10, epochs=3)
    hp = dict(sparse_level=sda.sparse_level, sparse_penalty=float(sda.sparse_penalty),
              consecutive_penalty=sda.consecutive_penalty)
    before = sda.get_weights()
    masks = [tuple(m.cpu().numpy() for m in layer.corruption_masks()) for layer in sda.layers]
    with caplog.at_level(logging.WARNING):
        sda.fit_dataset(frames)
    torch.cuda.synchronize()
    assert [l.global_step for l in sda.layers] == [3, 3]
    assert sum("Ignored last batch" in r.getMessage() for r in caplog.records) == 2       # once a layer
    after = sda.get_weights()

    batches = [np.stack(frames[i:i + 10]) for i in range(0, 17, 10)]
    ref = []
    for i in range(2):
        w, b0, b1, steps = od.fit_batches(batches, *masks[i], *before[i], 3, lr=sda.learning_rate, **hp)
        assert steps == 3
        checked, _ = oracle_steps(batches[0], *masks[i], *before[i], 3, sda.learning_rate, hp)
        assert all(np.array_equal(u, v) for u, v in zip(checked, (w, b0, b1)))       # (the same steps, preconditions checked)
        ref.append((w, b0, b1))
        batches = [od.sigmoid(b.reshape(-1, b.shape[2]) @ w + b0).reshape(b.shape[0], b.shape[1], -1) for b in batches]
    for i in range(2):
        assert_same_run(record_property, before[i], after[i], before[i], ref[i], name="max_delta_ratio_layer%d" % i)
