"""The SDAV training step (dlc_sdav_train_step, deeploopcloser_amd/csrc/train.hip) against the fp64 oracle
(oracle/sdav_train.py) on every route its products and reductions take -- at the widths, batches and modes SDAV.fit runs
and at the edges of each dispatch rule.

What is compared is the STEP, not the parameters after it: per tensor the GPU's change (after - before, both read back
from the device) against -lr * gradient from oracle.sdav_train.loss_and_grads,

    max |dGPU - dREF| <= 1e-9 * max |dREF|,

which holds a gradient to 1e-9 of its own size (a comparison of the updated parameters at 1e-9 of max |W| lets a
gradient that is off by a few per cent on its small entries through: one step moves a weight by 1e-3 .. 1e-1 of
its size).  {loss, cd, cs, cc} each within 1e-10 of the oracle's, and everything of the layers above the trained one
bit for bit as it was.

Routes, read from the dispatch code (plan_gemm / plan_dma_splitk / plan_split in gemm_dense.hip, plan_dma_forms /
plan_dma_launch in gemm_dma_f64.hip, weight_step in train.hip).  rows = batch x P.

 case | shape                                    | routes
 -----+------------------------------------------+---------------------------------------------------------------------
  A   | (1681, 2500 x 5), P 30, batch 10,        | layer 0 on the even pitch 1682: forward and dh = dz2 W through
      | layers 0..4, latency off / on            | gemm_bias_act_padded_f64 with Kb = 1681 < K = 1682 -- off: the LDS-DMA
      |                                          | kernel (64-row tiles); on: DMA split-K with the shorter B (5 chunks
      |                                          | of 352) + splitk_bias_act_kernel.  Decoder (h W^T, [N,K]) and dz1 W^T
      |                                          | on the LDS-DMA kernel (split-K when on).  Every layer's weight product
      |                                          | fused with its SGD step (gemm_axpy_dma_f64, K = 600 / 300).  Encoder
      |                                          | biases of layers 2 .. layer-1 through colsum_kernel (layers 3, 4).
  B   | (1681, 2499, 2499, 2499), layers 0, 2,   | odd N on [K,N] operands: the LDS-DMA kernel refuses the forward, dh and
      | latency off / on                         | every weight product -> register-staged gemm_bias_act_kernel (split by
      |                                          | plan_split into chunks + splitk_bias_act_kernel when on); odd K of the
      |                                          | decoder and dz1 W^T -> the same kernel; every weight gradient into the
      |                                          | workspace and stepped by update_kernel.
  C   | P 29, batch 9 (rows 261),                | the trained layer's product (K = 522) fused in the epilogue, layers 0 and
      | (1681, 2500, 2500, 2500), layer 2        | 1 (K = 261, odd) refused -> gradient into the workspace, update_kernel
  D   | batch 2, real widths, layer 0            | the smallest consecutive-frame term (one frame pair); 60 rows
  E   | P 2, batch 260, (64, 256, 256),          | the loss sum's second frame pass (batch > 256, update_kernel) and
      | layers 0, 1                              | hidden_grad_kernel's per-frame norms in LDS at that batch
  F   | P 120, batch 3, (64, 2500, 2500),        | frame_norm_kernel's slice count capped at FN_MAX_SLICES = 64
      | layer 1                                  | (P x N = 300 000 > 64 x 4096)
  G   | real widths, layer 1, batch 10,          | each loss term on its own: (sparse, consecutive) penalty (0, 0), (1, 0),
      | sparse level 0.1, lr 0.05                | (0, 0.2)
 ref  | real widths, N(0, 1) weights, layer 1    | the reference's initialisation, latency on

The paths users call -- SDAV.train_steps (one eager step, then HIP-graph replays, latency mode) and SDAV.fit (every layer,
epochs 3) -- are compared with consecutive oracle steps on the masks the network drew, redrawn here from the same
(seed, counter) pairs.
"""
import contextlib

import numpy as np
import pytest
import torch

from train_route_checks import assert_loss_parts, assert_step_delta    # (shared with test_gpu_da_train_routes.py)

pytestmark = pytest.mark.gpu

REAL = (1681,) + (2500,) * 5
DEFAULT_HP = dict(sparse_level=0.05, sparse_penalty=1.0, consecutive_penalty=0.2)


def problem(dims, patches, batch, seed, scale="fan_in"):
    """Frames in [0, 1), weights N(0, 1) / sqrt(fan_in) (or N(0, 1): the reference's), small random biases, one oracle mask
    per layer (corruption level 0.3)."""
    from oracle.tensor_ops import corruption_mask
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 1, size=(batch, patches, dims[0]))
    ws = [rng.standard_normal((a, b)) / (np.sqrt(a) if scale == "fan_in" else 1.0) for a, b in zip(dims[:-1], dims[1:])]
    bes = [rng.standard_normal(b) * 0.1 for b in dims[1:]]
    bds = [rng.standard_normal(a) * 0.1 for a in dims[:-1]]
    masks = [corruption_mask((patches, d), 0.3, rng) for d in dims[:-1]]
    return x, ws, bes, bds, masks


def check_engine_step(record_property, layer, dims, patches, batch, seed=0, latency=False, scale="fan_in", lr=0.1, **hp):
    """One Engine.sdav_train_step against oracle.sdav_train.loss_and_grads."""
    import deeploopcloser_amd as dlc
    from oracle import sdav_train as ot
    hp = dict(DEFAULT_HP, **hp)
    eng = dlc.default_engine()
    x, ws, bes, bds, masks = problem(dims, patches, batch, seed, scale)
    want, parts, g_ws, g_bes, g_bdec = ot.loss_and_grads(layer, x, masks, ws, bes, bds[layer], **hp)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    W, BE, BD, M = [dev(w) for w in ws], [dev(b) for b in bes], dev(bds[layer]), [dev(m) for m in masks]
    loss = torch.empty(4, dtype=torch.float64, device=eng.device)
    with eng.latency_mode() if latency else contextlib.nullcontext():
        eng.sdav_train_step(layer, dev(x.reshape(-1, dims[0])), batch, patches, M, W, BE, BD, hp["sparse_level"],
                            hp["sparse_penalty"], hp["consecutive_penalty"], lr, loss_out=loss)
        torch.cuda.synchronize()
    assert_loss_parts(loss.cpu().numpy(), (want,) + tuple(parts))
    worst = 0.0
    for l in range(len(ws)):
        w1, b1 = W[l].cpu().numpy(), BE[l].cpu().numpy()
        if l <= layer:
            worst = max(worst, assert_step_delta(ws[l], w1, -lr * g_ws[l], what="W[%d]" % l),
                        assert_step_delta(bes[l], b1, -lr * g_bes[l], what="b_enc[%d]" % l))
        else:
            assert np.array_equal(w1, ws[l]) and np.array_equal(b1, bes[l]), "layer %d above the trained one moved" % l
    worst = max(worst, assert_step_delta(bds[layer], BD.cpu().numpy(), -lr * g_bdec, what="b_dec[%d]" % layer))
    record_property("max_delta_ratio", worst)


@pytest.mark.parametrize("latency", [False, True], ids=["plain", "latency"])
@pytest.mark.parametrize("layer", [0, 1, 2, 3, 4])
def test_case_a_real_widths_batch10(record_property, layer, latency):
    check_engine_step(record_property, layer, REAL, 30, 10, seed=100 + layer, latency=latency)


@pytest.mark.parametrize("latency", [False, True], ids=["plain", "latency"])
@pytest.mark.parametrize("layer", [0, 2])
def test_case_b_odd_hidden_widths(record_property, layer, latency):
    check_engine_step(record_property, layer, (1681, 2499, 2499, 2499), 30, 10, seed=200 + layer, latency=latency)


@pytest.mark.parametrize("latency", [False, True], ids=["plain", "latency"])
def test_case_c_odd_rows_mixed_step(record_property, latency):
    check_engine_step(record_property, 2, (1681, 2500, 2500, 2500), 29, 9, seed=300, latency=latency)


@pytest.mark.parametrize("latency", [False, True], ids=["plain", "latency"])
def test_case_d_two_frames(record_property, latency):
    check_engine_step(record_property, 0, REAL, 30, 2, seed=400, latency=latency)


@pytest.mark.parametrize("layer", [0, 1])
def test_case_e_batch_above_256(record_property, layer):
    check_engine_step(record_property, layer, (64, 256, 256), 2, 260, seed=500 + layer)


def test_case_f_frame_norm_slice_cap(record_property):
    check_engine_step(record_property, 1, (64, 2500, 2500), 120, 3, seed=600)


@pytest.mark.parametrize("sparse_penalty,consecutive_penalty", [(0.0, 0.0), (1.0, 0.0), (0.0, 0.2)])
def test_case_g_one_loss_term_at_a_time(record_property, sparse_penalty, consecutive_penalty):
    check_engine_step(record_property, 1, REAL, 30, 10, seed=700, lr=0.05, sparse_level=0.1,
                      sparse_penalty=sparse_penalty, consecutive_penalty=consecutive_penalty)


def test_reference_initialisation(record_property):
    check_engine_step(record_property, 1, REAL, 30, 10, seed=800, latency=True, scale="reference")


# cc is a sum of distances between consecutive frames' codes.  A few steps of layer >= 2 saturate the sigmoids of the
# layers below (the reference's dynamics: one step moves W[1] by about its own size), the frames' codes then agree to
# 1e-10 .. 1e-13 and cc is the difference of nearly equal numbers: its rounding error is that of the codes themselves,
# a few eps times a frame's norm (<= sqrt(P x N) for codes in (0, 1)), not a few eps times cc.  1e-15 x sqrt(30 x 2500)
# = 2.7e-13 allows that and no more (measured: |dcc| <= 1.3e-17 at cc = 9.5e-13 .. 5.5e-10).
CC_FLOOR = 1e-15 * np.sqrt(30 * 2500)


# ---- the paths users call: SDAV.train_steps (eager step + graph replays) and SDAV.fit --------------------------------------
def redraw_masks(net, counter0, layers):
    """The masks SDAV._fill_mask drew for steps of the given layers, in its order (per step, l = 0 .. layer, the counter
    stepping by one), redrawn from the network's (seed, counter) pairs.  Returns them and the number of draws."""
    eng, c, out = net.engine, counter0, []
    for layer in layers:
        ms = []
        for l in range(layer + 1):
            p, k = net.get_layer_input_shape(l)
            m = torch.empty((p, k), dtype=torch.float64, device=eng.device)
            eng.random_mask(m, int(np.round(p * k * float(net.corruption_level))), net._mask_seed, c)
            c += 1
            ms.append(m.cpu().numpy())
        out.append(ms)
    return out, c - counter0


def oracle_steps(net, x, layers, masks, ws, bes, bds):
    """Consecutive oracle SGD steps with the network's hyper-parameters; returns the parameters after them and the loss
    parts of the last step (before its update)."""
    from oracle import sdav_train as ot
    hp = dict(sparse_level=net.sparse_level, sparse_penalty=net.sparse_penalty, consecutive_penalty=net.consecutive_penalty)
    lr, ws, bes, bds = net.learning_rate, list(ws), list(bes), list(bds)
    parts = None
    for layer, ms in zip(layers, masks):
        loss, p3, g_ws, g_bes, g_bdec = ot.loss_and_grads(layer, x, ms, ws, bes, bds[layer], **hp)
        parts = (loss,) + tuple(p3)
        for l in range(layer + 1):
            ws[l] = ws[l] - lr * g_ws[l]
            bes[l] = bes[l] - lr * g_bes[l]
        bds[layer] = bds[layer] - lr * g_bdec
    return ws, bes, bds, parts


def params(net):
    ws, bs = net.get_weights()
    return ws, bs, [b.cpu().numpy() for b in net._biases_dec]


def assert_same_run(record_property, net, layers, before, after, ref, bound=1e-9):
    """Every tensor some step reached moved as the oracle's steps moved it; the others are bit for bit as they were."""
    top = max(layers)
    worst = 0.0
    for kind, b, a, r in zip(("W", "b_enc", "b_dec"), before, after, ref):
        for l in range(len(b)):
            reached = l in layers if kind == "b_dec" else l <= top
            if reached:
                worst = max(worst, assert_step_delta(b[l], a[l], r[l] - b[l], bound, what="%s[%d]" % (kind, l)))
            else:
                assert np.array_equal(a[l], b[l]), "%s[%d] moved, no step reaches it" % (kind, l)
    record_property("max_delta_ratio", worst)


@pytest.mark.parametrize("layer", [0, 2, 4])
def test_train_steps_replayed_vs_oracle(record_property, layer):
    """SDAV.train_steps(layer, x, 4) in latency mode: one eager step, the capture, three replays (with the masks of the
    next step drawn beside the running one) == four consecutive oracle steps on the same masks."""
    import deeploopcloser_amd as dlc
    n = 4
    rng = np.random.RandomState(900 + layer)
    x = rng.uniform(0, 1, size=(10, 30, 1681))
    net = dlc.SDAV(seed=21 + layer, weight_scale="fan_in")
    before = params(net)
    c0, step0 = net._mask_counter, net.global_step
    with net.engine.latency_mode():
        loss = net.train_steps(layer, x, n).cpu().numpy()
    torch.cuda.synchronize()
    after = params(net)
    assert net.global_step == step0 + n
    masks, draws = redraw_masks(net, c0, [layer] * n)
    assert draws == net._mask_counter - c0, "SDAV draws its masks in another order than this test rebuilds them"
    ws, bes, bds, parts = oracle_steps(net, x, [layer] * n, masks, *before)
    assert_loss_parts(loss, parts, cc_floor=CC_FLOOR)
    assert_same_run(record_property, net, [layer], before, after, (ws, bes, bds))


def test_fit_vs_oracle(record_property):
    """SDAV.fit (the reference's train.py path): epochs 3 on one batch of 10 frames, layer by layer -- 15 steps, each
    layer's three as one eager step and two graph replays in latency mode -- == the oracle's 15 steps on the same masks."""
    import deeploopcloser_amd as dlc
    rng = np.random.RandomState(950)
    x = rng.uniform(0, 1, size=(10, 30, 1681))
    net = dlc.SDAV(seed=31, weight_scale="fan_in")
    net.epochs = 3
    before = params(net)
    c0 = net._mask_counter
    net.fit(x)
    torch.cuda.synchronize()
    after = params(net)
    layers = [l for l in range(len(net.hidden_units)) for _ in range(net.epochs)]
    assert net.global_step == len(layers)
    masks, draws = redraw_masks(net, c0, layers)
    assert draws == net._mask_counter - c0, "SDAV draws its masks in another order than this test rebuilds them"
    ws, bes, bds, _ = oracle_steps(net, x, layers, masks, *before)
    assert_same_run(record_property, net, sorted(set(layers)), before, after, (ws, bes, bds))
