"""GPU multi-descriptor fusion (dlc_fuse_rows, Engine.fuse_rows, fusion.fuse_scores, FusedLoopClosureDetector and the
CLI's --fuse) against the NumPy restatement of the definition (tests/fusion_oracle.py, pinned by test_fusion_cpu.py).
The definition fixes every rounding, so every comparison is by bit pattern -- zero tolerance -- any NaN equal to any NaN
by position (sequence_oracle.same_bits)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import chains_oracle as cho
import contrast_oracle as co
import elastic_oracle as eo
import fusion_oracle as fo
import peaks_oracle as po
import sequence_oracle as so

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
SHAPES = [(1, 1), (3, 2), (5, 63), (4, 64), (3, 65), (5, 255), (2, 256), (3, 257), (7, 1000), (2, 4095), (2, 4096), (2, 4097),
          (1, 8193), (2, 70001)]
NORM_IDS = {"none": 0, "zscore": 1, "minmax": 2}
AUTO, ROW, SLAB = 0, 1, 2


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def member(rng, i, rows, n):
    """Source i of a call: the dtypes in turn -- fp64 with a scale per row, fp32, int64 with values beyond 2^53."""
    if i % 3 == 0:
        return rng.standard_normal((rows, n)) * 10.0 ** rng.randint(-3, 4, size=(rows, 1))
    if i % 3 == 1:
        return rng.standard_normal((rows, n)).astype(np.float32)
    return rng.randint(-(1 << 62), 1 << 62, size=(rows, n), dtype=np.int64)


def on_device(e, m, ld):
    """m [rows, n] as the first n columns of a [rows, ld] device view whose rows start at an ODD element of their
    allocation; the padding holds a sentinel that would change every statistic if it were read."""
    rows, n = m.shape
    dt = torch.from_numpy(m[:1, :1]).dtype
    flat = torch.empty(rows * ld + 1, dtype=dt, device=e.device)
    buf = flat[1:].view(rows, ld)
    buf.fill_((1 << 62) if dt == torch.int64 else 1e30)
    buf[:, :n] = torch.from_numpy(m).to(e.device)
    return buf


def sentinel_out(e, rows, ld_out):
    return torch.full((rows, ld_out), SENTINEL, dtype=torch.int64, device=e.device).view(torch.float64)


def call(e, bufs, n, weights, lib, norm, plan, out, limit0=None, step=0, ws=None, rows=None, lds=None, dtypes=None):
    """The C entry point itself -> its status."""
    m = len(bufs)
    rows = bufs[0].shape[0] if rows is None else rows
    lds = [b.stride(0) for b in bufs] if lds is None else lds
    dtypes = [e._SEQ_DTYPES[b.dtype] for b in bufs] if dtypes is None else dtypes
    return e.lib.dlc_fuse_rows(
        e.ctx, m, (C.c_int * m)(*dtypes), (C.c_void_p * m)(*[b.data_ptr() for b in bufs]), (C.c_int64 * m)(*lds),
        (C.c_double * m)(*weights), (C.c_int * m)(*[int(v) for v in lib]), rows, n, n if limit0 is None else limit0, step,
        NORM_IDS[norm], plan, C.c_void_p(out.data_ptr()), out.stride(0), C.c_void_p(ws.data_ptr()) if ws is not None else None,
        ws.numel() if ws is not None else 0, None)


def words(e, bufs, n, weights, lib, norm, plan, limit0=None, step=0, with_ws=True):
    """One call into a sentinel-filled [rows, n + 3] buffer -> the whole buffer as int64 words."""
    rows = bufs[0].shape[0]
    out = sentinel_out(e, rows, n + 3)
    ws = None
    if with_ws:
        need = e.lib.dlc_fuse_rows_workspace_bytes(rows, n, len(bufs))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=e.device)
    assert call(e, bufs, n, weights, lib, norm, plan, out, limit0, step, ws) == 0, e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    return out.view(torch.int64).cpu().numpy()


def same_words(got, want_f64, ld_out):
    """got: int64 words [rows, ld_out]; want_f64 [rows, n] with NaN where a cell is not offered or its value is NaN: the
    offered non-NaN cells by bit pattern, NaN by position, the sentinel everywhere else."""
    rows, n = want_f64.shape
    if not (got[:, n:] == SENTINEL).all():
        return False
    return so.same_bits(got[:, :n].copy().view(np.float64), want_f64)


def sentinel_where(want, lim):
    """The oracle's result with the sentinel's bits in the cells that are not offered."""
    want = want.copy()
    want.view(np.int64)[np.arange(want.shape[1])[None, :] >= lim[:, None]] = SENTINEL
    return want


# ---- bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n", SHAPES)
def test_bits(dlc, rows, n):
    """Every plan, with and without a workspace, equals the oracle and so each other.  Forced SLAB at 4095 / 4096 / 4097
    and at 70001 (18 slabs, not a power of two) is where the slab tree can go wrong; 63 / 64 / 65 and 255 / 256 / 257 are
    where the lane and the chunk trees can."""
    e = dlc.default_engine()
    rng = np.random.RandomState(rows * 100003 + n)
    for m in (1, 2, 3, 8):
        mats = [member(rng, i, rows, n) for i in range(m)]
        bufs = [on_device(e, a, n + 3 + i) for i, a in enumerate(mats)]
        weights = [1.0, -0.75, 2.5, 0.3, 1.0, -1.0, 0.125, 3.0][:m]
        lib = [bool(i & 1) for i in range(m)]
        lim = so.limits(rows, n, n, 0)
        for norm in fo.NORMS:
            want = sentinel_where(fo.fuse_rows(mats, weights, lib, norm), lim)
            for plan, with_ws in ((ROW, False), (ROW, True), (SLAB, True), (AUTO, True), (AUTO, False)):
                got = words(e, bufs, n, weights, lib, norm, plan, with_ws=with_ws)
                assert same_words(got, want, n + 3), (m, norm, plan, with_ws)


def test_one_source_without_a_norm_is_a_conversion_copy(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(1)
    for i in range(3):
        a = member(rng, i, 3, 333)
        got = e.fuse_rows([on_device(e, a, 340)], norm="none", n=333)
        assert so.same_bits(got.cpu().numpy(), a.astype(np.float64))


def test_zscore_negation_with_the_flag_leaves_the_bits(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(2)
    a, b = member(rng, 0, 4, 500), member(rng, 1, 4, 500)
    for plan in ("row", "slab"):
        one = e.fuse_rows([on_device(e, a, 503), on_device(e, b, 504)], [1.0, -0.5], [False, True], n=500, plan=plan)
        two = e.fuse_rows([on_device(e, -a, 503), on_device(e, -b, 504)], [1.0, -0.5], [True, False], n=500, plan=plan)
        assert so.same_bits(one.cpu().numpy(), two.cpu().numpy())


# ---- limits, and what is left alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit0,step", [(-4, 1), (0, 1), (292, 1), (7, 0), (308, -2), (0, 0)])
def test_limits_and_what_is_left_alone(dlc, limit0, step):
    e = dlc.default_engine()
    rows, n = 12, 300
    rng = np.random.RandomState(abs(limit0) * 7 + step + 2)
    mats = [member(rng, i, rows, n) for i in range(3)]
    bufs = [on_device(e, a, n + 3 + i) for i, a in enumerate(mats)]
    weights, lib = [1.0, -2.0, 0.5], [False, True, True]
    lim = so.limits(rows, n, limit0, step)
    for norm in fo.NORMS:
        want = sentinel_where(fo.fuse_rows(mats, weights, lib, norm, limit0=limit0, limit_step=step), lim)
        for plan in (ROW, SLAB, AUTO):
            got = words(e, bufs, n, weights, lib, norm, plan, limit0, step)
            assert same_words(got, want, n + 3), (norm, plan)
            if not lim.any():
                assert (got == SENTINEL).all()


# ---- a row does not depend on its batch ------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_batch(dlc):
    e = dlc.default_engine()
    rows, n = 6, 4500
    rng = np.random.RandomState(9)
    mats = [member(rng, i, rows, n) for i in range(3)]
    weights, lib = [1.0, 1.0, -0.5], [False, True, False]
    for norm in fo.NORMS:
        for plan in (ROW, SLAB):
            whole = words(e, [on_device(e, a, n + 3 + i) for i, a in enumerate(mats)], n, weights, lib, norm, plan, 4000, 100)
            for size in (1, 2):
                parts = [words(e, [on_device(e, a[lo:lo + size], n + 5 + i) for i, a in enumerate(mats)], n, weights, lib, norm,
                               plan, 4000 + 100 * lo, 100) for lo in range(0, rows, size)]
                assert np.array_equal(np.concatenate(parts), whole), (norm, plan, size)


# ---- special values --------------------------------------------------------------------------------------------------------------
def test_special_values(dlc):
    e = dlc.default_engine()
    n = 70
    base = np.random.RandomState(4).standard_normal((8, n))
    x = base.copy()
    x[0, 5] = np.inf
    x[1, 6] = -np.inf
    x[2, 7] = np.nan
    x[3, :] = 2.5                                                  # a constant row
    x[4, :] = 0.0
    x[4, ::3] = -0.0                                               # -0.0 and +0.0 as the only values
    x[5, 9], x[5, 10] = 0.0, -0.0
    x[6, 3], x[6, 60] = np.inf, -np.inf
    x[7, :] = -0.0
    f32 = x.astype(np.float32)
    for norm in fo.NORMS:
        for mats, lib in (([x], [False]), ([x], [True]), ([base, x], [False, True]), ([f32, base], [True, False])):
            want = fo.fuse_rows(mats, None, lib, norm)
            for plan in ("row", "slab"):
                got = e.fuse_rows([on_device(e, a, n + 2) for a in mats], None, lib, norm, n=n, plan=plan)
                assert so.same_bits(got.cpu().numpy(), want), (norm, lib, plan)
    mm = fo.fuse_rows([x], norm="minmax")
    assert (mm[4] == 0.0).all() and (mm[7] == 0.0).all() and np.isnan(mm[2]).all()


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    a = torch.zeros((8, 50), dtype=torch.float64, device=e.device)
    b = torch.ones((8, 50), dtype=torch.float32, device=e.device)
    out = sentinel_out(e, 8, 50)
    ws = torch.empty(e.lib.dlc_fuse_rows_workspace_bytes(8, 50, 2), dtype=torch.uint8, device=e.device)
    good = dict(bufs=[a, b], n=50, weights=[1.0, 1.0], lib=[0, 1], norm="none", plan=AUTO, out=out, ws=ws)
    assert call(e, **good) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    out.view(torch.int64).fill_(SENTINEL)
    f64, f32 = _lib.DLC_F64, _lib.DLC_F32
    off4 = lambda t: torch.as_strided(t.view(torch.uint8), (8, 50), (t.stride(0) * t.element_size(), 1), 4)    # 4 bytes in
    bad = {"dtype": dict(dtypes=[f64, _lib.DLC_I8]), "weight inf": dict(weights=[1.0, float("inf")]),
           "weight nan": dict(weights=[float("nan"), 1.0]), "rows 0": dict(rows=0), "n 0": dict(n=0), "ld < n": dict(lds=[50, 49]),
           "ld_out < n": dict(out=torch.as_strided(out, (8, 49), (49, 1))),
           "misaligned fp64 source": dict(bufs=[off4(a), b], dtypes=[f64, f32], lds=[50, 50]),
           "misaligned fp32 source": dict(bufs=[a, torch.as_strided(b.view(torch.uint8), (8, 50), (200, 1), 2)], dtypes=[f64, f32],
                                          lds=[50, 50]),
           "misaligned out": dict(out=off4(out))}
    for what, change in bad.items():
        assert call(e, **dict(good, **change)) == _lib.DLC_ERR_BAD_ARG, what
        assert b"fuse_rows" in e.lib.dlc_last_error(e.ctx), what
    f = e.lib.dlc_fuse_rows
    two = lambda t, *v: (t * 2)(*v)
    ptrs, lds, w, lib, dts = two(C.c_void_p, a.data_ptr(), b.data_ptr()), two(C.c_int64, 50, 50), two(C.c_double, 1.0, 1.0), \
        two(C.c_int, 0, 1), two(C.c_int, f64, f32)
    dst, wsp = C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr())
    tail = (8, 50, 50, 0)
    assert f(e.ctx, 0, dts, ptrs, lds, w, lib, *tail, 1, AUTO, dst, 50, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_ARG
    assert f(e.ctx, 9, dts, ptrs, lds, w, lib, *tail, 1, AUTO, dst, 50, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_ARG
    assert f(e.ctx, 2, dts, ptrs, lds, w, lib, *tail, 3, AUTO, dst, 50, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_ARG      # norm
    assert f(e.ctx, 2, dts, ptrs, lds, w, lib, *tail, 1, 3, dst, 50, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_ARG         # plan
    for hole in range(2, 7):                                       # each of the five host arrays
        args = [e.ctx, 2, dts, ptrs, lds, w, lib, *tail, 1, AUTO, dst, 50, wsp, ws.numel(), None]
        args[hole] = None
        assert f(*args) == _lib.DLC_ERR_BAD_ARG, hole
    assert f(e.ctx, 2, dts, two(C.c_void_p, a.data_ptr(), None), lds, w, lib, *tail, 1, AUTO, dst, 50, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_ARG
    assert f(e.ctx, 2, dts, ptrs, lds, w, lib, *tail, 1, AUTO, None, 50, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_ARG
    assert f(None, 2, dts, ptrs, lds, w, lib, *tail, 1, AUTO, dst, 50, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_ARG
    big = two(C.c_int64, 1 << 31, 1 << 31)
    assert f(e.ctx, 2, dts, ptrs, big, w, lib, 8, 1 << 31, 50, 0, 1, AUTO, dst, 1 << 31, wsp, ws.numel(), None) == _lib.DLC_ERR_BAD_SHAPE
    # SLAB without its workspace: missing, too small, misaligned; AUTO takes ROW then (test_bits)
    assert f(e.ctx, 2, dts, ptrs, lds, w, lib, *tail, 1, SLAB, dst, 50, None, 0, None) == _lib.DLC_ERR_WORKSPACE
    assert f(e.ctx, 2, dts, ptrs, lds, w, lib, *tail, 1, SLAB, dst, 50, wsp, 8, None) == _lib.DLC_ERR_WORKSPACE
    odd = torch.empty(ws.numel() + 16, dtype=torch.uint8, device=e.device)
    assert f(e.ctx, 2, dts, ptrs, lds, w, lib, *tail, 1, SLAB, dst, 50, C.c_void_p(odd.data_ptr() + 8), ws.numel(), None) == _lib.DLC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out.view(torch.int64) == SENTINEL).all())
    # the engine's own checks
    for kw in (dict(norm="softmax"), dict(plan="tile"), dict(weights=[1.0]), dict(weights=[1.0, float("nan")]),
               dict(lower_is_better=[True, False, True]), dict(n=51), dict(out=torch.empty((8, 49), dtype=torch.float64, device=e.device)),
               dict(out=torch.empty((8, 50), dtype=torch.float32, device=e.device))):
        with pytest.raises(ValueError):
            e.fuse_rows([a, b], **kw)
    for srcs in ([], [a] * 9, [a, b[:7]], [a, b.to(torch.float16)], [a.cpu(), b]):
        with pytest.raises(ValueError):
            e.fuse_rows(srcs)


# ---- a planted revisit behind two confusers --------------------------------------------------------------------------------------
def test_planted_revisit_behind_two_confusers(dlc):
    """The reason for the fusion.  Each member alone ranks its own confuser first in every row; the sum of the
    standardised rows ranks the true column first in every row (asserted on the oracle, then on the GPU)."""
    a, d, true = fo.two_confusers_scene()
    assert (np.argmax(a, 1) != true).all() and (np.argmin(d, 1) != true).all()
    want = fo.fuse_rows([a, d], lower_is_better=[False, True])
    assert (np.argmax(want, 1) == true).all()
    offs = dlc.slope_offsets(1)
    _, alone_a, _ = dlc.sequence_topk(a, 1, 1, offs)
    _, alone_d, _ = dlc.sequence_topk(d, 1, 1, offs, lower_is_better=True)
    assert (alone_a[:, 0] != true).all() and (alone_d[:, 0] != true).all()
    fused = dlc.fuse_scores([a, d], lower_is_better=[False, True])
    assert isinstance(fused, np.ndarray) and so.same_bits(fused, want)
    s, i, _ = dlc.sequence_topk(fused, 1, 1, offs)
    assert np.array_equal(i[:, 0], true) and so.same_bits(s[:, 0], want[np.arange(len(true)), true])


# ---- the detector ----------------------------------------------------------------------------------------------------------------
FRAMES, K, EXCLUSION = 60, 3, 5
MEMBERS = [("cosine", 64), ("distance", 96), ("sad", 128, {})]
WEIGHTS = [1.0, 0.5, 2.0]


@pytest.fixture(scope="module")
def route():
    """60 frames seen by three descriptors; frames 40..55 revisit frames 8..23 in all three."""
    rng = np.random.RandomState(21)
    cos = rng.standard_normal((FRAMES, 64)).astype(np.float32)
    dist = rng.randint(-128, 128, size=(FRAMES, 96)).astype(np.int8)
    sad = rng.randint(0, 256, size=(FRAMES, 128)).astype(np.uint8)
    cos[40:56] = cos[8:24] + 0.4 * rng.standard_normal((16, 64)).astype(np.float32)
    dist[40:56] = dist[8:24]
    dist[40:56, ::3] = rng.randint(-128, 128, size=(16, 32)).astype(np.int8)
    sad[40:56] = sad[8:24]
    sad[40:56, ::4] = rng.randint(0, 256, size=(16, 32)).astype(np.uint8)
    return cos, dist, sad


def stream(det, xs, batch):
    e = det.engine
    outs = [det.query_and_insert([torch.from_numpy(x[lo:lo + batch]).to(e.device) for x in xs]) for lo in range(0, FRAMES, batch)]
    return tuple(torch.cat([o[t] for o in outs]).cpu().numpy() for t in range(len(outs[0])))


@pytest.fixture(scope="module")
def raw_rows(dlc, route):
    """The members' own raw rows as matrices [60, 60] (the stores' row methods over all frames at once), NumPy: computed
    once and shared."""
    det = dlc.FusedLoopClosureDetector(MEMBERS, k=K, exclusion=EXCLUSION, capacity=32)
    stream(det, route, 32)
    assert len(det) == FRAMES and all(len(db) == FRAMES and db.capacity >= 64 for db in det.dbs)      # the stores grew
    kw = dict(limit0=-EXCLUSION, limit_step=1)
    rows = [det.dbs[0].scores_f64(det.dbs[0].rows, **kw), det.dbs[1].distances(det.dbs[1].rows, **kw),
            det.dbs[2].differences(det.dbs[2].rows, **kw)]
    assert [r.dtype for r in rows] == [torch.float64, torch.int64, torch.int64]
    return [r.cpu().numpy() for r in rows]


@pytest.mark.parametrize("options", [{}, {"sequence": 4}, {"sequence": 4, "contrast": 3}, {"suppress": 2}, {"sequence": 4, "suppress": 2},
                                     {"sequence": 4, "steps": (0, 2)}, {"sequence": 4, "chains": True}, {"norm": "minmax"}],
                         ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()) or "plain")
def test_detector(dlc, route, raw_rows, options):
    def make():
        return dlc.FusedLoopClosureDetector(MEMBERS, weights=WEIGHTS, k=K, exclusion=EXCLUSION, capacity=32, **options)

    results = [stream(make(), route, batch) for batch in (1, 7, 32)]
    # the offline composition: the stores' rows, the fusion oracle, the sequence oracles
    kw = dict(limit0=-EXCLUSION, limit_step=1)
    fused = fo.fuse_rows(raw_rows, WEIGHTS, [False, True, True], options.get("norm", "zscore"), **kw)
    length = options.get("sequence") or 1
    if "contrast" in options:
        fused = co.contrast_rows(fused, options["contrast"], **kw)
    offs = dlc.slope_offsets(length)
    if "steps" in options:
        es, ei, _ = eo.elastic_topk(fused, K, length, *options["steps"], **kw)
    elif "suppress" in options:
        es, ei = po.peak_topk_rows(so.sequence_scores(fused, length, offs, **kw)[0], K, options["suppress"], **kw)
    else:
        es, ei, _ = so.sequence_topk(fused, K, length, offs, **kw)
    for res in results:
        assert res[0].dtype == np.float64 and res[1].dtype == np.int64
        assert np.array_equal(res[1], ei) and so.same_bits(res[0], es)
        if options.get("chains"):
            assert res[2].dtype == np.int32 and np.array_equal(res[2], cho.line_chains(fused, ei, length, offs, **kw)[0])
    # a frame with nothing old enough
    nothing = EXCLUSION + length
    assert (ei[:nothing] == -1).all() and np.isneginf(es[:nothing]).all() and (ei[nothing + K:, 0] >= 0).all()
    if not options:
        assert int((ei[43:56, 0] == np.arange(11, 24)).sum()) == 13                 # the revisit is found


def test_detector_surface(dlc, route):
    e = dlc.default_engine()
    det = dlc.FusedLoopClosureDetector(MEMBERS, k=K, exclusion=EXCLUSION, capacity=32, threshold=3.0)
    s, i = det.query_and_insert([torch.from_numpy(x).to(e.device) for x in route])
    found = det.loops(s, i, 0)
    assert found and all(score >= 3.0 and isinstance(score, float) and f - j > EXCLUSION for f, j, score in found)
    assert {f for f, _, _ in found} >= set(range(43, 56))
    everything = dlc.FusedLoopClosureDetector(MEMBERS, k=K, exclusion=EXCLUSION, capacity=32)
    s2, i2 = everything.query_and_insert(list(route))               # NumPy descriptors are taken too
    assert so.same_bits(s2.cpu().numpy(), s.cpu().numpy()) and len(everything.loops(s2, i2, 0)) == int((i2 >= 0).sum())
    empty = det.query_and_insert([x[:0] for x in route])
    assert empty[0].shape == (0, K) and empty[0].dtype == torch.float64 and empty[1].dtype == torch.int64
    judge = dlc.LoopClosureEvaluator(np.concatenate([np.arange(40), np.arange(8, 24), np.arange(100, 104)]), 0, EXCLUSION)
    judge.add(s, i, 0)                                             # the evaluator takes the detector's output as it is
    curve, _ = judge.result()
    assert judge.queries == FRAMES and curve.average_precision > 0.9
    for bad in (dict(members=[]), dict(members=[("sdav", 4)]), dict(members=MEMBERS, weights=[1.0]), dict(members=MEMBERS, norm="l2"),
                dict(members=MEMBERS, contrast=3), dict(members=MEMBERS, chains=True), dict(members=MEMBERS, steps=(0, 2)),
                dict(members=[("distance", 96, {"shift": 1})]), dict(members=[("sad", 128, {"shift": 2})]), dict(members=MEMBERS, k=0)):
        with pytest.raises(ValueError):
            dlc.FusedLoopClosureDetector(**bad)
    with pytest.raises(ValueError):
        det.query_and_insert([route[0]])
    with pytest.raises(ValueError):
        det.query_and_insert([route[0][:3], route[1][:2], route[2][:3]])
    shifted = dlc.FusedLoopClosureDetector([("sad", 128, {"shift": 2, "width": 16}), ("distance", 96)], k=K, exclusion=EXCLUSION)
    s3, i3 = shifted.query_and_insert([route[2], route[1]])
    rows = [shifted.dbs[0].differences(shifted.dbs[0].rows, limit0=-EXCLUSION, limit_step=1, shift=2, width=16).cpu().numpy(),
            shifted.dbs[1].distances(shifted.dbs[1].rows, limit0=-EXCLUSION, limit_step=1).cpu().numpy()]
    es, ei, _ = so.sequence_topk(fo.fuse_rows(rows, None, True, limit0=-EXCLUSION, limit_step=1), K, 1, [[0]], limit0=-EXCLUSION,
                                 limit_step=1)
    assert np.array_equal(i3.cpu().numpy(), ei) and so.same_bits(s3.cpu().numpy(), es)


# ---- the module's surface --------------------------------------------------------------------------------------------------------
def test_module_functions_numpy_and_tensors(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(12)
    mats = [member(rng, i, 40, 70) for i in range(3)]
    for norm in fo.NORMS:
        want = fo.fuse_rows(mats, [1.0, 2.0, -1.0], [False, True, False], norm, limit0=-3, limit_step=2)
        z = dlc.fuse_scores(mats, [1.0, 2.0, -1.0], [False, True, False], norm, limit0=-3, limit_step=2)
        assert isinstance(z, np.ndarray) and z.dtype == np.float64 and so.same_bits(z, want)           # NaN where not offered
        t = dlc.fuse_scores([torch.from_numpy(a).to(e.device) for a in mats], [1.0, 2.0, -1.0], [False, True, False], norm,
                            limit0=-3, limit_step=2)
        assert isinstance(t, torch.Tensor) and t.device == e.device and so.same_bits(t.cpu().numpy(), want)
    assert so.same_bits(dlc.fuse_scores(mats[:2], lower_is_better=True), fo.fuse_rows(mats[:2], lower_is_better=True))
    assert so.same_bits(dlc.fuse_scores([mats[0].astype(np.float16), mats[2].astype(np.int32)]),
                        fo.fuse_rows([mats[0].astype(np.float16).astype(np.float64), mats[2].astype(np.int32).astype(np.int64)]))
    assert dlc.fusion.fuse_scores is dlc.fuse_scores
    # the fused matrix feeds what takes any fp64 score matrix
    fused = dlc.fuse_scores(mats[:2], lower_is_better=[False, True], limit0=-3, limit_step=2)
    kw = dict(limit0=-3, limit_step=2)
    s, i, _ = dlc.sequence_topk(fused, 3, 4, **kw)
    es, ei, _ = so.sequence_topk(fused, 3, 4, dlc.slope_offsets(4), **kw)
    assert so.same_bits(s, es) and np.array_equal(i, ei)
    s, i = dlc.sequence_peaks(fused, 3, 4, 2, **kw)
    es, ei = po.peak_topk_rows(so.sequence_scores(fused, 4, dlc.slope_offsets(4), **kw)[0], 3, 2, **kw)
    assert so.same_bits(s, es) and np.array_equal(i, ei)
    truth = np.zeros(fused.shape, np.uint8)
    truth[np.arange(40), np.arange(40) // 2] = 1
    curve = dlc.pr_curve_cells(fused, truth, 16, **kw)
    assert curve.rows() and curve.positives > 0 and 0.0 <= curve.average_precision <= 1.0
    view = torch.randn((30, 700), dtype=torch.float64, device=e.device)[:, 100:500]      # a row-strided view, taken as it is
    assert so.same_bits(dlc.fuse_scores([view, view], [1.0, 0.5]).cpu().numpy(), fo.fuse_rows([view.cpu().numpy()] * 2, [1.0, 0.5]))
    for bad in (dict(matrices=[]), dict(matrices=[mats[0], mats[1][:, :60]]), dict(matrices=mats, norm="l2"),
                dict(matrices=[mats[0], torch.from_numpy(mats[1]).to(e.device)])):
        with pytest.raises(ValueError):
            dlc.fuse_scores(**bad)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_fuse(dlc):
    import glob
    from deeploopcloser_amd import loop_closure as lc, pipeline
    res = run_cli("--fuse", "sad,distance", "--sequence", "4", "--exclusion", "2", "--k", "2", "--batch", "4", "--no-latency-mode",
                  "--fuse-weights", "1,0.5")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    loops = [l for l in res.stdout.splitlines() if l.startswith("loop\t")]
    assert loops and len(loops) == len(res.stdout.splitlines())
    # the same in Python: the descriptors, the drivers' matrices, fuse_scores, sequence_topk
    files = sorted(glob.glob(os.path.join(GOLDEN, "datasets_test", "*.ppm")))
    frames = np.stack([dlc.read_ppm(f) for f in files])
    sad = pipeline.seqslam_descriptors_from_frames(frames, dlc.SeqSlam(size=(32, 64), patch=8, strength=32))
    net = dlc.CnnVtl(input_shape=[4] + list(frames.shape[1:]))
    deep = torch.cat([lc.describe_cnn_vtl(files[lo:lo + 4], net, as_int8=True) for lo in range(0, len(files), 4)])
    fused = dlc.fuse_scores([dlc.DifferenceCalculator.difference_matrix(sad), dlc.DistanceCalculator.distance_matrix(deep.cpu().numpy())],
                            weights=[1.0, 0.5], lower_is_better=True, limit0=-2, limit_step=1)
    s, i, _ = dlc.sequence_topk(fused, 2, 4, limit0=-2, limit_step=1)
    want = ["loop\t%d\t%s\t%d\t%s\t%.4f" % (f, os.path.basename(files[f]), i[f, c], os.path.basename(files[i[f, c]]), s[f, c])
            for f in range(len(files)) for c in range(2) if i[f, c] >= 0]
    assert loops == want
