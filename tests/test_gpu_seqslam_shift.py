"""GPU lateral-shift tolerant SeqSLAM difference: dlc_sad_u8_shift_rows / Engine.sad_rows(shift=, width=), the shift
arguments of DifferenceCalculator, SadKeyframeDatabase, SeqSlamLoopClosureDetector, the pipeline, the driver and the CLI.
The reference is tests/seqslam_shift_oracle.py (the definition of include/dlc.h restated in NumPy) and, behind it, the
existing sequence / elastic / peaks / chains / contrast oracles.  Every comparison is exact, values and shifts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import chains_oracle as ch
import contrast_oracle as co
import elastic_oracle as eo
import peaks_oracle as po
import real_frames
import seqslam_oracle as sq
import seqslam_shift_oracle as ss
import sequence_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def dev(e, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(e.device)


def padded_rows(x, extra=16, fill=0xFF):
    """x [n, d] uint8 inside rows of a larger 16-byte pitch whose padding is `fill`."""
    n, d = x.shape
    p = np.full((n, (d + 15) // 16 * 16 + extra), fill, dtype=np.uint8)
    p[:, :d] = x
    return p


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------
def thread_plan(q):
    """(threads across db rows, queries per thread): tk_plan of deeploopcloser_amd/csrc/distance_tile.h, restated."""
    if q <= 4:
        return 64, 1
    big, mid = -(-q // 64) * 64, -(-q // 16) * 16
    return (16, 4) if big <= mid else (64, 4)


# 70 pads to 80 by sixteens and to 128 by sixty-fours, so it takes the same plan as 5 and 17: 64 is here for the third one
SWEEP_Q = [1, 4, 5, 17, 64, 70]
SWEEP_N = [1, 63, 65, 130, 260]
# w < 16, not a multiple of 4; a multiple of 4 only; one 16-byte block; not a multiple of 16, between one block and a
# segment; one whole segment; two segments, the second 6 columns; three segments, the last 2 columns; two whole segments
# (the fast path's inner chunks reading across the segment boundary)
SWEEP_HW = [(3, 5), (2, 12), (4, 16), (8, 20), (32, 64), (3, 70), (2, 130), (2, 128)]
SWEEP_S = [1, 3, 4, 7, 8]


def test_sweep_reaches_every_plan():
    assert {thread_plan(q) for q in SWEEP_Q} == {(64, 1), (64, 4), (16, 4)}
    assert [thread_plan(q) for q in SWEEP_Q] == [(64, 1), (64, 1), (64, 4), (64, 4), (16, 4), (64, 4)]
    assert {s % 4 for s in SWEEP_S} == {0, 1, 3} and {w % 16 == 0 for _, w in SWEEP_HW} == {True, False}


@pytest.mark.parametrize("hw", SWEEP_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("q", SWEEP_Q)
def test_shift_rows_sweep(dlc, q, hw):
    """Every plan x every width x every S (capped at w - 1): each (plan, width class, S mod 4) occurs; N walks its values."""
    e = dlc.default_engine()
    h, w = hw
    d = h * w
    rng = np.random.RandomState(q * 1000 + d)
    for si, S in enumerate(sorted({min(s, w - 1) for s in SWEEP_S})):
        n = SWEEP_N[(si + SWEEP_Q.index(q) + SWEEP_HW.index(hw)) % len(SWEEP_N)]
        if d == 2048 and q >= 64:
            n = min(n, 65)                                             # (keeps the oracle of the largest case within a second)
        qs = rng.randint(0, 256, size=(q, d)).astype(np.uint8)
        db = rng.randint(0, 256, size=(n, d)).astype(np.uint8)
        qs[-1], db[-1] = 0, 255                                        # the largest sum of the shape: an unsigned read
        k = min(n - 1, 2)
        sh = min(S, 2)
        img = db[k].reshape(h, w)
        moved = rng.randint(0, 256, size=(h, w)).astype(np.uint8)
        moved[:, :w - sh] = img[:, sh:]
        qs[0] = moved.reshape(-1)                                      # query 0 is key-frame k moved sh columns to the left
        want_v, want_s = ss.shift_rows(qs, db, h, w, S)
        if n > 1:
            assert want_v[0, k] == 0 and want_s[0, k] == sh
        got_v, got_s = e.sad_rows(dev(e, qs), dev(e, db), shift=S, width=w, shift_out=True)
        assert got_v.dtype == torch.int64 and got_s.dtype == torch.int8
        assert np.array_equal(got_v.cpu().numpy(), want_v), (n, S)
        assert np.array_equal(got_s.cpu().numpy(), want_s), (n, S)


# ---- 2. limits, sentinels, operands ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,n,hw,S", [(1, 130, (8, 20), 3), (5, 63, (4, 16), 4), (17, 260, (3, 70), 8), (64, 65, (2, 12), 1)])
def test_limits_and_sentinels(dlc, q, n, hw, S):
    e = dlc.default_engine()
    h, w = hw
    rng = np.random.RandomState(q + n)
    qs = rng.randint(0, 256, size=(q, h * w)).astype(np.uint8)
    db = rng.randint(0, 256, size=(n, h * w)).astype(np.uint8)
    want_v, want_s = ss.shift_rows(qs, db, h, w, S)
    assert want_s.any()
    dq, ddb = dev(e, padded_rows(qs)), dev(e, padded_rows(db))
    sent_v = -(np.arange(q * (n + 3), dtype=np.int64).reshape(q, n + 3) * 2654435761 + 12345)
    sent_s = (np.arange(q * (n + 5)).reshape(q, n + 5) % 100 + 20).astype(np.int8)         # 20 .. 119: no shift looks so
    for limit0, step in ((n, 0), (3, 1), (n, -3), (2, 2), (0, 0)):
        buf_v, buf_s = dev(e, sent_v), dev(e, sent_s)
        out, sh = e.sad_rows(dq, ddb, d=h * w, limit0=limit0, limit_step=step, out=buf_v[:, :n], shift=S, width=w,
                             shift_out=buf_s[:, :n])
        assert out.data_ptr() == buf_v.data_ptr() and sh.data_ptr() == buf_s.data_ptr()
        offered = sq.offered(q, n, limit0, step)
        got_v, got_s = buf_v.cpu().numpy(), buf_s.cpu().numpy()
        assert np.array_equal(got_v[:, :n], np.where(offered, want_v, sent_v[:, :n])), (limit0, step)
        assert np.array_equal(got_s[:, :n], np.where(offered, want_s, sent_s[:, :n])), (limit0, step)
        assert np.array_equal(got_v[:, n:], sent_v[:, n:]) and np.array_equal(got_s[:, n:], sent_s[:, n:])
        # without shift_out (a null pointer) the values are the same
        buf_v = dev(e, sent_v)
        only = e.sad_rows(dq, ddb, d=h * w, limit0=limit0, limit_step=step, out=buf_v[:, :n], shift=S, width=w)
        assert isinstance(only, torch.Tensor) and np.array_equal(buf_v.cpu().numpy(), got_v)
    v, s = e.sad_rows(dq, ddb, d=h * w, limit0=3, limit_step=1, shift=S, width=w, shift_out=True)       # allocated: -1 and 0
    off = sq.offered(q, n, 3, 1)
    assert np.array_equal(v.cpu().numpy(), np.where(off, want_v, -1)) and np.array_equal(s.cpu().numpy(), np.where(off, want_s, 0))
    assert np.array_equal(e.sad_rows(dq, ddb, d=h * w, limit0=3, limit_step=1, shift=S, width=w).cpu().numpy(), np.where(off, want_v, -1))


def test_padded_rows_and_queries_that_are_db_rows(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(8)
    for (h, w), S in (((3, 70), 8), ((4, 16), 4), ((1, 37), 5)):
        x = rng.randint(0, 256, size=(300, h * w)).astype(np.uint8)
        rows = dev(e, padded_rows(x))                                  # 0xFF past D, and 16 bytes more of it
        want_v, want_s = ss.shift_rows(x[100:133], x, h, w, S)
        v, s = e.sad_rows(rows[100:133], rows, d=h * w, shift=S, width=w, shift_out=True)
        assert np.array_equal(v.cpu().numpy(), want_v) and np.array_equal(s.cpu().numpy(), want_s)
        assert (np.diag(want_v[:, 100:133]) == 0).all() and not np.diag(want_s[:, 100:133]).any()
        plain = e.sad_rows(dev(e, x[:9]), dev(e, x), shift=S, width=w)          # an unaligned pitch: copied to a padded one
        assert np.array_equal(plain.cpu().numpy(), ss.shift_rows(x[:9], x, h, w, S)[0])
        full = e.sad_rows(rows[:40], rows[:40], d=h * w, shift=S, width=w).cpu().numpy()   # shift s of (i, j) is -s of (j, i)
        assert np.array_equal(full, full.T)


def test_more_db_tiles_than_one_grid_row(dlc):
    """Past 65 536 db tiles a workgroup walks several of them (the grid's x extent is capped), at the smallest descriptor
    that has a shift (1 x 2, S = 1): 256-row tiles at Q = 1 against the oracle, 64-row tiles at Q = 64 against the same
    call on slices of the db that stay below the cap."""
    e = dlc.default_engine()
    rng = np.random.RandomState(21)
    n = 256 * 65536 + 300
    db = rng.randint(0, 256, size=(n, 2)).astype(np.uint8)
    q = np.array([[255, 3]], dtype=np.uint8)
    rows = e._rows16_u8(dev(e, db), 2)
    v, s = e.sad_rows(dev(e, q), rows, d=2, limit0=n - 7, shift=1, width=2, shift_out=True)
    d64 = db.astype(np.int64)
    v0 = np.abs(255 - d64[:, 0]) + np.abs(3 - d64[:, 1])               # the definition at 1 x 2, written out
    vm, vp = 2 * np.abs(3 - d64[:, 0]), 2 * np.abs(255 - d64[:, 1])    # s = -1: q[1] with d[0]; s = +1: q[0] with d[1]
    want_v = np.minimum(v0, np.minimum(vm, vp))
    want_s = np.where(v0 <= np.minimum(vm, vp), 0, np.where(vm <= vp, -1, 1)).astype(np.int8)
    small_v, small_s = ss.shift_rows(q, db[:1000], 1, 2, 1)
    assert np.array_equal(small_v[0], want_v[:1000]) and np.array_equal(small_s[0], want_s[:1000])
    want_v[n - 7:], want_s[n - 7:] = -1, 0
    assert np.array_equal(v.cpu().numpy()[0], want_v) and np.array_equal(s.cpu().numpy()[0], want_s)
    n = 64 * 65536 + 100
    rows = rows[:n]
    qs = rows[rng.randint(0, n, size=64)].clone()
    whole = e.sad_rows(qs, rows, d=2, shift=1, width=2)
    for lo in range(0, n, 1 << 21):
        assert torch.equal(whole[:, lo:lo + (1 << 21)], e.sad_rows(qs, rows[lo:lo + (1 << 21)], d=2, shift=1, width=2)), lo
    assert np.array_equal(whole[:2, :5000].cpu().numpy(), ss.shift_rows(qs[:2, :2].cpu().numpy(), db[:5000], 1, 2, 1)[0])


def test_shift_zero_is_the_plain_rows(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(9)
    from deeploopcloser_amd import _lib
    for (h, w), q, n in (((4, 16), 5, 130), ((3, 70), 64, 63), ((1, 1), 3, 9), ((32, 64), 1, 65)):
        qs, db = dev(e, rng.randint(0, 256, size=(q, h * w)).astype(np.uint8)), dev(e, rng.randint(0, 256, size=(n, h * w)).astype(np.uint8))
        plain = e.sad_rows(qs, db)
        assert torch.equal(e.sad_rows(qs, db, shift=0, width=w), plain) and torch.equal(e.sad_rows(qs, db, shift=None), plain)
        # the C call itself at max_shift = 0
        q16, d16 = e._rows16_u8(qs, h * w), e._rows16_u8(db, h * w)
        out = torch.full((q, n), -5, dtype=torch.int64, device=e.device)
        sh = torch.full((q, n), 77, dtype=torch.int8, device=e.device)
        assert e.lib.dlc_sad_u8_shift_rows(e.ctx, C.c_void_p(q16.data_ptr()), q, q16.stride(0), C.c_void_p(d16.data_ptr()), n,
                                           d16.stride(0), h, w, 0, n, 0, C.c_void_p(out.data_ptr()), n,
                                           C.c_void_p(sh.data_ptr()), n, e._stream()) == _lib.DLC_OK
        assert torch.equal(out, plain) and not bool(sh.any())


@pytest.mark.parametrize("h", [1, 256])
def test_the_extreme_sums(dlc, h):
    """0 against 255 at h * w = 65536: 255 * 65536 at every shift, the tie goes to shift 0 -- and one pair of random rows of
    the same shape, whose seventeen sums are all near 85 * 65536 and rescaled by 65536 / (65536 - |s|) or 256 / (256 - |s|)."""
    e = dlc.default_engine()
    w = 65536 // h
    q, d = np.zeros((1, 65536), np.uint8), np.full((1, 65536), 255, np.uint8)
    v, s = e.sad_rows(dev(e, q), dev(e, d), shift=8, width=w, shift_out=True)
    assert int(v[0, 0]) == 255 * 65536 and int(s[0, 0]) == 0
    rng = np.random.RandomState(h)
    q, d = rng.randint(0, 256, size=(1, 65536)).astype(np.uint8), rng.randint(0, 256, size=(1, 65536)).astype(np.uint8)
    v, s = e.sad_rows(dev(e, q), dev(e, d), shift=8, width=w, shift_out=True)
    want_v, want_s = ss.shift_rows(q, d, h, w, 8)
    assert np.array_equal(v.cpu().numpy(), want_v) and np.array_equal(s.cpu().numpy(), want_s)


# ---- 3. the real frames ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crops(dlc):
    """(A, B) uint8 [20, 192, 192]: the green channel of the real frames, columns 0 .. 191 and 24 .. 215 -- the revisit an
    eighth of the crop to the side, 8 thumbnail columns at 32 x 64."""
    g = np.stack([dlc.read_ppm(p)[:, :, 1] for p in real_frames.frame_paths()])
    return np.ascontiguousarray(g[:, :, :192]), np.ascontiguousarray(g[:, :, 24:216])


def test_real_frames_through_the_database(dlc, crops):
    a, b = crops
    net = dlc.SeqSlam(size=(32, 64), patch=8, strength=32)
    e = net.engine
    da, dq = net.transform_tensor(dev(e, a)), net.transform_tensor(dev(e, b))
    assert np.array_equal(da.cpu().numpy(), sq.describe(a, (32, 64), 8, 32))
    db = dlc.SadKeyframeDatabase.empty(2048, capacity=32)
    db.append(da)
    v, s = db.differences(dq, shift=8, width=64, return_shift=True)
    want_v, want_s = ss.shift_rows(dq.cpu().numpy(), da.cpu().numpy(), 32, 64, 8)
    assert np.array_equal(v.cpu().numpy(), want_v) and np.array_equal(s.cpu().numpy(), want_s)
    truth = np.arange(20)
    assert (np.diag(want_v) == 0).all() and (np.diag(want_s) == 8).all()
    assert np.array_equal(v.argmin(dim=1).cpu().numpy(), truth)
    plain = db.differences(dq)
    assert int((plain.argmin(dim=1).cpu() != torch.from_numpy(truth)).sum()) >= 1
    assert isinstance(db.differences(dq, shift=8, width=64), torch.Tensor)
    # the calculator's two calls, NumPy in and out
    cv, cs = dlc.DifferenceCalculator.difference_rows(dq.cpu().numpy(), da, shift=8, width=64, return_shift=True)
    assert isinstance(cv, np.ndarray) and cs.dtype == np.int8 and np.array_equal(cv, want_v) and np.array_equal(cs, want_s)
    assert np.array_equal(dlc.DifferenceCalculator.difference_rows(dq, da, shift=8, width=64), want_v)
    mv, ms = dlc.DifferenceCalculator.difference_matrix(da, shift=3, width=64, return_shift=True)
    wv, ws = ss.shift_rows(da.cpu().numpy(), da.cpu().numpy(), 32, 64, 3)
    assert np.array_equal(mv, wv) and np.array_equal(ms, ws)
    assert np.array_equal(dlc.DifferenceCalculator.difference_matrix(da, shift=3, width=64), wv)


# ---- 4. errors ------------------------------------------------------------------------------------------------------------
def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    db = torch.zeros((50, 32), dtype=torch.uint8, device=e.device)
    qs = torch.zeros((4, 32), dtype=torch.uint8, device=e.device)
    out = torch.full((4, 50), -7, dtype=torch.int64, device=e.device)
    sh = torch.full((4, 50), 55, dtype=torch.int8, device=e.device)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def c_call(qp=vp(qs), Q=4, ldq=32, dbp=vp(db), N=50, ldd=32, h=2, w=16, S=3, ld_out=50, o=vp(out), s=vp(sh), ld_shift=50):
        return e.lib.dlc_sad_u8_shift_rows(e.ctx, qp, Q, ldq, dbp, N, ldd, h, w, S, 50, 0, o, ld_out, s, ld_shift, e._stream())
    arg, shape = _lib.DLC_ERR_BAD_ARG, _lib.DLC_ERR_BAD_SHAPE
    cases = [(dict(qp=vp(qs, 1), h=1), arg), (dict(dbp=vp(db, 8), h=1), arg), (dict(ldq=24, h=1), arg), (dict(ldd=40), arg),
             (dict(ld_out=49), arg), (dict(qp=None), arg), (dict(dbp=None), arg), (dict(o=None), arg), (dict(o=vp(out, 4)), arg),
             (dict(Q=0), arg), (dict(N=0), arg), (dict(h=3), arg),                      # 48 bytes in rows of 32
             (dict(h=0), arg), (dict(w=0), arg), (dict(h=-1), arg), (dict(S=-1), arg), (dict(ld_shift=49), arg),
             (dict(S=9), shape), (dict(h=4, w=8, S=8), shape), (dict(h=32, w=1, S=1), shape),          # S > 8; S >= w
             (dict(h=1, w=65552, ldq=1 << 17, ldd=1 << 17), shape),                     # w > 65536
             (dict(h=257, w=65536, ldq=1 << 25, ldd=1 << 25), shape),                   # h * w > 2^24
             (dict(Q=(1 << 20) + 1), shape), (dict(N=1 << 32, ld_out=1 << 32, ld_shift=1 << 32), shape)]
    for kw, want in cases:
        rc = c_call(**kw)
        assert rc == want, kw
        with pytest.raises(ValueError):
            e._check(rc)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((sh == 55).all())         # nothing was written
    assert c_call(ld_shift=0, s=None) == _lib.DLC_OK                   # a null shift_out: its pitch is not looked at
    assert c_call(h=4, w=8, S=7) == _lib.DLC_OK and c_call(S=8) == _lib.DLC_OK           # the limits themselves are inside
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(sh.any())
    db8 = dlc.SadKeyframeDatabase.empty(32)
    db8.append(db)
    for bad in (lambda: e.sad_rows(qs, db, shift=2),                   # no width
                lambda: e.sad_rows(qs, db, shift=2, width=5),          # 32 is no multiple of it
                lambda: e.sad_rows(qs, db, shift=2, width=0),
                lambda: e.sad_rows(qs, db, shift=9, width=16), lambda: e.sad_rows(qs, db, shift=-1, width=16),
                lambda: e.sad_rows(qs, db, shift=4, width=4), lambda: e.sad_rows(qs, db, shift=1, width=1),
                lambda: e.sad_rows(qs, db, shift_out=True),            # shifts of the plain rows
                lambda: e.sad_rows(qs, db, shift=2, width=16, shift_out=torch.zeros((4, 49), dtype=torch.int8, device=e.device)),
                lambda: e.sad_rows(qs, db, shift=2, width=16, shift_out=torch.zeros((4, 50), dtype=torch.int16, device=e.device)),
                lambda: e.sad_rows(qs, db, shift=2, width=16, out=torch.zeros((4, 50), dtype=torch.int32, device=e.device)),
                lambda: e.sad_rows(qs.to(torch.int8), db, shift=2, width=16),
                lambda: db8.differences(qs, shift=2), lambda: db8.differences(qs, shift=2, width=5),
                lambda: dlc.DifferenceCalculator.difference_rows(qs, db, shift=2),
                lambda: dlc.DifferenceCalculator.difference_matrix(db, shift=16, width=16),
                lambda: dlc.SeqSlamLoopClosureDetector(32, shift=2), lambda: dlc.SeqSlamLoopClosureDetector(32, shift=2, width=5),
                lambda: dlc.SeqSlamLoopClosureDetector(32, shift=9, width=16),
                lambda: dlc.SeqSlamLoopClosureDetector(32, shift=-1, width=16),
                lambda: dlc.SeqSlamLoopClosureDetector(32, shift=4, width=4)):
        with pytest.raises(ValueError):
            bad()
    assert torch.equal(e.sad_rows(qs, db, shift=3, width=4), e.sad_rows(qs, db, shift=3, width=16))    # (all zeros either way)


# ---- 5. the detector ------------------------------------------------------------------------------------------------------
K_DET, EXCLUSION, L_SEQ = 3, 5, 4
SIZE, S_DET = (32, 64), 8


@pytest.fixture(scope="module")
def scene(crops):
    """40 frames: the 20 crops A, then the 20 crops B -- the same route again, 8 thumbnail columns to the side.  (oracle
    descriptors [40, 2048], the oracle's shifted matrix, the oracle's plain matrix)."""
    a, b = crops
    desc = sq.describe(np.concatenate([a, b]), SIZE, 8, 32)
    return desc, ss.shift_rows(desc, desc, SIZE[0], SIZE[1], S_DET)[0], sq.sad_rows(desc, desc)


def stream(det, x, batch):
    outs = [det.query_and_insert(x[lo:lo + batch]) for lo in range(0, x.shape[0], batch)]
    return tuple(torch.cat([o[t] for o in outs]).cpu().numpy() for t in range(len(outs[0])))


def expected(dlc, m, variant):
    """The oracle pipeline over the oracle's shifted matrix m for one detector variant: (diff, ids[, chain])."""
    kw = dict(limit0=-EXCLUSION, limit_step=1, lower_is_better=True)
    if "sequence" not in variant:
        return po.peak_topk_rows(m, K_DET, variant.get("suppress", 0), **kw)
    offs = dlc.slope_offsets(L_SEQ)
    if "steps" in variant:
        s, i, _ = eo.elastic_topk(m, K_DET, L_SEQ, *variant["steps"], **kw)
        return s, i, ch.elastic_chains(m, i, L_SEQ, *variant["steps"], **kw)[0]
    if "contrast" in variant:
        return so.sequence_topk(co.contrast_rows(m, variant["contrast"], limit0=-EXCLUSION, limit_step=1), K_DET, L_SEQ, offs, **kw)[:2]
    return so.sequence_topk(m, K_DET, L_SEQ, offs, **kw)[:2]


@pytest.mark.parametrize("variant", [dict(), dict(suppress=3), dict(sequence=L_SEQ), dict(sequence=L_SEQ, contrast=5),
                                     dict(sequence=L_SEQ, steps=(0, 2), chains=True)],
                         ids=lambda v: "-".join("%s%s" % kv for kv in v.items()) or "plain")
def test_detector(dlc, scene, variant):
    desc, m, plain = scene
    want = expected(dlc, m, variant)
    results = []
    for batch in (1, 7, 40):
        det = dlc.SeqSlamLoopClosureDetector(2048, k=K_DET, exclusion=EXCLUSION, capacity=8, shift=S_DET, width=SIZE[1], **variant)
        got = stream(det, desc, batch)
        results.append(got)
        assert len(det) == 40 and len(got) == len(want)
        assert so.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), batch
        if len(want) == 3:
            assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), batch
    for got in results[1:]:                                            # the lists do not depend on the batching
        assert all(so.same_bits(x, y) for x, y in zip(got, results[0]))
    ids, diff = results[0][1], results[0][0]
    if not variant:
        # frame 20 + i is frame i seen 8 columns to the side: the shifted difference is 0, the plain one loses frames
        assert np.array_equal(ids[20:, 0], np.arange(20)) and (diff[20:, 0] == 0).all()
        det = dlc.SeqSlamLoopClosureDetector(2048, k=K_DET, exclusion=EXCLUSION)
        assert (stream(det, desc, 40)[1][20:, 0] != np.arange(20)).any()
    if variant == dict(sequence=L_SEQ):
        assert np.array_equal(ids[23:, 0], np.arange(3, 20)) and (diff[23:, 0] == 0).all() and diff.dtype == np.int64
    zero = dlc.SeqSlamLoopClosureDetector(2048, k=K_DET, exclusion=EXCLUSION, shift=0, width=SIZE[1], **variant)    # S = 0: plain
    none = dlc.SeqSlamLoopClosureDetector(2048, k=K_DET, exclusion=EXCLUSION, **variant)
    assert all(so.same_bits(x, y) for x, y in zip(stream(zero, desc, 40), stream(none, desc, 40)))


# ---- 6. driver and CLI ----------------------------------------------------------------------------------------------------
def golden_gray(dlc):
    from oracle import patches as opatch
    folder = os.path.join(GOLDEN, "datasets_test")
    return folder, np.stack([opatch.bgr2gray_opencv(dlc.read_ppm(os.path.join(folder, f))) for f in sorted(os.listdir(folder))])


def test_create_difference_matrix(dlc):
    from deeploopcloser_amd import drivers
    folder, gray = golden_gray(dlc)
    net = dlc.SeqSlam(size=(24, 32), patch=8, strength=32)
    d = sq.describe(gray, (24, 32), 8, 32)
    got = drivers.create_difference_matrix(folder, network=net, shift=4)
    assert got.dtype == np.int64 and np.array_equal(got, ss.shift_rows(d, d, 24, 32, 4)[0])
    assert np.array_equal(drivers.create_difference_matrix(folder, network=net, shift=0), sq.sad_rows(d, d))


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_shift(dlc):
    res = run_cli("--network", "seqslam", "--metric", "sad", "--sequence", "3", "--exclusion", "2", "--k", "2", "--batch", "4",
                  "--size", "24x32", "--shift", "4")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    loops = [l.split("\t") for l in res.stdout.splitlines() if l.startswith("loop\t")]
    _, gray = golden_gray(dlc)
    d = sq.describe(gray, (24, 32), 8, 32)
    m = ss.shift_rows(d, d, 24, 32, 4)[0]
    assert not np.array_equal(m, sq.sad_rows(d, d))
    s, i, _ = so.sequence_topk(m, 2, 3, dlc.slope_offsets(3), limit0=-2, limit_step=1, lower_is_better=True)
    want = [(f, int(i[f, c]), int(s[f, c])) for f in range(17) for c in range(2) if i[f, c] >= 0]
    assert loops and [(int(l[1]), int(l[3]), int(l[5])) for l in loops] == want
