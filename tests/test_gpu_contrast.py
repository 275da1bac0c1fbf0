"""GPU local contrast normalisation of score rows (dlc_contrast_rows, Engine.contrast_rows, sequence.contrast_normalize,
contrast=R on sequence_topk / sequence_scores, on the three detectors and on the CLI) against the NumPy restatement of
the definition (tests/contrast_oracle.py, pinned by test_contrast_cpu.py).  Every comparison is by bit pattern, any NaN
equal to any NaN by position (sequence_oracle.same_bits)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import contrast_oracle as co
import sequence_oracle as so

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
RADII = (1, 5, 32)
SHAPES = [(1, 1), (1, 2), (3, 11), (5, 3), (33, 130), (7, 1100), (3, 4100), (70_000, 3)]
KINDS = ["f64", "f32", "i64_distance", "i64_key"]


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def data(rng, kind, rows, n):
    if kind == "f64":
        return rng.standard_normal((rows, n)) * 10.0 ** rng.randint(-3, 4, size=(rows, 1))
    if kind == "f32":
        return rng.standard_normal((rows, n)).astype(np.float32)
    if kind == "i64_distance":
        return rng.randint(0, 4097, size=(rows, n)).astype(np.int64)
    return rng.randint(-(1 << 41), (1 << 41) + 1, size=(rows, n), dtype=np.int64)        # sums of cosine keys


def on_device(e, m, ld, beyond=None):
    """m [rows, n] as the first n columns of a [rows, ld] device view whose rows start at an ODD element of their
    allocation (8 bytes off a 16-byte boundary, 4 for fp32); the other columns hold `beyond` (default: a value no
    window may see without changing the result)."""
    rows, n = m.shape
    dt = torch.from_numpy(m[:1, :1]).dtype
    flat = torch.empty(rows * ld + 1, dtype=dt, device=e.device)
    buf = flat[1:].view(rows, ld)
    buf.fill_((1 << 50) if dt == torch.int64 else 1e30)
    if beyond is not None:
        buf.fill_(beyond)
    buf[:, :n] = torch.from_numpy(m).to(e.device)
    return buf


def sentinel_out(e, rows, ld_out):
    return torch.full((rows, ld_out), SENTINEL, dtype=torch.int64, device=e.device).view(torch.float64)


def expected_words(want, ld_out):
    """int64 [rows, ld_out]: the oracle's bits where a cell is offered (not NaN-by-absence), the sentinel elsewhere."""
    rows, n = want.shape
    words = np.full((rows, ld_out), SENTINEL, dtype=np.int64)
    words[:, :n] = want.view(np.int64)
    return words


def run(e, m, radius, limit0=None, step=0, beyond=None, offered=None):
    """One call at ld = n + 5, ld_out = n + 3 into a sentinel-filled buffer; returns the whole buffer as int64 words and
    checks the returned view."""
    rows, n = m.shape
    buf = on_device(e, m, n + 5, beyond)
    out = sentinel_out(e, rows, n + 3)
    got = e.contrast_rows(buf, radius, n=n, limit0=limit0, limit_step=step, out=out)
    assert got.shape == (rows, n) and got.data_ptr() == out.data_ptr() and got.stride(0) == n + 3
    return out.view(torch.int64).cpu().numpy()


def same_words(got, want):
    """Bit equality of two int64 word arrays that hold fp64 results, any NaN equal to any NaN by position."""
    return so.same_bits(got.view(np.float64), want.view(np.float64))


def check(e, m, radius, limit0=None, step=0, beyond=None):
    rows, n = m.shape
    want = co.contrast_rows(m, radius, limit0=limit0, limit_step=step)
    off = np.arange(n)[None, :] < so.limits(rows, n, n if limit0 is None else limit0, step)[:, None]
    words = expected_words(np.where(off, want, 0.0), n + 3)
    words[:, :n][~off] = SENTINEL
    got = run(e, m, radius, limit0, step, beyond)
    assert np.array_equal(got[:, n:], words[:, n:]), "columns n .. ld_out - 1 were touched"
    assert np.array_equal(got[:, :n][~off], words[:, :n][~off]), "cells at or past lim(r) were touched"
    assert same_words(got[:, :n][off], words[:, :n][off]), "offered cells differ from the definition"
    return got


# ---- B1: bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_bits(dlc, kind, shape):
    e = dlc.default_engine()
    rng = np.random.RandomState(1000 + 17 * KINDS.index(kind) + SHAPES.index(shape))
    m = data(rng, kind, *shape)
    for radius in RADII:
        check(e, m, radius)


@pytest.mark.parametrize("radius", RADII)
def test_special_values(dlc, radius):
    """-0.0, an infinity, a NaN, a constant stretch of 2 radius + 3 values, an int64 above 2^53 (it rounds on conversion)."""
    e = dlc.default_engine()
    rng = np.random.RandomState(7 + radius)
    n, c = 300, 2 * radius + 3
    m = rng.standard_normal((6, n))
    m[0, :] = -0.0
    m[1, 40:40 + c] = -0.0
    m[2, 100] = np.inf
    m[2, 299] = -np.inf
    m[3, 0] = np.nan
    m[3, 200] = np.nan
    m[4, 120:120 + c] = 3.25
    m[5, 255:255 + c] = m[5, 255]                                   # across the boundary of two column slabs
    got = check(e, m, radius).view(np.float64)
    assert np.array_equal(got[0, :n].view(np.uint64), np.zeros(n, np.uint64))             # +0.0, bit for bit
    mid = 120 + radius + 1
    assert got[4, mid] == 0.0 and got[4, mid - 1] == 0.0 and got[4, mid + 1] == 0.0 and got[4, 119] != 0.0
    assert np.isnan(got[2, 100 - radius:100 + radius + 1]).all() and not np.isnan(got[2, 100 + radius + 1])
    assert np.isnan(got[3, :radius + 1]).all() and not np.isnan(got[3, radius + 1])
    mi = rng.randint(0, 4097, size=(3, n)).astype(np.int64)
    mi[0, 50] = (1 << 53) + 1                                        # a tie: rounds to even, 2^53
    mi[1, 60] = (1 << 62) + 12345
    mi[1, 61] = -(1 << 60) - 3
    mi[2, 70:70 + c] = 1 << 41
    got = check(e, mi, radius).view(np.float64)
    assert got[2, 70 + radius + 1] == 0.0
    mf = rng.standard_normal((2, n)).astype(np.float32)
    mf[0, 10:10 + c] = np.float32(-0.0)
    mf[1, 33] = np.float32(np.inf)
    check(e, mf, radius)


# ---- B2: limits, and what is left alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("limit0,step", [(-4, 1), (0, 1), (120, 1), (7, 0), (136, -2), (20, -2)])
def test_limits_and_what_is_left_alone(dlc, limit0, step):
    e = dlc.default_engine()
    rng = np.random.RandomState(50 + limit0)
    for kind in ("f64", "i64_distance"):
        m = data(rng, kind, 33, 130)
        for radius in RADII:
            got = check(e, m, radius, limit0, step)
            if kind == "f64":
                # what lies at or past lim(r) is never read: NaN there -- in the matrix's columns and beyond them -- changes nothing
                lim = so.limits(33, 130, limit0, step)
                poisoned = m.copy()
                poisoned[np.arange(130)[None, :] >= lim[:, None]] = np.nan
                again = run(e, poisoned, radius, limit0, step, beyond=float("nan"))
                assert np.array_equal(again, got)


@pytest.mark.parametrize("limit0,step", [(0, 0), (-32, 1), (0, -1)])
def test_nothing_offered_touches_nothing(dlc, limit0, step):
    e = dlc.default_engine()
    m = data(np.random.RandomState(3), "f64", 33, 130)
    for radius in RADII:
        got = run(e, m, radius, limit0, step)
        assert (got == SENTINEL).all()
    buf, out = on_device(e, m, 135), sentinel_out(e, 33, 133)
    rc = e.lib.dlc_contrast_rows(e.ctx, 3, C.c_void_p(buf.data_ptr()), 33, 130, 135, limit0, step, 5, C.c_void_p(out.data_ptr()), 133, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((out.view(torch.int64) == SENTINEL).all())


# ---- B3: a row does not depend on its batch ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_row_does_not_depend_on_its_batch(dlc, kind):
    e = dlc.default_engine()
    m = data(np.random.RandomState(60), kind, 33, 130)
    for radius in RADII:
        for limit0 in (90, -3):
            whole = check(e, m, radius, limit0, 1)
            for size in (1, 5, 27):
                parts = [run(e, m[lo:lo + size], radius, limit0 + lo, 1) for lo in range(0, 33, size)]
                assert np.array_equal(np.concatenate(parts), whole), (radius, limit0, size)


# ---- B4: bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    m = torch.zeros((8, 50), dtype=torch.float64, device=e.device)
    out = sentinel_out(e, 8, 50)
    src, dst = C.c_void_p(m.data_ptr()), C.c_void_p(out.data_ptr())
    f = e.lib.dlc_contrast_rows
    assert f(e.ctx, _lib.DLC_F64, src, 8, 50, 50, 50, 0, 5, dst, 50, None) == _lib.DLC_OK
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    out.view(torch.int64).fill_(SENTINEL)
    bad = {"radius 0": (e.ctx, _lib.DLC_F64, src, 8, 50, 50, 50, 0, 0, dst, 50, None),
           "radius 33": (e.ctx, _lib.DLC_F64, src, 8, 50, 50, 50, 0, 33, dst, 50, None),
           "ld < n": (e.ctx, _lib.DLC_F64, src, 8, 50, 49, 50, 0, 5, dst, 50, None),
           "ld_out < n": (e.ctx, _lib.DLC_F64, src, 8, 50, 50, 50, 0, 5, dst, 49, None),
           "null out": (e.ctx, _lib.DLC_F64, src, 8, 50, 50, 50, 0, 5, None, 50, None),
           "null scores": (e.ctx, _lib.DLC_F64, None, 8, 50, 50, 50, 0, 5, dst, 50, None),
           "dtype": (e.ctx, _lib.DLC_I8, src, 8, 50, 50, 50, 0, 5, dst, 50, None),
           "rows 0": (e.ctx, _lib.DLC_F64, src, 0, 50, 50, 50, 0, 5, dst, 50, None),
           "n 0": (e.ctx, _lib.DLC_F64, src, 8, 0, 50, 50, 0, 5, dst, 50, None)}
    for what, args in bad.items():
        assert f(*args) == _lib.DLC_ERR_BAD_ARG, what
        assert b"contrast_rows" in e.lib.dlc_last_error(e.ctx), what
    assert f(e.ctx, _lib.DLC_F64, src, 8, 1 << 31, 1 << 31, 50, 0, 5, dst, 1 << 31, None) == _lib.DLC_ERR_BAD_SHAPE
    assert f(None, _lib.DLC_F64, src, 8, 50, 50, 50, 0, 5, dst, 50, None) == _lib.DLC_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out.view(torch.int64) == SENTINEL).all())
    # the engine's own checks
    for kw in (dict(radius=0), dict(radius=33), dict(radius=5, n=51), dict(radius=5, n=0),
               dict(radius=5, out=torch.empty((8, 49), dtype=torch.float64, device=e.device)),
               dict(radius=5, out=torch.empty((7, 50), dtype=torch.float64, device=e.device)),
               dict(radius=5, out=torch.empty((8, 50), dtype=torch.float32, device=e.device)),
               dict(radius=5, out=torch.empty((8, 50), dtype=torch.float64))):
        with pytest.raises(ValueError):
            e.contrast_rows(m, **kw)
    for scores in (m.to(torch.float16), m.cpu(), m[0]):
        with pytest.raises(ValueError):
            e.contrast_rows(scores, 5)


# ---- B5: a planted revisit behind a confuser band --------------------------------------------------------------------------
def test_planted_revisit_behind_a_confuser_band(dlc):
    """The reason for the normalisation.  Every revisiting frame shares 40 of its 64 bytes with a band of 40 older frames
    and 36 with the frame it revisits: every line through the band sums to a better score than the true line, and the
    plain sequence search answers with the band.  Within the band every neighbour is equally near, so the band
    normalises to nothing; the revisited frame stands out from ITS neighbours."""
    x, true = co.confuser_band_scene(0)
    d = dlc.DistanceCalculator.distance_matrix(x)
    kw = dict(limit0=-30, limit_step=1, lower_is_better=True)
    offs = dlc.slope_offsets(10)
    _, plain, _ = dlc.sequence_topk(d, 1, 10, offs, **kw)
    assert all(70 <= plain[f, 0] <= 109 for f in range(159, 180))
    s, i, v = dlc.sequence_topk(d, 1, 10, offs, contrast=5, **kw)
    assert np.array_equal(i[159:180, 0], np.arange(159, 180) - 130) and np.array_equal(i[159:180, 0], true[9:])
    es, ei, ev = so.sequence_topk(co.contrast_rows(d, 5, limit0=-30, limit_step=1), 1, 10, offs, **kw)
    assert s.dtype == np.float64 and so.same_bits(s, es) and np.array_equal(i, ei) and np.array_equal(v, ev)


# ---- B6: the detectors -----------------------------------------------------------------------------------------------------
L_SEQ, R_CON = 10, 5


def stream(det, x, batch):
    outs = [det.query_and_insert(x[lo:lo + batch]) for lo in range(0, x.shape[0], batch)]
    return torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy()


def same_lists(results, es, ei):
    for s, i in results:
        assert s.dtype == np.float64 and np.array_equal(i, ei) and so.same_bits(s, es)


def test_cnn_vtl_detector(dlc):
    x, true = co.confuser_band_scene(0)
    k, exclusion = 3, 30

    def make(**kw):
        return dlc.CnnVtlLoopClosureDetector(64, k=k, exclusion=exclusion, capacity=64, **kw)

    results = [stream(make(sequence=L_SEQ, contrast=R_CON), x, batch) for batch in (1, 7, 32)]
    d = dlc.DistanceCalculator.distance_matrix(x)                                  # the detector's own raw rows, as a matrix
    es, ei, _ = dlc.sequence_topk(d, k, L_SEQ, contrast=R_CON, limit0=-exclusion, limit_step=1, lower_is_better=True)
    same_lists(results, es, ei)
    assert np.array_equal(ei[159:180, 0], true[9:])                                # the revisit, not the band
    assert (ei[:L_SEQ - 1 + exclusion] == -1).all() and np.isposinf(es[:L_SEQ - 1 + exclusion]).all()
    _, plain = stream(make(sequence=L_SEQ), x, 32)
    assert all(70 <= plain[f, 0] <= 109 for f in range(159, 180))                  # without it: the band
    det = make(sequence=L_SEQ, contrast=R_CON, max_distance=-10.0)
    s, i = det.query_and_insert(x)
    found = det.loops(s, i, 0)
    assert found and all(dist <= -10.0 and isinstance(dist, float) for _, _, dist in found)
    assert {f for f, _, _ in found} >= set(range(159, 180))
    empty = det.query_and_insert(x[:0])
    assert empty[0].shape == (0, k) and empty[0].dtype == torch.float64
    with pytest.raises(ValueError):
        make(contrast=R_CON)
    with pytest.raises(ValueError):
        make(sequence=L_SEQ, contrast=33)
    # the default constructor is the detector as it was
    a, b = stream(make(), x, 32), stream(dlc.CnnVtlLoopClosureDetector(64, k=k, exclusion=exclusion, capacity=64), x, 32)
    assert a[0].dtype == np.int64 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = stream(make(sequence=L_SEQ, contrast=None), x, 32), stream(make(sequence=L_SEQ), x, 7)
    assert a[0].dtype == np.int64 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_cosine_detector(dlc):
    rng = np.random.RandomState(5)
    n, dim, k, exclusion = 90, 64, 4, 3
    x = rng.standard_normal((n, dim))
    x[60:80] = x[10:30] + 0.5 * rng.standard_normal((20, dim))

    def make(**kw):
        return dlc.LoopClosureDetector(dim, k=k, exclusion=exclusion, capacity=16, **kw)

    results = []
    for batch in (1, 7, 32):
        det = make(sequence=L_SEQ, contrast=R_CON)
        results.append(stream(det, x, batch))
    keys = det.db.score_keys(det.db.rows)                                          # the detector's own raw rows: int64 keys
    assert keys.dtype == torch.int64 and tuple(keys.shape) == (n, n)
    es, ei, _ = dlc.sequence_topk(keys, k, L_SEQ, contrast=R_CON, limit0=-exclusion, limit_step=1)
    es, ei = es.cpu().numpy(), ei.cpu().numpy()
    same_lists(results, es, ei)                                                    # (no 2^-40 rescale: sums of normalised values)
    assert (ei[:L_SEQ - 1 + exclusion] == -1).all() and np.isneginf(es[:L_SEQ - 1 + exclusion]).all()
    assert int((ei[69:80, 0] == np.arange(19, 30)).sum()) == 11                    # the revisit is found
    with pytest.raises(ValueError):
        make(contrast=R_CON)
    a, b = stream(make(), x, 32), stream(dlc.LoopClosureDetector(dim, k=k, exclusion=exclusion, capacity=16), x, 32)
    assert a[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = stream(make(sequence=L_SEQ, contrast=None), x, 32), stream(make(sequence=L_SEQ), x, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sdav_detector(dlc):
    e = dlc.default_engine()
    g = torch.Generator(device=e.device)
    g.manual_seed(77)
    n, p, h, k, exclusion = 80, 30, 250, 4, 3
    ds = torch.sigmoid(4.0 * torch.randn((n, p, h), generator=g, device=e.device, dtype=torch.float64))
    ds[50:75] = (ds[10:35] + 0.01 * torch.rand((25, p, h), generator=g, device=e.device, dtype=torch.float64)).clamp(0.001, 0.999)

    def make(**kw):
        return dlc.SdavLoopClosureDetector(ds, patches=p, width=h, k=k, exclusion=exclusion, capacity=8, **kw)

    results = [stream(make(sequence=L_SEQ, contrast=R_CON), ds, batch) for batch in (1, 7, 32)]
    sim = dlc.SimilarityCalculator(ds.cpu().numpy()).similarity_matrix(as_int64=False)      # the detector's own raw rows
    es, ei, _ = dlc.sequence_topk(sim, k, L_SEQ, contrast=R_CON, limit0=-exclusion, limit_step=1)
    same_lists(results, es, ei)
    assert (ei[:L_SEQ - 1 + exclusion] == -1).all() and np.isneginf(es[:L_SEQ - 1 + exclusion]).all()
    assert int((ei[59:75, 0] == np.arange(19, 35)).sum()) == 16                    # the revisit is found
    det, outs, tickets = make(sequence=L_SEQ, contrast=R_CON), [], []
    for lo in range(0, n, 16):                                                     # two batches in flight
        tickets.append(det.submit(ds[lo:lo + 16]))
        if len(tickets) > 1:
            outs.append(det.result(tickets[-2]))
    outs.append(det.result(tickets[-1]))
    same_lists([(torch.cat([o[0] for o in outs]).cpu().numpy(), torch.cat([o[1] for o in outs]).cpu().numpy())], es, ei)
    with pytest.raises(ValueError):
        make(contrast=R_CON)
    a, b = stream(make(), ds, 32), stream(dlc.SdavLoopClosureDetector(ds, patches=p, width=h, k=k, exclusion=exclusion, capacity=8), ds, 32)
    assert so.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = stream(make(sequence=L_SEQ, contrast=None), ds, 32), stream(make(sequence=L_SEQ), ds, 7)
    assert so.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a poisoned stream still answers (NaN, -1)
    det = make(sequence=3, contrast=2)
    det.query_and_insert(ds[:20])
    bad = ds[20].clone()
    bad[1, 1] = 1.5
    s, i = det.query_and_insert(bad)
    assert bool(s.isnan().all()) and bool((i == -1).all())


# ---- B7: the module's surface ----------------------------------------------------------------------------------------------
def test_module_functions_numpy_and_tensors(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(12)
    for kind in KINDS:
        m = data(rng, kind, 40, 70)
        want = co.contrast_rows(m, 4, limit0=-3, limit_step=1)
        z = dlc.contrast_normalize(m, 4, limit0=-3, limit_step=1)
        assert isinstance(z, np.ndarray) and z.dtype == np.float64 and so.same_bits(z, want)       # NaN where not offered
        t = dlc.contrast_normalize(torch.from_numpy(m).to(e.device), 4, limit0=-3, limit_step=1)
        assert isinstance(t, torch.Tensor) and t.device == e.device and so.same_bits(t.cpu().numpy(), want)
        assert so.same_bits(dlc.contrast_normalize(m, 4), co.contrast_rows(m, 4))
        for lower in (False, True):
            kw = dict(limit0=-3, limit_step=1, lower_is_better=lower)
            d = dlc.sequence_scores(m, 5, contrast=4, **kw)
            assert d.dtype == np.float64 and so.same_bits(d, dlc.sequence_scores(z, 5, **kw))
            assert so.same_bits(d, so.sequence_scores(want, 5, dlc.slope_offsets(5), **kw)[0])
            s, i, v = dlc.sequence_topk(m, 3, 5, contrast=4, **kw)
            s2, i2, v2 = dlc.sequence_topk(z, 3, 5, **kw)
            assert s.dtype == np.float64 and so.same_bits(s, s2) and np.array_equal(i, i2) and np.array_equal(v, v2)
    assert dlc.sequence.contrast_normalize is dlc.contrast_normalize and "contrast_normalize" in dlc.__all__
    with pytest.raises(ValueError):
        dlc.contrast_normalize(m, 0)
    with pytest.raises(ValueError):
        dlc.sequence_topk(m, 3, 5, contrast=33)
    view = torch.randn((30, 700), dtype=torch.float64, device=e.device)[:, 100:500]      # a row-strided view, taken as it is
    assert so.same_bits(dlc.contrast_normalize(view, 7).cpu().numpy(), co.contrast_rows(view.cpu().numpy(), 7))


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_contrast(dlc):
    res = run_cli("--network", "sdav", "--metric", "similarity", "--sequence", "5", "--contrast", "3", "--exclusion", "2", "--k", "2",
                  "--batch", "4")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    loops = [l.split("\t") for l in res.stdout.splitlines() if l.startswith("loop\t")]
    assert loops and all(int(l[1]) - int(l[3]) > 2 and int(l[1]) >= 2 + 4 + 1 for l in loops)   # old enough, and a full line behind it
    for args in (("--network", "sdav", "--metric", "similarity", "--contrast", "3"),
                 ("--network", "sdav", "--metric", "similarity", "--sequence", "5", "--contrast", "0"),
                 ("--network", "sdav", "--metric", "similarity", "--sequence", "5", "--contrast", "33")):
        res = run_cli(*args)
        assert res.returncode == 2 and "error:" in res.stderr and "usage:" in res.stderr
