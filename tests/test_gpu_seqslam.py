"""GPU SeqSLAM front-end: dlc_seqslam_describe_u8 / Engine.seqslam_describe, dlc_sad_u8_rows / Engine.sad_rows, SeqSlam,
DifferenceCalculator, SadKeyframeDatabase, SeqSlamLoopClosureDetector, the pipeline, the driver and the CLI.  The reference
is tests/seqslam_oracle.py (the two definitions of include/dlc.h restated in NumPy) and, behind it, the existing sequence /
elastic / peaks / chains / contrast oracles.  Every comparison is exact."""
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
import sequence_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def golden_gray(dlc):
    """uint8 [20, 192, 240]: the real frames, grey by the oracle's conversion."""
    from oracle import patches as opatch
    return np.stack([opatch.bgr2gray_opencv(dlc.read_ppm(p)) for p in real_frames.frame_paths()])


def describe(dlc, gray, size, patch, strength, **kw):
    e = dlc.default_engine()
    return e.seqslam_describe(torch.from_numpy(np.ascontiguousarray(gray)).to(e.device), size, patch, strength, **kw).cpu().numpy()


# ---- 1. describe ----------------------------------------------------------------------------------------------------------
def test_describe_golden_frames(dlc, golden_gray):
    for size in ((24, 32), (32, 64)):                                  # 8 x 7.5 pixels per cell; 6 x 3.75
        got = describe(dlc, golden_gray, size, 8, 32)
        want = sq.describe(golden_gray, size, 8, 32)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), size
        assert ((want == 0) | (want == 255)).mean() < 0.01 and len(np.unique(want)) > 100       # ordinary descriptors
    # grey on the device first: what SeqSlam.transform_tensor runs
    e = dlc.default_engine()
    rgb = np.stack([dlc.read_ppm(p) for p in real_frames.frame_paths()[:3]])
    assert np.array_equal(e.rgb_to_gray(torch.from_numpy(rgb).to(e.device)).cpu().numpy(), golden_gray[:3])


# (H, W), (h, w), patch: clipped edge tiles and ragged weights; the identity resize; one tile larger than the image; tiles
# of one cell; fewer cells than lanes; a single cell; the largest thumbnail (64 KiB of LDS) with the largest tile
SHAPES = [((10, 13), (3, 5), 2), ((7, 9), (7, 9), 4), ((16, 16), (4, 4), 64), ((10, 13), (3, 5), 1), ((33, 47), (2, 3), 3),
          ((40, 50), (1, 1), 8), ((19, 23), (19, 1), 5), ((256, 256), (256, 256), 64), ((50, 70), (9, 11), 64)]


@pytest.mark.parametrize("shape,size,patch", SHAPES)
@pytest.mark.parametrize("frames", [1, 5])
def test_describe_shapes(dlc, shape, size, patch, frames):
    rng = np.random.RandomState(shape[0] * 31 + size[1] * 7 + patch + frames)
    gray = rng.randint(0, 256, size=(frames,) + shape).astype(np.uint8)
    if frames == 5:
        gray[1] = rng.randint(100, 104, size=shape)                    # nearly flat: tiles with tiny variances
        gray[2] = gray[2] // 64 * 64                                   # four grey levels: some tiles flat after the resize
    for strength in (32, 1, 127):
        got = describe(dlc, gray, size, patch, strength)
        want = sq.describe(gray, size, patch, strength)
        assert np.array_equal(got, want), strength
        if patch == 1 or size == (1, 1):
            assert (got == 128).all()


def test_describe_constant_checkerboard_and_clamp(dlc):
    flat = np.full((1, 16, 16), 77, np.uint8)
    assert (describe(dlc, flat, (4, 4), 2, 32) == 128).all()
    board = (np.indices((8, 8)).sum(axis=0) % 2 * 255).astype(np.uint8)[None]
    for strength in (1, 32, 127):
        got = describe(dlc, board, (8, 8), 4, strength)
        assert np.array_equal(got, sq.describe(board, (8, 8), 4, strength)) and len(np.unique(got)) == 2
    assert (describe(dlc, board, (4, 4), 2, 127) == 128).all()         # 2 x 2 block means of a checkerboard are equal
    sharp = np.zeros((1, 8, 8), np.uint8)
    sharp[0, 0, 0] = 255
    got = describe(dlc, sharp, (8, 8), 8, 127)
    assert np.array_equal(got, sq.describe(sharp, (8, 8), 8, 127)) and got[0, 0] == 255 and got[0, 1] < 128     # the clamp
    dark = 255 - sharp
    got = describe(dlc, dark, (8, 8), 8, 127)
    assert np.array_equal(got, sq.describe(dark, (8, 8), 8, 127)) and got[0, 0] == 0


def test_describe_padding_survives(dlc, golden_gray):
    e = dlc.default_engine()
    gray = torch.from_numpy(golden_gray[:5]).to(e.device)
    for f in (5, 1):
        buf = torch.full((f, 24 * 32 + 48), 201, dtype=torch.uint8, device=e.device)
        out = e.seqslam_describe(gray[:f], (24, 32), 8, 32, out=buf)
        assert out.data_ptr() == buf.data_ptr() and tuple(out.shape) == (f, 768)
        assert np.array_equal(out.cpu().numpy(), sq.describe(golden_gray[:f], (24, 32), 8, 32))
        assert bool((buf[:, 768:] == 201).all())
    wide = torch.full((5, 2000), 7, dtype=torch.uint8, device=e.device)
    e.seqslam_describe(gray, (24, 32), 8, 32, out=wide[:, :800])       # a row-strided view: ld_out = 2000
    assert np.array_equal(wide[:, :768].cpu().numpy(), sq.describe(golden_gray[:5], (24, 32), 8, 32))
    assert bool((wide[:, 768:] == 7).all())


def test_describe_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    gray = torch.zeros((2, 300, 300), dtype=torch.uint8, device=e.device)
    out = torch.full((2, 70000), 9, dtype=torch.uint8, device=e.device)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def call(g=vp(gray), frames=2, H=300, W=300, h=4, w=5, patch=2, strength=32, o=vp(out), ld=70000):
        return e.lib.dlc_seqslam_describe_u8(e.ctx, g, frames, H, W, h, w, patch, strength, o, ld, e._stream())
    arg, shape = _lib.DLC_ERR_BAD_ARG, _lib.DLC_ERR_BAD_SHAPE
    cases = [(dict(g=None), arg), (dict(o=None), arg), (dict(frames=0), arg), (dict(patch=0), arg), (dict(patch=65), arg),
             (dict(strength=0), arg), (dict(strength=128), arg), (dict(ld=19), arg),
             (dict(h=0), shape), (dict(w=0), shape), (dict(h=301), shape), (dict(w=301), shape),
             (dict(h=257, w=256), shape),                              # 65 792 cells
             (dict(H=4096, W=2048, h=4, w=4), shape)]                  # 2^23 pixels (refused before anything is read)
    for kw, want in cases:
        rc = call(**kw)
        assert rc == want, kw
        with pytest.raises(ValueError):
            e._check(rc)
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                      # nothing was written
    assert call(h=256, w=256, patch=64, strength=127) == _lib.DLC_OK   # the limits themselves are inside
    assert call(patch=1, strength=1, ld=20) == _lib.DLC_OK
    torch.cuda.synchronize()
    for bad in (lambda: e.seqslam_describe(gray.float(), (4, 5), 2, 32), lambda: e.seqslam_describe(gray[0], (4, 5), 2, 32),
                lambda: e.seqslam_describe(gray.cpu(), (4, 5), 2, 32), lambda: e.seqslam_describe(gray, (0, 5), 2, 32),
                lambda: e.seqslam_describe(gray, (4, 5), 2, 32, out=out[:, :19]),
                lambda: e.seqslam_describe(gray, (4, 5), 2, 32, out=out[:1]),
                lambda: dlc.SeqSlam(size=(300, 300)), lambda: dlc.SeqSlam(patch=0), lambda: dlc.SeqSlam(strength=128)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. SAD rows ----------------------------------------------------------------------------------------------------------
NS, DS = (1, 63, 257), (1, 15, 16, 17, 64, 65, 200)


def padded_rows(rng, x, extra=16):
    """x [n, d] uint8 inside rows of a larger 16-byte pitch whose padding is random."""
    n, d = x.shape
    p = rng.randint(0, 256, size=(n, (d + 15) // 16 * 16 + extra)).astype(np.uint8)
    p[:, :d] = x
    return p


def tile_plan(q):
    """(queries, db rows) of a tile: tk_plan of deeploopcloser_amd/csrc/distance_tile.h, restated."""
    if q <= 4:
        return 1, 256
    big, mid = -(-q // 64) * 64, -(-q // 16) * 16
    return (64, 64) if big <= mid else (16, 256)


SWEEP_Q = [1, 4, 5, 17, 64, 65, 128]


def test_sweep_reaches_every_tile_plan():
    """1 x 256 tiles up to Q = 4; 64 x 64 where padding Q to 64 costs no more than padding it to 16 (Q mod 64 in 49 .. 64:
    64, and 128 for two query tiles); 16 x 256 otherwise (5, 17, 65: one, two and five query tiles)."""
    assert [tile_plan(q) for q in SWEEP_Q] == [(1, 256), (1, 256), (16, 256), (16, 256), (64, 64), (16, 256), (64, 64)]


@pytest.mark.parametrize("q", SWEEP_Q)
def test_sad_rows_sweep(dlc, q):
    e = dlc.default_engine()
    rng = np.random.RandomState(q)
    for n in NS:
        for d in DS:
            qs = rng.randint(0, 256, size=(q, d)).astype(np.uint8)
            db = rng.randint(0, 256, size=(n, d)).astype(np.uint8)
            qs[-1], db[-1] = 0, 255                                    # |0 - 255| = 255 per byte: a signed read would say 1
            want = sq.sad_rows(qs, db)
            assert want[-1, -1] == 255 * d
            dq, ddb = torch.from_numpy(padded_rows(rng, qs)).to(e.device), torch.from_numpy(padded_rows(rng, db)).to(e.device)
            sentinel = -(np.arange(q * (n + 3), dtype=np.int64).reshape(q, n + 3) * 2654435761 + 12345)
            for limit0, step in ((n, 0), (3, 1), (n, -1), (0, 0)):
                buf = torch.from_numpy(sentinel.copy()).to(e.device)
                out = e.sad_rows(dq, ddb, d=d, limit0=limit0, limit_step=step, out=buf[:, :n])
                assert out.data_ptr() == buf.data_ptr()
                got = buf.cpu().numpy()
                offered = np.zeros((q, n + 3), bool)
                offered[:, :n] = sq.offered(q, n, limit0, step)
                assert np.array_equal(got[offered], want[offered[:, :n]]), (n, d, limit0, step)
                assert np.array_equal(got[~offered], sentinel[~offered]), (n, d, limit0, step)
            fresh = e.sad_rows(dq, ddb, d=d, limit0=3, limit_step=1).cpu().numpy()       # engine-allocated: -1 where not offered
            assert np.array_equal(fresh, np.where(sq.offered(q, n, 3, 1), want, -1))
            assert np.array_equal(e.sad_rows(dq, ddb, d=d).cpu().numpy(), want)


def test_sad_rows_queries_may_be_db_rows_and_unpadded_rows(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(8)
    x = rng.randint(0, 256, size=(300, 37)).astype(np.uint8)
    dev = torch.from_numpy(padded_rows(rng, x)).to(e.device)
    own = e.sad_rows(dev[100:133], dev, d=37)
    assert np.array_equal(own.cpu().numpy(), sq.sad_rows(x[100:133], x))
    full = e.sad_rows(dev, dev, d=37).cpu().numpy()                    # the difference matrix: symmetric, zero diagonal
    assert np.array_equal(full, full.T) and (np.diag(full) == 0).all() and np.array_equal(full, sq.sad_rows(x, x))
    plain = e.sad_rows(torch.from_numpy(x[:9]).to(e.device), torch.from_numpy(x).to(e.device))     # 37-byte pitch: copied to 48
    assert np.array_equal(plain.cpu().numpy(), full[:9])


def test_sad_rows_more_db_tiles_than_one_grid_row(dlc):
    """Past 65 536 db tiles a workgroup walks several of them (the grid's x extent is capped): 256-row tiles at Q = 1
    against the oracle, 64-row tiles at Q = 64 against the same call on slices of the db that stay below the cap."""
    e = dlc.default_engine()
    rng = np.random.RandomState(21)
    n = 256 * 65536 + 300
    db = rng.randint(0, 256, size=(n, 1)).astype(np.uint8)
    q = np.array([[255]], dtype=np.uint8)
    dev = e._rows16_u8(torch.from_numpy(db).to(e.device), 1)
    got = e.sad_rows(torch.from_numpy(q).to(e.device), dev, d=1, limit0=n - 7).cpu().numpy()
    want = sq.sad_rows(q, db)
    want[0, n - 7:] = -1
    assert np.array_equal(got, want)
    n = 64 * 65536 + 100
    dev = dev[:n]
    qs = dev[rng.randint(0, n, size=64)].clone()
    whole = e.sad_rows(qs, dev, d=1)
    for lo in range(0, n, 1 << 21):
        assert torch.equal(whole[:, lo:lo + (1 << 21)], e.sad_rows(qs, dev[lo:lo + (1 << 21)], d=1)), lo
    assert np.array_equal(whole[:2].cpu().numpy(), sq.sad_rows(qs[:2, :1].cpu().numpy(), db[:n]))


def test_sad_rows_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    db = torch.zeros((50, 32), dtype=torch.uint8, device=e.device)
    qs = torch.zeros((4, 32), dtype=torch.uint8, device=e.device)
    out = torch.full((4, 50), -7, dtype=torch.int64, device=e.device)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def c_call(qp=vp(qs), ldq=32, dbp=vp(db), ldd=32, d=32, ld_out=50, o=vp(out)):
        return e.lib.dlc_sad_u8_rows(e.ctx, qp, 4, ldq, dbp, 50, ldd, d, 50, 0, o, ld_out, e._stream())
    for kw in (dict(qp=vp(qs, 1), d=16), dict(dbp=vp(db, 8), d=16), dict(ldq=24, d=16), dict(ldd=40), dict(ld_out=49),
               dict(d=0), dict(d=33), dict(qp=None), dict(o=None), dict(o=vp(out, 4))):
        rc = c_call(**kw)
        assert rc == _lib.DLC_ERR_BAD_ARG, kw
        with pytest.raises(ValueError):
            e._check(rc)
    assert e.lib.dlc_sad_u8_rows(e.ctx, vp(qs), 4, 1 << 25, vp(db), 50, 1 << 25, (1 << 24) + 1, 50, 0, vp(out), 50,
                                 e._stream()) == _lib.DLC_ERR_BAD_SHAPE
    for rows in ((1 << 20) + 1, 1 << 22):                             # Q > 2^20, as the header states it (refused before any read)
        assert e.lib.dlc_sad_u8_rows(e.ctx, vp(qs), rows, 32, vp(db), 50, 32, 32, 50, 0, vp(out), 50,
                                     e._stream()) == _lib.DLC_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert c_call() == _lib.DLC_OK
    torch.cuda.synchronize()
    assert not bool(out.any())
    for bad in (lambda: e.sad_rows(qs.to(torch.int8), db), lambda: e.sad_rows(qs, db.float()), lambda: e.sad_rows(qs[:, :16], db),
                lambda: e.sad_rows(qs, db, d=33), lambda: e.sad_rows(qs[0], db), lambda: e.sad_rows(qs.cpu(), db),
                lambda: e.sad_rows(qs, db, out=torch.zeros((4, 49), dtype=torch.int64, device=e.device)),
                lambda: e.sad_rows(qs, db, out=torch.zeros((4, 50), dtype=torch.int32, device=e.device))):
        with pytest.raises((ValueError, RuntimeError)):
            bad()
    for bad in (lambda: e.sad_rows(qs[0], db), lambda: e.sad_rows(qs[:, :16], db)):     # the message names the type it wants
        with pytest.raises(ValueError, match="sad_rows: .*(uint8|widths)"):
            bad()
    with pytest.raises(ValueError, match="2-D uint8"):
        e.sad_rows(qs.to(torch.int8), db)


# ---- 3. the Python surface ------------------------------------------------------------------------------------------------
SIZE, PATCH, STRENGTH = (24, 32), 8, 32


@pytest.fixture(scope="module")
def scene(dlc, golden_gray):
    """40 frames, 20 .. 39 exact repeats of 0 .. 19: (uint8 RGB frames, oracle descriptors [40, 768], oracle SAD matrix)."""
    frames = real_frames.tiled_u8_frames(dlc, 40)
    assert np.array_equal(frames[20:], frames[:20])
    desc = sq.describe(np.concatenate([golden_gray, golden_gray]), SIZE, PATCH, STRENGTH)
    return frames, desc, sq.sad_rows(desc, desc)


def test_seqslam_transform_routes_agree(dlc, scene, golden_gray):
    frames, desc, _ = scene
    net = dlc.SeqSlam(size=SIZE, patch=PATCH, strength=STRENGTH)
    assert net.dim == 768
    got = net.transform(frames[:20])
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, desc[:20])
    t = net.transform_tensor(torch.from_numpy(frames[:20]).to(net.engine.device))
    assert t.device == net.engine.device and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), got)
    assert np.array_equal(net.transform(golden_gray[:4]), desc[:4])    # grey frames as they are
    from deeploopcloser_amd import pipeline
    for src in (frames, torch.from_numpy(frames).to(net.engine.device)):
        assert np.array_equal(pipeline.seqslam_descriptors_from_frames(src, net, chunk_frames=16).cpu().numpy(), desc)
    with pytest.raises(ValueError):
        net.transform(frames[:2].astype(np.float32))


def test_difference_calculator_and_database(dlc, scene):
    _, desc, m = scene
    got = dlc.DifferenceCalculator.difference_matrix(desc)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, m)
    assert np.array_equal(dlc.DifferenceCalculator.difference_rows(desc[[7, 2]], desc), m[[7, 2]])
    with pytest.raises(ValueError):
        dlc.DifferenceCalculator.difference_rows(desc[:, :700], desc)
    dev = torch.from_numpy(desc).to(dlc.default_engine().device)      # both calls take tensors as they take arrays
    assert np.array_equal(dlc.DifferenceCalculator.difference_matrix(dev), m)
    assert np.array_equal(dlc.DifferenceCalculator.difference_rows(dev[[7, 2]], desc), m[[7, 2]])
    for bad in (desc.astype(np.int8), dev.to(torch.int8), dev[0], desc[0]):
        with pytest.raises(ValueError, match="uint8"):
            dlc.DifferenceCalculator.difference_matrix(bad)
        with pytest.raises(ValueError, match="uint8"):
            dlc.DifferenceCalculator.difference_rows(bad, desc)
    d2 = desc[:, :37]                                                  # a width that needs padding
    m2 = sq.sad_rows(d2, d2)
    db = dlc.SadKeyframeDatabase.empty(37, capacity=16)
    assert len(db) == 0 and db.capacity == 16
    db.append(d2[:10])
    assert db.append(d2[10:]) == (10, 40) and len(db) == 40 and db.capacity >= 40          # grown from 16
    assert tuple(db.rows.shape) == (40, 48) and db.rows.dtype == torch.uint8
    db.reserve(100)
    assert db.capacity == 100 and np.array_equal(db.rows[:, :37].cpu().numpy(), d2)
    rows = db.differences(d2[:9])
    assert rows.dtype == torch.int64 and rows.device == db.engine.device and np.array_equal(rows.cpu().numpy(), m2[:9])
    assert np.array_equal(db.differences(d2[0]).cpu().numpy(), m2[:1])
    lim = db.differences(d2[:9], limit0=35, limit_step=2).cpu().numpy()
    assert np.array_equal(lim, np.where(sq.offered(9, 40, 35, 2), m2[:9], -1)) and (lim == -1).any()
    assert np.array_equal(db.differences(db.rows[20:30]).cpu().numpy(), m2[20:30])         # stored rows as queries
    keep = torch.full((9, 50), -3, dtype=torch.int64, device=db.engine.device)
    assert db.differences(d2[:9], limit0=0, limit_step=5, out=keep[:, :40]).data_ptr() == keep.data_ptr()
    assert np.array_equal(keep[:, :40].cpu().numpy(), np.where(sq.offered(9, 40, 0, 5), m2[:9], -3))
    assert bool((keep[:, 40:] == -3).all())
    for bad in (lambda: db.differences(np.zeros((2, 38), np.uint8)), lambda: db.append(d2.astype(np.int8)),
                lambda: dlc.SadKeyframeDatabase.empty(0)):
        with pytest.raises(ValueError):
            bad()


# ---- 4. the detector ------------------------------------------------------------------------------------------------------
K_DET, EXCLUSION, L_SEQ = 3, 5, 4


def stream(det, x, batch):
    outs = [det.query_and_insert(x[lo:lo + batch]) for lo in range(0, x.shape[0], batch)]
    return tuple(torch.cat([o[t] for o in outs]).cpu().numpy() for t in range(len(outs[0])))


def expected(dlc, m, variant):
    """The oracle pipeline over the oracle SAD matrix m for one detector variant: (diff, ids[, chain])."""
    kw = dict(limit0=-EXCLUSION, limit_step=1, lower_is_better=True)
    if "sequence" not in variant:
        return po.peak_topk_rows(m, K_DET, variant.get("suppress", 0), **kw)
    offs = dlc.slope_offsets(L_SEQ)
    if "steps" in variant:
        s, i, _ = eo.elastic_topk(m, K_DET, L_SEQ, *variant["steps"], **kw)
        return s, i, ch.elastic_chains(m, i, L_SEQ, *variant["steps"], **kw)[0]
    if "contrast" in variant:
        return so.sequence_topk(co.contrast_rows(m, variant["contrast"], limit0=-EXCLUSION, limit_step=1), K_DET, L_SEQ, offs, **kw)[:2]
    if "suppress" in variant:
        return po.peak_topk_rows(so.sequence_scores(m, L_SEQ, offs, **kw)[0], K_DET, variant["suppress"], absent=-1, **kw)
    return so.sequence_topk(m, K_DET, L_SEQ, offs, **kw)[:2]


@pytest.mark.parametrize("variant", [dict(), dict(suppress=3), dict(sequence=L_SEQ), dict(sequence=L_SEQ, contrast=5),
                                     dict(sequence=L_SEQ, suppress=3), dict(sequence=L_SEQ, steps=(0, 2), chains=True)],
                         ids=lambda v: "-".join("%s%s" % kv for kv in v.items()) or "plain")
def test_detector(dlc, scene, variant):
    _, desc, m = scene
    want = expected(dlc, m, variant)
    for batch in (1, 7, 16):
        det = dlc.SeqSlamLoopClosureDetector(768, k=K_DET, exclusion=EXCLUSION, capacity=8, **variant)
        got = stream(det, desc, batch)
        assert len(det) == 40 and det.db.capacity >= 40 and len(got) == len(want)
        assert so.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), batch
        if len(want) == 3:
            assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), batch
    ids, diff = got[1], got[0]
    assert (ids[:EXCLUSION + 1] == -1).all()
    if variant.get("sequence") and "contrast" not in variant and "steps" not in variant:
        # frames 20 + i repeat frames i: from i = 3 on the line of four exact repeats is the first candidate, sum 0
        assert np.array_equal(ids[23:, 0], np.arange(3, 20)) and (diff[23:, 0] == 0).all() and diff.dtype == np.int64
    if not variant:
        assert np.array_equal(ids[20:, 0], np.arange(20)) and (diff[20:, 0] == 0).all()


def test_detector_loops_empty_batch_and_arguments(dlc, scene):
    _, desc, m = scene
    det = dlc.SeqSlamLoopClosureDetector(768, k=K_DET, exclusion=EXCLUSION, sequence=L_SEQ, max_difference=0)
    s, i = det.query_and_insert(desc[:0])
    assert tuple(s.shape) == (0, K_DET) and s.dtype == torch.int64
    found = []
    for lo in range(0, 40, 16):
        found += det.loops(*det.query_and_insert(desc[lo:lo + 16]), lo)
    assert found == [(20 + f, f, 0) for f in range(3, 20)]
    det = dlc.SeqSlamLoopClosureDetector(768, k=2, exclusion=EXCLUSION, sequence=L_SEQ, chains=True)
    s, i, chain = det.query_and_insert(desc[:0])
    assert tuple(chain.shape) == (0, 2, L_SEQ)
    s, i, chain = det.query_and_insert(desc)
    listed = det.loops(s, i, 0, chain)
    assert (39, 19, 0, [(36, 16), (37, 17), (38, 18), (39, 19)]) in listed
    for bad in (dict(k=0), dict(exclusion=-1), dict(max_difference=-1), dict(contrast=5), dict(steps=(0, 2)), dict(chains=True),
                dict(slopes=[[0, 1]]), dict(suppress=-1), dict(sequence=65)):
        with pytest.raises(ValueError):
            dlc.SeqSlamLoopClosureDetector(768, **bad)
    with pytest.raises(ValueError):
        dlc.SeqSlamLoopClosureDetector(0)


# ---- 5. driver and CLI ----------------------------------------------------------------------------------------------------
def test_create_difference_matrix(dlc, tmp_path):
    from oracle import patches as opatch
    from deeploopcloser_amd import drivers
    folder = os.path.join(GOLDEN, "datasets_test")
    files = sorted(os.listdir(folder))
    gray = np.stack([opatch.bgr2gray_opencv(dlc.read_ppm(os.path.join(folder, f))) for f in files])
    net = dlc.SeqSlam(size=SIZE, patch=PATCH, strength=STRENGTH)
    png = str(tmp_path / "difference.png")
    got = drivers.create_difference_matrix(folder, out_png=png, network=net)
    want_desc = sq.describe(gray, SIZE, PATCH, STRENGTH)
    assert got.dtype == np.int64 and np.array_equal(got, sq.sad_rows(want_desc, want_desc)) and os.path.getsize(png) > 0
    default = drivers.create_difference_matrix(folder)                 # SeqSlam(): 32 x 64
    d = sq.describe(gray, (32, 64), 8, 32)
    assert np.array_equal(default, sq.sad_rows(d, d))


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_seqslam(dlc):
    from oracle import patches as opatch
    res = run_cli("--network", "seqslam", "--metric", "sad", "--sequence", "3", "--exclusion", "2", "--k", "2", "--batch", "4",
                  "--size", "24x32", "--chains")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    lines = res.stdout.splitlines()
    loops = [l.split("\t") for l in lines if l.startswith("loop\t")]
    assert loops and all(int(l[1]) - int(l[3]) > 2 and int(l[1]) >= 2 + 2 + 1 for l in loops)   # old enough, a full line behind it
    assert sum(l.startswith("chain\t") for l in lines) == len(loops)
    # the lines are the oracle pipeline's
    folder = os.path.join(GOLDEN, "datasets_test")
    gray = np.stack([opatch.bgr2gray_opencv(dlc.read_ppm(os.path.join(folder, f))) for f in sorted(os.listdir(folder))])
    d = sq.describe(gray, (24, 32), 8, 32)
    s, i, _ = so.sequence_topk(sq.sad_rows(d, d), 2, 3, dlc.slope_offsets(3), limit0=-2, limit_step=1, lower_is_better=True)
    want = [(f, int(i[f, c]), int(s[f, c])) for f in range(17) for c in range(2) if i[f, c] >= 0]
    assert [(int(l[1]), int(l[3]), int(l[5])) for l in loops] == want
