"""GPU binary place descriptor: dlc_ldb_describe_u8 / Engine.ldb_describe, dlc_hamming_rows / Engine.hamming_rows, Ldb,
HammingCalculator, HammingKeyframeDatabase, LdbLoopClosureDetector, the pipeline, the driver, the CLI and the evaluator.
The reference is tests/ldb_oracle.py (the two definitions of include/dlc.h restated in NumPy) and, behind it, the existing
sequence / elastic / peaks / chains / contrast / track / evaluate oracles.  Every comparison is exact."""
import ctypes as C
import glob
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
import evaluate_oracle as ev
import ldb_oracle as lo
import peaks_oracle as po
import real_frames
import sequence_oracle as so
import track_oracle as to

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
    return np.stack([opatch.bgr2gray_opencv(dlc.read_ppm(p)) for p in real_frames.frame_paths()]).astype(np.uint8)


def describe(dlc, gray, size, levels, **kw):
    e = dlc.default_engine()
    return e.ldb_describe(torch.from_numpy(np.ascontiguousarray(gray)).to(e.device), size, levels, **kw).cpu().numpy()


def pad_bits(rows, levels):
    return np.unpackbits(rows, axis=1, bitorder="little")[:, lo.n_bits(levels):]


# ---- 1. describe ----------------------------------------------------------------------------------------------------------
def test_worked_example_of_the_header(dlc):
    t = np.array([[[1, 2, 5, 5], [3, 4, 5, 5], [9, 7, 0, 8], [9, 7, 8, 0]]], dtype=np.uint8)
    assert bytes(describe(dlc, t, (4, 4), (2,))[0]) == bytes([0xB6, 0x95, 0x00]) + bytes(13)


@pytest.mark.parametrize("size,levels", [((48, 48), (2, 3, 4)), ((24, 48), (2, 3, 4)), ((64, 64), (2, 4, 8))])
def test_describe_golden_frames(dlc, golden_gray, size, levels):
    got = describe(dlc, golden_gray, size, levels)
    want = lo.describe(golden_gray, size, levels)
    assert got.dtype == np.uint8 and got.shape == want.shape == (20, lo.row_bytes(levels)) and np.array_equal(got, want)
    assert not pad_bits(got, levels).any()
    m = lo.hamming_rows(want, want)
    assert m[~np.eye(20, dtype=bool)].min() > 0                        # ordinary codes: no two frames share one


# (H, W), (h, w), levels: a real resize with lane groups in both phases; the 1-pixel quadrant, 336 quadrants in two passes;
# the two largest grids on a thumbnail one pixel smaller than the frame; the two odd-sided grids 5 and 6 on a ragged
# resize; the largest thumbnail (64 KiB of LDS, the quadrant sums taking its place)
SHAPES = [((37, 53), (12, 12), (2, 3)), ((16, 16), (16, 16), (2, 4, 8)), ((113, 127), (112, 112), (7, 8)),
          ((61, 200), (60, 120), (5, 6)), ((256, 256), (256, 256), (8,))]


@pytest.mark.parametrize("shape,size,levels", SHAPES)
@pytest.mark.parametrize("frames", [1, 5])
def test_describe_shapes(dlc, shape, size, levels, frames):
    rng = np.random.RandomState(shape[0] * 31 + size[1] * 7 + frames)
    gray = rng.randint(0, 256, size=(frames,) + shape).astype(np.uint8)
    if frames == 5:
        gray[1] = rng.randint(100, 104, size=shape)                    # nearly flat: many ties
        gray[2] = gray[2] // 64 * 64                                   # four grey levels
    got = describe(dlc, gray, size, levels)
    assert np.array_equal(got, lo.describe(gray, size, levels))
    assert not pad_bits(got, levels).any() and got.any()


def test_describe_four_levels(dlc):
    """Four levels at once, up to three passes over the quadrants: (4, 5, 6, 8) has 564 of them and fits 240 x 240, the
    smallest side every 2 g divides.  ((5, 6, 7, 8) would need a side of 1680: no thumbnail of 65536 cells takes it.)"""
    rng = np.random.RandomState(5)
    gray = rng.randint(0, 256, size=(2, 250, 250)).astype(np.uint8)
    for size, levels in (((84, 84), (2, 3, 6, 7)), ((48, 240), (3, 4, 6, 8)), ((240, 240), (4, 5, 6, 8))):
        got = describe(dlc, gray, size, levels)
        assert np.array_equal(got, lo.describe(gray, size, levels)), levels
        assert not pad_bits(got, levels).any()
    with pytest.raises(ValueError):
        describe(dlc, gray, (240, 240), (5, 6, 7, 8))                  # 14 does not divide 240


def test_describe_constant_checkerboard_and_extremes(dlc):
    for v in (0, 77, 255):
        assert not describe(dlc, np.full((2, 37, 53), v, np.uint8), (12, 12), (2, 3)).any()
    board = (np.indices((16, 16)).sum(axis=0) % 2 * 255).astype(np.uint8)[None]
    # every quadrant of (2) and (4) holds as many 0 as 255, and every cell of (8) is the same 2 x 2 block: all cells tie
    assert not lo.describe(board, (16, 16), (2, 4, 8)).any() and not describe(dlc, board, (16, 16), (2, 4, 8)).any()
    board[0, 5, 9] = 128                                               # one pixel off: a handful of bits
    off = describe(dlc, board, (16, 16), (2, 4, 8))
    assert np.array_equal(off, lo.describe(board, (16, 16), (2, 4, 8))) and off.any()
    rng = np.random.RandomState(6)
    ext = np.zeros((4, 256, 256), np.uint8)
    ext[0, :, 128:] = 255                                              # whole cells of 0 and of 255: S differs, DX = DY = 0
    ext[1, :64] = 255
    ext[1, 128:192] = 255                                              # DY = -255 * 64 * 64 * 2 in every cell, the largest |sum|
    ext[2] = 255
    ext[3] = rng.randint(0, 2, size=(256, 256)) * 255
    got = describe(dlc, ext, (256, 256), (2,))
    assert np.array_equal(got, lo.describe(ext, (256, 256), (2,)))
    s, dx, dy = lo.cell_values(ext[1].astype(np.int64), 2)
    assert (dy == -255 * 64 * 128).all() and (s == 255 * 64 * 128).all()
    assert not got[2].any() and got[0].any() and got[3].any()


def test_describe_padding_survives(dlc, golden_gray):
    e = dlc.default_engine()
    gray = torch.from_numpy(golden_gray[:5]).to(e.device)
    want = lo.describe(golden_gray[:5], (48, 48), (2, 3, 4))
    for f in (5, 1):
        buf = torch.full((f, 64 + 16), 201, dtype=torch.uint8, device=e.device)               # ld_out = row_bytes + 16
        out = e.ldb_describe(gray[:f], (48, 48), (2, 3, 4), out=buf)
        assert out.data_ptr() == buf.data_ptr() and tuple(out.shape) == (f, 64)
        assert np.array_equal(out.cpu().numpy(), want[:f]) and bool((buf[:, 64:] == 201).all())
    wide = torch.full((5, 200), 7, dtype=torch.uint8, device=e.device)
    e.ldb_describe(gray, (48, 48), (2, 3, 4), out=wide[:, 3:90])       # a row-strided view on an odd base: ld_out = 200
    assert np.array_equal(wide[:, 3:67].cpu().numpy(), want)
    assert bool((wide[:, 67:] == 7).all()) and bool((wide[:, :3] == 7).all())


def test_describe_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    gray = torch.zeros((2, 300, 300), dtype=torch.uint8, device=e.device)
    out = torch.full((2, 2000), 9, dtype=torch.uint8, device=e.device)
    vp = lambda t: C.c_void_p(t.data_ptr())
    ints = lambda *v: (C.c_int * max(1, len(v)))(*v)

    def call(g=vp(gray), frames=2, H=300, W=300, h=48, w=48, lv=(2, 3, 4), n=None, o=vp(out), ld=2000):
        return e.lib.dlc_ldb_describe_u8(e.ctx, g, frames, H, W, h, w, None if lv is None else ints(*lv),
                                         len(lv) if n is None else n, o, ld, e._stream())
    arg, shape = _lib.DLC_ERR_BAD_ARG, _lib.DLC_ERR_BAD_SHAPE
    cases = [(dict(g=None), arg), (dict(o=None), arg), (dict(lv=None, n=1), arg), (dict(frames=0), arg),
             (dict(lv=(), n=0), arg), (dict(lv=(2, 3, 4, 6, 8)), arg), (dict(lv=(1,)), arg), (dict(lv=(9,)), arg),
             (dict(lv=(3, 2)), arg), (dict(lv=(2, 2)), arg), (dict(ld=63), arg),
             (dict(h=0), shape), (dict(w=0), shape), (dict(h=301, w=300, lv=(2,)), shape), (dict(h=48, w=304), shape),
             (dict(h=264, w=256, lv=(2,)), shape),                     # 67 584 cells
             (dict(H=4096, W=2048), shape),                            # 2^23 pixels (refused before anything is read)
             (dict(h=40), shape), (dict(w=36), shape),                 # 6 does not divide 40; 8 does not divide 36
             (dict(h=50, w=50, lv=(5, 8)), shape)]
    for kw, want in cases:
        rc = call(**kw)
        assert rc == want, kw
        with pytest.raises(ValueError):
            e._check(rc)
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                      # nothing was written
    assert call(h=256, w=256, lv=(8,), ld=768) == _lib.DLC_OK          # the limits themselves are inside
    assert call(ld=64) == _lib.DLC_OK
    torch.cuda.synchronize()
    for bad in (lambda: e.ldb_describe(gray.float(), (48, 48), (2,)), lambda: e.ldb_describe(gray[0], (48, 48), (2,)),
                lambda: e.ldb_describe(gray.cpu(), (48, 48), (2,)), lambda: e.ldb_describe(gray, (0, 48), (2,)),
                lambda: e.ldb_describe(gray, (48, 48), (3, 2)), lambda: e.ldb_describe(gray, (48, 48), ()),
                lambda: e.ldb_describe(gray, (48, 48), (2, 3, 4), out=out[:, :63]),
                lambda: e.ldb_describe(gray, (48, 48), (2, 3, 4), out=out[:1]),
                lambda: e.ldb_row_bytes((9,))):
        with pytest.raises(ValueError):
            bad()
    assert e.ldb_row_bytes((2, 3, 4)) == 64


# ---- 2. Hamming rows ------------------------------------------------------------------------------------------------------
NS, DS = (1, 63, 257), (1, 3, 4, 15, 16, 17, 64, 65, 176, 816)


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
    assert [tile_plan(q) for q in SWEEP_Q] == [(1, 256), (1, 256), (16, 256), (16, 256), (64, 64), (16, 256), (64, 64)]


@pytest.mark.parametrize("q", SWEEP_Q)
def test_hamming_rows_sweep(dlc, q):
    e = dlc.default_engine()
    rng = np.random.RandomState(q)
    for n in NS:
        for d in DS:
            qs = rng.randint(0, 256, size=(q, d)).astype(np.uint8)
            db = rng.randint(0, 256, size=(n, d)).astype(np.uint8)
            qs[-1], db[-1] = 0, 255                                    # all-zeros against all-ones: 8 bits a byte
            want = lo.hamming_rows(qs, db)
            assert want[-1, -1] == 8 * d
            dq, ddb = torch.from_numpy(padded_rows(rng, qs)).to(e.device), torch.from_numpy(padded_rows(rng, db)).to(e.device)
            sentinel = -(np.arange(q * (n + 3), dtype=np.int64).reshape(q, n + 3) * 2654435761 + 12345)
            for limit0, step in ((n, 0), (3, 1), (n, -1), (0, 0)):
                buf = torch.from_numpy(sentinel.copy()).to(e.device)
                out = e.hamming_rows(dq, ddb, d=d, limit0=limit0, limit_step=step, out=buf[:, :n])
                assert out.data_ptr() == buf.data_ptr()
                got = buf.cpu().numpy()
                offered = np.zeros((q, n + 3), bool)
                offered[:, :n] = lo.offered(q, n, limit0, step)
                assert np.array_equal(got[offered], want[offered[:, :n]]), (n, d, limit0, step)
                assert np.array_equal(got[~offered], sentinel[~offered]), (n, d, limit0, step)
            fresh = e.hamming_rows(dq, ddb, d=d, limit0=3, limit_step=1).cpu().numpy()   # engine-allocated: -1 where not offered
            assert np.array_equal(fresh, np.where(lo.offered(q, n, 3, 1), want, -1))
            assert np.array_equal(e.hamming_rows(dq, ddb, d=d).cpu().numpy(), want)


def test_hamming_rows_ones_against_zeros(dlc):
    e = dlc.default_engine()
    ones = torch.full((3, 816), 255, dtype=torch.uint8, device=e.device)
    zeros = torch.zeros((70, 816), dtype=torch.uint8, device=e.device)
    assert bool((e.hamming_rows(ones, zeros) == 6528).all()) and bool((e.hamming_rows(zeros, ones) == 6528).all())
    assert not bool(e.hamming_rows(ones, ones).any())


def test_hamming_rows_queries_may_be_db_rows_and_unpadded_rows(dlc):
    e = dlc.default_engine()
    rng = np.random.RandomState(8)
    x = rng.randint(0, 256, size=(300, 37)).astype(np.uint8)
    dev = torch.from_numpy(padded_rows(rng, x)).to(e.device)
    own = e.hamming_rows(dev[100:133], dev, d=37)
    assert np.array_equal(own.cpu().numpy(), lo.hamming_rows(x[100:133], x))
    full = e.hamming_rows(dev, dev, d=37).cpu().numpy()                # the Hamming matrix: symmetric, zero diagonal
    assert np.array_equal(full, full.T) and (np.diag(full) == 0).all() and np.array_equal(full, lo.hamming_rows(x, x))
    plain = e.hamming_rows(torch.from_numpy(x[:9]).to(e.device), torch.from_numpy(x).to(e.device))   # 37-byte pitch: copied to 48
    assert np.array_equal(plain.cpu().numpy(), full[:9])


def test_hamming_rows_more_db_tiles_than_one_grid_row(dlc):
    """Past 65 536 db tiles a workgroup walks several of them (the grid's x extent is capped): 256-row tiles at Q = 1
    against the oracle, 64-row tiles at Q = 64 against the same call on slices of the db that stay below the cap."""
    e = dlc.default_engine()
    rng = np.random.RandomState(21)
    n = 256 * 65536 + 300
    db = rng.randint(0, 256, size=(n, 1)).astype(np.uint8)
    q = np.array([[0x5A]], dtype=np.uint8)
    dev = e._rows16_u8(torch.from_numpy(db).to(e.device), 1)
    got = e.hamming_rows(torch.from_numpy(q).to(e.device), dev, d=1, limit0=n - 7).cpu().numpy()
    want = lo.hamming_rows(q, db)
    want[0, n - 7:] = -1
    assert np.array_equal(got, want)
    n = 64 * 65536 + 100
    dev = dev[:n]
    qs = dev[rng.randint(0, n, size=64)].clone()
    whole = e.hamming_rows(qs, dev, d=1)
    for first in range(0, n, 1 << 21):
        assert torch.equal(whole[:, first:first + (1 << 21)], e.hamming_rows(qs, dev[first:first + (1 << 21)], d=1)), first
    assert np.array_equal(whole[:2].cpu().numpy(), lo.hamming_rows(qs[:2, :1].cpu().numpy(), db[:n]))


def test_hamming_rows_bad_arguments(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    db = torch.zeros((50, 32), dtype=torch.uint8, device=e.device)
    qs = torch.full((4, 32), 255, dtype=torch.uint8, device=e.device)
    out = torch.full((4, 50), -7, dtype=torch.int64, device=e.device)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def c_call(qp=vp(qs), q=4, ldq=32, dbp=vp(db), n=50, ldd=32, d=32, ld_out=50, o=vp(out)):
        return e.lib.dlc_hamming_rows(e.ctx, qp, q, ldq, dbp, n, ldd, d, 50, 0, o, ld_out, e._stream())
    for kw in (dict(qp=vp(qs, 1), d=16), dict(dbp=vp(db, 8), d=16), dict(ldq=24, d=16), dict(ldd=40), dict(ld_out=49),
               dict(d=0), dict(d=33), dict(q=0), dict(n=0), dict(qp=None), dict(dbp=None), dict(o=None), dict(o=vp(out, 4))):
        rc = c_call(**kw)
        assert rc == _lib.DLC_ERR_BAD_ARG, kw
        with pytest.raises(ValueError):
            e._check(rc)
    for kw in (dict(ldq=1 << 25, ldd=1 << 25, d=(1 << 24) + 1), dict(q=(1 << 20) + 1), dict(q=1 << 22),
               dict(n=1 << 32, ld_out=1 << 32)):                       # refused before any read
        assert c_call(**kw) == _lib.DLC_ERR_BAD_SHAPE, kw
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert c_call() == _lib.DLC_OK
    torch.cuda.synchronize()
    assert bool((out == 256).all())
    for bad in (lambda: e.hamming_rows(qs.to(torch.int8), db), lambda: e.hamming_rows(qs, db.float()),
                lambda: e.hamming_rows(qs[:, :16], db), lambda: e.hamming_rows(qs, db, d=33), lambda: e.hamming_rows(qs[0], db),
                lambda: e.hamming_rows(qs.cpu(), db),
                lambda: e.hamming_rows(qs, db, out=torch.zeros((4, 49), dtype=torch.int64, device=e.device)),
                lambda: e.hamming_rows(qs, db, out=torch.zeros((4, 50), dtype=torch.int32, device=e.device))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="hamming_rows: .*2-D uint8"):
        e.hamming_rows(qs.to(torch.int8), db)


# ---- 3. the Python surface ------------------------------------------------------------------------------------------------
SIZE, LEVELS = (48, 48), (2, 3, 4)


@pytest.fixture(scope="module")
def scene(dlc, golden_gray):
    """40 frames, 20 .. 39 exact repeats of 0 .. 19: (uint8 RGB frames, oracle descriptors [40, 64], oracle Hamming matrix)."""
    frames = real_frames.tiled_u8_frames(dlc, 40)
    assert np.array_equal(frames[20:], frames[:20])
    desc = lo.describe(np.concatenate([golden_gray, golden_gray]), SIZE, LEVELS)
    return frames, desc, lo.hamming_rows(desc, desc)


def test_ldb_transform_routes_agree(dlc, scene, golden_gray):
    frames, desc, _ = scene
    net = dlc.Ldb()
    assert net.dim == 64 and net.n_bits == 486 and net.size == SIZE and net.levels == LEVELS
    assert dlc.Ldb(size=(64, 64), levels=(2, 4, 8)).dim == 816
    got = net.transform(frames[:20])
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, desc[:20])
    t = net.transform_tensor(torch.from_numpy(frames[:20]).to(net.engine.device))
    assert t.device == net.engine.device and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), got)
    assert np.array_equal(net.transform(golden_gray[:4]), desc[:4])    # grey frames as they are
    from deeploopcloser_amd import pipeline
    for src in (frames, torch.from_numpy(frames).to(net.engine.device)):
        assert np.array_equal(pipeline.ldb_descriptors_from_frames(src, net, chunk_frames=16).cpu().numpy(), desc)
    m = pipeline.ldb_hamming_matrix_from_frames(frames, net)
    assert isinstance(m, np.ndarray) and np.array_equal(m, scene[2])
    with pytest.raises(ValueError):
        net.transform(frames[:2].astype(np.float32))


def test_hamming_calculator_and_database(dlc, scene):
    _, desc, m = scene
    got = dlc.HammingCalculator.hamming_matrix(desc)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, m)
    assert np.array_equal(dlc.HammingCalculator.hamming_rows(desc[[7, 2]], desc), m[[7, 2]])
    with pytest.raises(ValueError):
        dlc.HammingCalculator.hamming_rows(desc[:, :60], desc)
    dev = torch.from_numpy(desc).to(dlc.default_engine().device)      # both calls take tensors as they take arrays
    assert np.array_equal(dlc.HammingCalculator.hamming_matrix(dev), m)
    assert np.array_equal(dlc.HammingCalculator.hamming_rows(dev[[7, 2]], desc), m[[7, 2]])
    for bad in (desc.astype(np.int8), dev.to(torch.int8), dev[0], desc[0]):
        with pytest.raises(ValueError, match="uint8"):
            dlc.HammingCalculator.hamming_matrix(bad)
        with pytest.raises(ValueError, match="uint8"):
            dlc.HammingCalculator.hamming_rows(bad, desc)
    d2 = desc[:, :37]                                                  # a width that needs padding
    m2 = lo.hamming_rows(d2, d2)
    db = dlc.HammingKeyframeDatabase.empty(37, capacity=16)
    assert len(db) == 0 and db.capacity == 16
    db.append(d2[:10])
    assert db.append(d2[10:]) == (10, 40) and len(db) == 40 and db.capacity >= 40          # grown from 16
    assert tuple(db.rows.shape) == (40, 48) and db.rows.dtype == torch.uint8
    db.reserve(100)
    assert db.capacity == 100 and np.array_equal(db.rows[:, :37].cpu().numpy(), d2)
    rows = db.distances(d2[:9])
    assert rows.dtype == torch.int64 and rows.device == db.engine.device and np.array_equal(rows.cpu().numpy(), m2[:9])
    assert np.array_equal(db.distances(d2[0]).cpu().numpy(), m2[:1])
    lim = db.distances(d2[:9], limit0=35, limit_step=2).cpu().numpy()
    assert np.array_equal(lim, np.where(lo.offered(9, 40, 35, 2), m2[:9], -1)) and (lim == -1).any()
    assert np.array_equal(db.distances(db.rows[20:30]).cpu().numpy(), m2[20:30])           # stored rows as queries
    keep = torch.full((9, 50), -3, dtype=torch.int64, device=db.engine.device)
    assert db.distances(d2[:9], limit0=0, limit_step=5, out=keep[:, :40]).data_ptr() == keep.data_ptr()
    assert np.array_equal(keep[:, :40].cpu().numpy(), np.where(lo.offered(9, 40, 0, 5), m2[:9], -3))
    assert bool((keep[:, 40:] == -3).all())
    for bad in (lambda: db.distances(np.zeros((2, 38), np.uint8)), lambda: db.append(d2.astype(np.int8)),
                lambda: dlc.HammingKeyframeDatabase.empty(0)):
        with pytest.raises(ValueError):
            bad()


# ---- 4. the detector ------------------------------------------------------------------------------------------------------
K_DET, EXCLUSION, L_SEQ = 3, 5, 4


def stream(det, x, batch):
    outs = [det.query_and_insert(x[first:first + batch]) for first in range(0, x.shape[0], batch)]
    return tuple(torch.cat([o[t] for o in outs]).cpu().numpy() for t in range(len(outs[0])))


def expected(dlc, m, variant):
    """The oracle pipeline over the oracle Hamming matrix m for one detector variant: (dist, ids[, chain])."""
    kw = dict(limit0=-EXCLUSION, limit_step=1, lower_is_better=True)
    if "sequence" not in variant:
        return po.peak_topk_rows(m, K_DET, variant.get("suppress", 0), **kw)
    length = variant["sequence"]
    offs = dlc.slope_offsets(length)
    if "steps" in variant:
        s, i, _ = eo.elastic_topk(m, K_DET, length, *variant["steps"], **kw)
        return s, i, ch.elastic_chains(m, i, length, *variant["steps"], **kw)[0]
    if "contrast" in variant:
        return so.sequence_topk(co.contrast_rows(m, variant["contrast"], limit0=-EXCLUSION, limit_step=1), K_DET, length, offs, **kw)[:2]
    if "suppress" in variant:
        return po.peak_topk_rows(so.sequence_scores(m, length, offs, **kw)[0], K_DET, variant["suppress"], absent=-1, **kw)
    if variant.get("chains"):
        s, i, _ = so.sequence_topk(m, K_DET, length, offs, **kw)
        return s, i, ch.line_chains(m, i, length, offs, **kw)[0]
    return so.sequence_topk(m, K_DET, length, offs, **kw)[:2]


TRACK = dict(steps=(0, 2), jump=40, gate=40, null_score=40)


@pytest.mark.parametrize("variant", [dict(), dict(suppress=3), dict(sequence=L_SEQ), dict(sequence=L_SEQ, contrast=5),
                                     dict(sequence=L_SEQ, suppress=3), dict(sequence=L_SEQ, steps=(0, 2), chains=True),
                                     dict(sequence=L_SEQ, chains=True), dict(sequence=1, track=TRACK)],
                         ids=lambda v: "-".join("%s%s" % (k, "" if isinstance(x, dict) else x) for k, x in v.items()) or "plain")
def test_detector(dlc, scene, variant):
    _, desc, m = scene
    want = expected(dlc, m, {k: v for k, v in variant.items() if k != "track"})
    for batch in (1, 7, 40):
        det = dlc.LdbLoopClosureDetector(64, k=K_DET, exclusion=EXCLUSION, capacity=8, **variant)
        got = stream(det, desc, batch)
        assert len(det) == 40 and det.db.capacity >= 40 and len(got) == len(want)
        assert so.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), batch
        if len(want) == 3:
            assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), batch
        if "track" in variant:
            path = to.track_places(m, lower_is_better=True, limit0=-EXCLUSION, limit_step=1, **TRACK)[1]
            assert np.array_equal(det.tracker.path().cpu().numpy(), path), batch
            assert (path[:20] == -1).all() and (path[20:] == np.arange(20)).all()      # no loop, then the repeat is followed
        else:
            assert det.tracker is None
    ids, dist = got[1], got[0]
    assert (ids[:EXCLUSION + 1] == -1).all()
    if variant.get("sequence") == L_SEQ and "contrast" not in variant and "steps" not in variant:
        # frames 20 + i repeat frames i: from i = 3 on the line of four exact repeats is the first candidate, sum 0
        assert np.array_equal(ids[23:, 0], np.arange(3, 20)) and (dist[23:, 0] == 0).all() and dist.dtype == np.int64
    if not variant:
        assert np.array_equal(ids[20:, 0], np.arange(20)) and (dist[20:, 0] == 0).all()


def test_detector_loops_empty_batch_and_arguments(dlc, scene):
    _, desc, m = scene
    det = dlc.LdbLoopClosureDetector(64, k=K_DET, exclusion=EXCLUSION, sequence=L_SEQ, max_distance=0)
    assert det.max_distance == 0
    s, i = det.query_and_insert(desc[:0])
    assert tuple(s.shape) == (0, K_DET) and s.dtype == torch.int64
    found = []
    for first in range(0, 40, 16):
        found += det.loops(*det.query_and_insert(desc[first:first + 16]), first)
    assert found == [(20 + f, f, 0) for f in range(3, 20)]
    det = dlc.LdbLoopClosureDetector(64, k=2, exclusion=EXCLUSION, sequence=L_SEQ, chains=True)
    s, i, chain = det.query_and_insert(desc[:0])
    assert tuple(chain.shape) == (0, 2, L_SEQ)
    s, i, chain = det.query_and_insert(desc)
    assert (39, 19, 0, [(36, 16), (37, 17), (38, 18), (39, 19)]) in det.loops(s, i, 0, chain)
    for bad in (dict(k=0), dict(exclusion=-1), dict(max_distance=-1), dict(contrast=5), dict(steps=(0, 2)), dict(chains=True),
                dict(slopes=[[0, 1]]), dict(suppress=-1), dict(sequence=65), dict(track=TRACK)):
        with pytest.raises(ValueError):
            dlc.LdbLoopClosureDetector(64, **bad)
    with pytest.raises(ValueError):
        dlc.LdbLoopClosureDetector(0)
    with pytest.raises(TypeError):
        dlc.LdbLoopClosureDetector(64, shift=1, width=8)               # no lateral shift here
    # the SeqSLAM detector, which shares the body, keeps its own names
    sad = dlc.SeqSlamLoopClosureDetector(768, max_difference=7, shift=2, width=32)
    assert sad.max_difference == 7 and sad.shift == 2 and sad.width == 32 and not hasattr(sad, "max_distance")


# ---- 5. driver, CLI, evaluator --------------------------------------------------------------------------------------------
def folder_gray(dlc):
    from oracle import patches as opatch
    folder = os.path.join(GOLDEN, "datasets_test")
    return folder, np.stack([opatch.bgr2gray_opencv(dlc.read_ppm(os.path.join(folder, f)))
                             for f in sorted(os.listdir(folder))]).astype(np.uint8)


def test_create_hamming_matrix(dlc, tmp_path):
    from deeploopcloser_amd import drivers
    folder, gray = folder_gray(dlc)
    png = str(tmp_path / "hamming.png")
    got = drivers.create_hamming_matrix(folder, out_png=png)           # Ldb(): 48 x 48, (2, 3, 4)
    d = lo.describe(gray, SIZE, LEVELS)
    assert got.dtype == np.int64 and np.array_equal(got, lo.hamming_rows(d, d)) and os.path.getsize(png) > 0
    other = drivers.create_hamming_matrix(folder, network=dlc.Ldb(size=(64, 64), levels=(2, 4, 8)))
    d = lo.describe(gray, (64, 64), (2, 4, 8))
    assert np.array_equal(other, lo.hamming_rows(d, d))


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_ldb(dlc):
    res = run_cli("--network", "ldb")
    assert res.returncode == 2 and "error: --network ldb and --metric hamming need each other" in res.stderr
    res = run_cli("--network", "ldb", "--metric", "hamming", "--sequence", "3", "--exclusion", "2", "--k", "2", "--batch", "4",
                  "--chains")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "frames\t17\tkey-frames\t17" in res.stderr
    lines = res.stdout.splitlines()
    loops = [l.split("\t") for l in lines if l.startswith("loop\t")]
    assert loops and all(int(l[1]) - int(l[3]) > 2 and int(l[1]) >= 2 + 2 + 1 for l in loops)   # old enough, a full line behind it
    assert sum(l.startswith("chain\t") for l in lines) == len(loops)
    # the lines are the oracle pipeline's, at the defaults 48x48 and 2,3,4
    _, gray = folder_gray(dlc)
    d = lo.describe(gray, SIZE, LEVELS)
    s, i, _ = so.sequence_topk(lo.hamming_rows(d, d), 2, 3, dlc.slope_offsets(3), limit0=-2, limit_step=1, lower_is_better=True)
    want = [(f, int(i[f, c]), int(s[f, c])) for f in range(17) for c in range(2) if i[f, c] >= 0]
    assert [(int(l[1]), int(l[3]), int(l[5])) for l in loops] == want


def test_evaluator_on_the_ldb_detector(dlc):
    """A planted route: 17 real frames said to pass the same six places again and again."""
    from deeploopcloser_amd import pipeline
    files = sorted(glob.glob(os.path.join(GOLDEN, "datasets_test", "*.ppm")))
    positions, radius, exclusion = [t % 6 for t in range(len(files))], 1, 2
    desc = pipeline.ldb_descriptors_from_frames(np.stack([dlc.read_ppm(f) for f in files]), dlc.Ldb())
    for k, batch in ((1, 4), (3, 5)):
        det = dlc.LdbLoopClosureDetector(desc.shape[1], k=k, exclusion=exclusion, capacity=64)
        judge = dlc.LoopClosureEvaluator(np.array(positions), radius, exclusion, lower_is_better=True)
        lists = []
        for first in range(0, len(files), batch):
            s, i = det.query_and_insert(desc[first:first + batch])
            judge.add(s, i, first)
            lists.append((s.cpu().numpy(), i.cpu().numpy(), first))
        curve, candidates_recall = judge.result()
        flags = [ev.detector_flags(positions, radius, exclusion, first, i) for _, i, first in lists]
        hit, any_hit, has = (np.concatenate([f[c] for f in flags]) for c in range(3))
        t, tp, fp, positives = ev.queries_curve(np.concatenate([s[:, 0] for s, _, _ in lists]),
                                                np.concatenate([i[:, 0] for _, i, _ in lists]), hit, has, True)
        assert judge.queries == len(files) and positives == has.sum() > 0 and len(t) > 1
        assert np.array_equal(curve.thresholds, t) and np.array_equal(curve.tp, tp) and np.array_equal(curve.fp, fp)
        assert curve.positives == positives and candidates_recall == any_hit.sum() / has.sum()
        assert curve.average_precision == ev.average_precision(tp, fp, positives)
