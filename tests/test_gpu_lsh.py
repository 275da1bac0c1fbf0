"""GPU sign-random-projection hashes (dlc_lsh_quantize_i8 and dlc_lsh_hash_i8 through the raw C ABI; Engine.lsh_quantize /
lsh_hash, Lsh, HashedLoopClosureDetector and the CLI on top) against the NumPy restatement of the definitions
(tests/lsh_oracle.py, pinned by test_lsh_cpu.py).  Every sum is an exact integer and every rounding is stated, so all
comparisons are `==` on the bytes.  Operands carry garbage in their padding bytes, which would change the codes if it
were read; outputs sit in poisoned buffers wider than what may be written."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import lsh_oracle as lo

pytestmark = pytest.mark.gpu

AUTO, ONE_PASS, SPLIT = lo.AUTO, lo.ONE_PASS, lo.SPLIT
BF16, F16, F32, F64 = 0, 1, 2, 3
BAD_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -5
POISON = 0xA5
DTYPES = {"f64": (torch.float64, F64), "f32": (torch.float32, F32), "bf16": (torch.bfloat16, BF16)}


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def e(dlc):
    return dlc.default_engine()


def p(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


def dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def padded_i8(e, m, rng, extra=16):
    """m int8 [rows, D] as the first D columns of a [rows, ceil16(D) + extra] device matrix whose other bytes are random
    garbage (-128 and 127 among them)."""
    ld = (m.shape[1] + 15) // 16 * 16 + extra
    buf = rng.randint(-128, 128, size=(m.shape[0], ld)).astype(np.int8)
    buf[:, m.shape[1]], buf[:, m.shape[1] + 1] = -128, 127
    buf[:, :m.shape[1]] = m
    return dev(e, buf)


def raw_hash(e, qb, D, pb, bits, plan, extra=5):
    """dlc_lsh_hash_i8 into a poisoned [rows, row_bytes + extra] buffer -> (its first row_bytes columns, the rest)."""
    rows, nb = qb.shape[0], lo.row_bytes(bits)
    out = torch.full((rows, nb + extra), POISON, dtype=torch.uint8, device=e.device)
    need = e.lib.dlc_lsh_hash_workspace_bytes(rows, D, bits, plan)
    ws = torch.empty(need, dtype=torch.uint8, device=e.device) if need else None
    rc = e.lib.dlc_lsh_hash_i8(e.ctx, p(qb), rows, D, qb.stride(0), p(pb), bits, pb.stride(0), p(out), out.stride(0), plan, p(ws),
                               need, None)
    assert rc == 0, e.lib.dlc_last_error(e.ctx)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return got[:, :nb], got[:, nb:]


def plans_for(rows):
    return (AUTO, ONE_PASS, SPLIT) if rows <= lo.SPLIT_MAX_ROWS else (AUTO, ONE_PASS)


def operands(rng, rows, bits, D, kind):
    if kind == "pm1":
        return (rng.randint(0, 2, size=(rows, D)) * 2 - 1).astype(np.int8), (rng.randint(0, 2, size=(bits, D)) * 2 - 1).astype(np.int8)
    q, pl = rng.randint(-128, 128, size=(rows, D)).astype(np.int8), rng.randint(-128, 128, size=(bits, D)).astype(np.int8)
    q.flat[0] = pl.flat[0] = -128
    return q, pl


# ---- 1. the worked examples and the operand layout -------------------------------------------------------------------------
def test_worked_examples(dlc, e):
    x = torch.tensor([[0.5, -1.0, 0.25, 0.0]], dtype=torch.float64, device=e.device)
    q = e.lsh_quantize(x)
    assert q.dtype == torch.int8 and q.cpu().tolist() == [[64, -127, 32, 0]]
    planes = np.array([[1, 1, 1, 1], [-1, 1, 1, -1], [1, 1, -1, -1], [1, -1, 1, 1]], dtype=np.int8)
    qq = np.array([[3, -2, 0, 1]], dtype=np.int8)
    code = e.lsh_hash(dev(e, qq), dev(e, planes))
    assert code.dtype == torch.uint8 and code.cpu().tolist() == [[0x09] + [0] * 15]
    assert e.lsh_row_bytes(4) == 16 and e.lsh_row_bytes(8192) == 1024
    # the raw C ABI: quantise into a poisoned pitched buffer, then hash under every plan
    out = torch.full((1, 16), 0x5A, dtype=torch.int8, device=e.device)
    assert e.lib.dlc_lsh_quantize_i8(e.ctx, F64, p(x), 1, 4, 4, None, p(out), 16, None) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[64, -127, 32, 0] + [0x5A] * 12]
    rng = np.random.RandomState(0)
    for plan in (AUTO, ONE_PASS, SPLIT):
        got, rest = raw_hash(e, padded_i8(e, qq, rng), 4, padded_i8(e, planes, rng), 4, plan)
        assert got.tolist() == [[0x09] + [0] * 15] and (rest == POISON).all(), plan


@pytest.mark.parametrize("rows", [1, 37, 150])
def test_layout_signed_identity_asymmetric_rows(e, rows):
    """Planes are rows of a signed identity and q[r][d] = ((3 r + 5 d) % 11) - 5 is asymmetric: bit (r, t) is q[r][t] > 0
    under +1 and q[r][t] < 0 under -1.  A row / column swap or a k map that differs between the operands fails here."""
    D = 200
    q = ((3 * np.arange(rows)[:, None] + 5 * np.arange(D)[None, :]) % 11 - 5).astype(np.int8)
    sign = np.where(np.arange(D) % 3 == 0, -1, 1).astype(np.int8)
    rng = np.random.RandomState(rows)
    for planes, want in ((np.eye(D, dtype=np.int8), q > 0), (np.eye(D, dtype=np.int8) * sign[:, None], q * sign[None, :] > 0)):
        for plan in plans_for(rows):
            got, rest = raw_hash(e, padded_i8(e, q, rng), D, padded_i8(e, planes, rng), D, plan)
            on = np.unpackbits(got, axis=1, bitorder="little")
            assert np.array_equal(on[:, :D], want.astype(np.uint8)) and not on[:, D:].any() and (rest == POISON).all(), plan
            assert np.array_equal(got, lo.hash_rows(q, planes))


# ---- 2. quantise -----------------------------------------------------------------------------------------------------------
def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float64).numpy()


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_quantize_against_the_oracle(e, dtype, with_mean):
    tdt, code = DTYPES[dtype]
    rng = np.random.RandomState(7)
    ties = np.array([127.0, 0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5])              # m = 127, s = 1: .5 ties of both parities
    for rows in (1, 5, 70):
        for D in (1, 63, 64, 65, 1000, 4097):
            mean = None
            if with_mean:                                                         # representable in every dtype, 0 under the ties
                mean = bf16_round(rng.standard_normal(D))
                mean[:8] = 0.0
            x = rng.standard_normal((rows, D)) * 3.0
            special = rows >= 5
            if special:
                x[1] = 0.0 if mean is None else mean                              # t = 0 everywhere
                x[2, D // 2] = np.nan
                x[3, D - 1] = -np.inf
                if D >= 8:
                    x[4] = rng.uniform(-100, 100, size=D)
                    x[4, :8] = ties
            xb = torch.full((rows, D + 3), float("nan"), dtype=tdt, device=e.device)          # pitched, NaN past D
            xb[:, :D] = torch.from_numpy(x).to(e.device).to(tdt)
            stored = xb[:, :D].to(torch.float64).cpu().numpy()                    # what the kernel reads, exactly
            want = lo.quantize(stored, mean)
            if special:
                assert not want[1:4].any() and want[0].any()
                if D >= 8:
                    assert want[4, :8].tolist() == [127, 0, 2, 2, 4, 0, -2, -2]
            mu = dev(e, mean) if mean is not None else None
            out = torch.full((rows, D + 5), 0x5A, dtype=torch.int8, device=e.device)
            rc = e.lib.dlc_lsh_quantize_i8(e.ctx, code, p(xb), rows, D, xb.stride(0), p(mu), p(out), out.stride(0), None)
            assert rc == 0, e.lib.dlc_last_error(e.ctx)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[:, :D], want) and (got[:, D:] == 0x5A).all(), (rows, D)
            # the engine: the pitched view as it is, and into a caller-kept wider buffer
            assert np.array_equal(e.lsh_quantize(xb[:, :D], mu).cpu().numpy(), want)
            keep = torch.full((rows, D + 2), 0x33, dtype=torch.int8, device=e.device)
            view = e.lsh_quantize(xb[:, :D], mu, out=keep)
            assert view.data_ptr() == keep.data_ptr() and np.array_equal(view.cpu().numpy(), want) and (keep[:, D:] == 0x33).all()
    assert e.lsh_quantize(torch.tensor([[5e-324, -5e-324, 0.0]], dtype=torch.float64, device=e.device)).cpu().tolist() == [[127, -127, 0]]


# ---- 3. hash ---------------------------------------------------------------------------------------------------------------
CROSS_SECTION = [(1, 1, 1), (1, 7, 15), (15, 8, 16), (16, 127, 63), (17, 128, 64), (130, 129, 65), (17, 1000, 200), (1, 1000, 4099),
                 (130, 7, 4099), (16, 129, 200), (15, 1000, 64), (130, 128, 16), (1, 129, 15), (17, 7, 1), (16, 1, 4099), (130, 1000, 63)]


@pytest.mark.parametrize("kind", ["pm1", "full"])
def test_hash_against_the_oracle(e, kind):
    rng = np.random.RandomState(11)
    for rows, bits, D in CROSS_SECTION:
        q, pl = operands(rng, rows, bits, D, kind)
        want = lo.hash_rows(q, pl)
        qb, pb = padded_i8(e, q, rng), padded_i8(e, pl, rng)
        for plan in plans_for(rows):
            got, rest = raw_hash(e, qb, D, pb, bits, plan)
            assert np.array_equal(got, want), (rows, bits, D, plan)
            assert (rest == POISON).all(), (rows, bits, D, plan)
        on = np.unpackbits(want, axis=1, bitorder="little")
        assert not on[:, bits:].any()
        assert np.array_equal(e.lsh_hash(dev(e, q), dev(e, pl)).cpu().numpy(), want)          # the engine pads the rows itself


def test_hash_many_rows_the_large_tile(e):
    """Enough rows that the 128 x 128 workgroup tile is taken (4101 rows x 8 bit tiles), with a row tail, a bit tail and a
    K tail."""
    rng = np.random.RandomState(12)
    rows, bits, D = 4101, 1000, 203
    q, pl = operands(rng, rows, bits, D, "full")
    want = lo.hash_rows(q, pl)
    for plan in (AUTO, ONE_PASS):
        got, rest = raw_hash(e, padded_i8(e, q, rng), D, padded_i8(e, pl, rng), bits, plan)
        assert np.array_equal(got, want) and (rest == POISON).all(), plan


def test_hash_planted_sums_zero_plus_one_minus_one(e):
    """Sums of exactly 0, +1 and -1 -- also as chunk sums that cancel: 0 and -1 give bit 0, +1 gives bit 1."""
    rng = np.random.RandomState(3)
    for D in (129, 2 * lo.CHUNK + 1):
        q = np.ones((2, D), dtype=np.int8)
        q[1] *= 100
        q[:, D - 1] = 1
        half = (D - 1) // 2
        base = np.concatenate([np.ones(half), -np.ones(half)]).astype(np.int8)    # the first D - 1 columns cancel
        pl = np.stack([np.append(base, 0), np.append(base, 1), np.append(base, -1), np.append(-base, 1), np.append(-base, -1)]).astype(np.int8)
        assert lo.sums(q, pl).tolist() == [[0, 1, -1, 1, -1]] * 2
        want = lo.hash_rows(q, pl)
        assert want[:, 0].tolist() == [0b01010, 0b01010]
        for plan in (AUTO, ONE_PASS, SPLIT):
            got, _ = raw_hash(e, padded_i8(e, q, rng), D, padded_i8(e, pl, rng), 5, plan)
            assert np.array_equal(got, want), (D, plan)


def test_hash_overflow_edge(e):
    """D = DLC_LSH_MAX_D, every product 16384 or -16256: |S| reaches 2 147 467 264 < 2^31."""
    D = lo.MAX_D
    rng = np.random.RandomState(4)
    q = np.full((1, D), -128, dtype=np.int8)
    pl = np.concatenate([np.full((4, D), -128), np.full((4, D), 127)]).astype(np.int8)
    assert lo.sums(q, pl)[0, 0] == 128 * 128 * D < 2 ** 31 and lo.sums(q, pl)[0, 7] == -128 * 127 * D > -2 ** 31
    qb, pb = padded_i8(e, q, rng), padded_i8(e, pl, rng)
    for plan in (AUTO, ONE_PASS, SPLIT):
        got, rest = raw_hash(e, qb, D, pb, 8, plan)
        assert got[0].tolist() == [0x0F] + [0] * 15 and (rest == POISON).all(), plan


@pytest.mark.parametrize("D", [lo.CHUNK - 37, lo.CHUNK, lo.CHUNK + 100, 3 * lo.CHUNK])
def test_plans_give_the_same_bytes(e, D):
    rng = np.random.RandomState(D)
    rows, bits = 64, 200
    q, pl = operands(rng, rows, bits, D, "full")
    want = lo.hash_rows(q, pl)
    qb, pb = padded_i8(e, q, rng), padded_i8(e, pl, rng)
    for plan in (AUTO, ONE_PASS, SPLIT):
        assert np.array_equal(raw_hash(e, qb, D, pb, bits, plan)[0], want), plan
    assert np.array_equal(e.lsh_hash(qb[:, :D], pb[:, :D], plan="split").cpu().numpy(), want)
    assert np.array_equal(e.lsh_hash(qb[:, :D], pb[:, :D], bits=77, plan="one_pass").cpu().numpy(), lo.hash_rows(q, pl[:77]))


def test_workspace_bytes(e):
    ws = e.lib.dlc_lsh_hash_workspace_bytes
    for rows in (1, 17, 64, 65, 1000):
        for D in (1, 4096, lo.CHUNK, lo.CHUNK + 1, 75000, lo.MAX_D):
            for bits in (1, 128, 1000, 8192):
                chunks = -(-D // lo.CHUNK)
                assert ws(rows, D, bits, ONE_PASS) == 0
                if rows <= lo.SPLIT_MAX_ROWS:
                    assert ws(rows, D, bits, SPLIT) >= rows * chunks * bits * 4
                else:
                    assert ws(rows, D, bits, SPLIT) == 0                           # refused
                assert ws(rows, D, bits, AUTO) == ws(rows, D, bits, lo.auto_plan(rows, D))
    assert ws(1, 75000, 1024, AUTO) > 0 and ws(1, 4096, 1024, AUTO) == 0 and ws(65, 75000, 1024, AUTO) == 0
    for bad in ((0, 8, 8, SPLIT), (1, 0, 8, SPLIT), (1, 8, 0, SPLIT), (1, lo.MAX_D + 1, 8, SPLIT), (1, 8, lo.MAX_BITS + 1, SPLIT),
                (1 << 31, 8, 8, SPLIT), (1, 8, 8, 3)):
        assert ws(*bad) == 0
    assert [e.lib.dlc_lsh_row_bytes(b) for b in (-1, 0, 1, 128, 129, 8192, 8193)] == [0, 0, 16, 16, 32, 1024, 0]


def test_a_row_alone_equals_itself_in_a_batch(e):
    rng = np.random.RandomState(5)
    rows, bits, D = 130, 1000, 4099
    q, pl = operands(rng, rows, bits, D, "full")
    qb, pb = padded_i8(e, q, rng), padded_i8(e, pl, rng)
    batch, _ = raw_hash(e, qb, D, pb, bits, AUTO)
    assert np.array_equal(batch, lo.hash_rows(q, pl))
    for r in (0, 77, 129):
        for plan in (AUTO, ONE_PASS, SPLIT):
            alone, _ = raw_hash(e, qb[r:r + 1], D, pb, bits, plan)
            assert np.array_equal(alone[0], batch[r]), (r, plan)


def test_refused_arguments_write_nothing(e):
    rng = np.random.RandomState(6)
    rows, bits, D = 8, 130, 100
    q, pl = operands(rng, rows, bits, D, "full")
    qb, pb = padded_i8(e, q, rng), padded_i8(e, pl, rng)
    nb = lo.row_bytes(bits)
    out = torch.full((rows, nb), POISON, dtype=torch.uint8, device=e.device)
    ws = torch.full((e.lib.dlc_lsh_hash_workspace_bytes(rows, D, bits, SPLIT) + 16,), POISON, dtype=torch.uint8, device=e.device)
    before = [t.clone() for t in (qb, pb, ws)]

    def call(**kw):
        a = dict(q=p(qb), rows=rows, D=D, ldq=qb.stride(0), pl=p(pb), bits=bits, ldp=pb.stride(0), o=p(out), ld_out=nb, plan=SPLIT,
                 w=p(ws), wb=ws.numel() - 16)
        a.update(kw)
        return e.lib.dlc_lsh_hash_i8(e.ctx, a["q"], a["rows"], a["D"], a["ldq"], a["pl"], a["bits"], a["ldp"], a["o"], a["ld_out"],
                                     a["plan"], a["w"], a["wb"], None)

    cases = [
        (dict(q=None), BAD_ARG), (dict(pl=None), BAD_ARG), (dict(o=None), BAD_ARG), (dict(q=p(qb, 8)), BAD_ARG), (dict(pl=p(pb, 1)), BAD_ARG),
        (dict(rows=0), BAD_ARG), (dict(rows=-1), BAD_ARG), (dict(D=0), BAD_ARG), (dict(bits=0), BAD_ARG), (dict(ldq=96), BAD_ARG),
        (dict(ldq=D), BAD_ARG), (dict(ldq=qb.stride(0) + 8), BAD_ARG), (dict(ldp=96), BAD_ARG), (dict(ldp=pb.stride(0) + 4), BAD_ARG),
        (dict(ld_out=nb - 1), BAD_ARG), (dict(plan=3), BAD_ARG), (dict(plan=-1), BAD_ARG),
        (dict(o=p(qb)), BAD_ARG), (dict(o=p(pb, 16)), BAD_ARG),                                # out overlaps an input
        (dict(D=lo.MAX_D + 1, ldq=lo.MAX_D + 1, ldp=lo.MAX_D + 1), BAD_SHAPE), (dict(bits=lo.MAX_BITS + 1, ld_out=2048), BAD_SHAPE),
        (dict(rows=1 << 31, plan=ONE_PASS), BAD_SHAPE), (dict(rows=lo.SPLIT_MAX_ROWS + 1), BAD_SHAPE),
        (dict(w=None), WORKSPACE), (dict(wb=0), WORKSPACE), (dict(wb=ws.numel() - 17 - 255), WORKSPACE), (dict(w=p(ws, 8)), WORKSPACE),
    ]
    for kw, want in cases:
        assert call(**kw) == want, kw
        assert e.lib.dlc_last_error(e.ctx)
    # quantise: a float64 matrix, its mean and a poisoned destination
    x = dev(e, rng.standard_normal((rows, D)))
    mu = dev(e, rng.standard_normal(D))
    qo = torch.full((rows, D), 0x5A, dtype=torch.int8, device=e.device)
    x0, mu0 = x.clone(), mu.clone()

    def quant(**kw):
        a = dict(dt=F64, x=p(x), rows=rows, D=D, ldx=D, mu=p(mu), q=p(qo), ldq=D)
        a.update(kw)
        return e.lib.dlc_lsh_quantize_i8(e.ctx, a["dt"], a["x"], a["rows"], a["D"], a["ldx"], a["mu"], a["q"], a["ldq"], None)

    for kw, want in [(dict(x=None), BAD_ARG), (dict(q=None), BAD_ARG), (dict(dt=F16), BAD_ARG), (dict(dt=4), BAD_ARG), (dict(dt=-1), BAD_ARG),
                     (dict(x=p(x, 4)), BAD_ARG), (dict(mu=p(mu, 4)), BAD_ARG), (dict(x=p(x, 2), dt=F32), BAD_ARG), (dict(x=p(x, 1), dt=BF16), BAD_ARG),
                     (dict(rows=0), BAD_ARG), (dict(D=0), BAD_ARG), (dict(ldx=D - 1), BAD_ARG), (dict(ldq=D - 1), BAD_ARG),
                     (dict(q=p(x)), BAD_ARG), (dict(q=p(mu, 8)), BAD_ARG),
                     (dict(D=lo.MAX_D + 1, ldx=lo.MAX_D + 1, ldq=lo.MAX_D + 1), BAD_SHAPE), (dict(rows=1 << 31), BAD_SHAPE)]:
        assert quant(**kw) == want, kw
    torch.cuda.synchronize()
    assert (out == POISON).all() and (qo == 0x5A).all()
    for t, b in zip((qb, pb, ws), before):
        assert torch.equal(t, b)
    assert torch.equal(x.view(torch.int64), x0.view(torch.int64)) and torch.equal(mu.view(torch.int64), mu0.view(torch.int64))
    # and the calls they were derived from are accepted
    assert call() == 0 and call(plan=ONE_PASS, w=None, wb=0) == 0 and quant() == 0 and quant(mu=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), lo.hash_rows(q, pl))
    assert np.array_equal(qo.cpu().numpy(), lo.quantize(x.cpu().numpy(), None))
    # the engine refuses in its own words
    for bad in (lambda: e.lsh_hash(qb[:, :D], pb[:, :D], plan="fast"), lambda: e.lsh_hash(qb[:, :D], pb[:, :D - 1]),
                lambda: e.lsh_hash(qb[:, :D], pb[:, :D], bits=bits + 1), lambda: e.lsh_hash(qb[:, :D].to(torch.uint8), pb[:, :D]),
                lambda: e.lsh_hash(qb[:, :D], pb[:, :D], out=torch.empty((rows, nb - 1), dtype=torch.uint8, device=e.device)),
                lambda: e.lsh_hash(qb[:1].expand(65, -1)[:, :D], pb[:, :D], plan="split"),
                lambda: e.lsh_quantize(x.to(torch.float16)), lambda: e.lsh_quantize(x, mu[:-1]), lambda: e.lsh_quantize(x.cpu()),
                lambda: e.lsh_quantize(x, out=torch.empty((rows, D - 1), dtype=torch.int8, device=e.device)), lambda: e.lsh_row_bytes(0)):
        with pytest.raises(ValueError):
            bad()


# ---- 4. Lsh ----------------------------------------------------------------------------------------------------------------
def test_lsh_fit_transform_save_load(dlc, e, tmp_path):
    rng = np.random.RandomState(8)
    train, x = rng.standard_normal((50, 333)) + 2.0, rng.standard_normal((9, 333)) + 2.0
    h = dlc.Lsh(n_bits=200, seed=5).fit(train)
    assert (h.n_bits, h.dim, h.width, h.seed) == (200, 32, 333, 5)
    mean = h.mean.cpu().numpy()
    assert np.abs(mean - train.mean(axis=0)).max() < 1e-12                        # (the defined mean is not NumPy's, bit for bit)
    planes = lo.planes(200, 333, 5)
    assert np.array_equal(h.planes.cpu().numpy(), planes) and np.array_equal(dlc.lsh_planes(200, 333, 5), planes)
    want = lo.hash_rows(lo.quantize(x, mean), planes)
    got = h.transform(x)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    for plan in ("auto", "one_pass", "split"):
        assert np.array_equal(h.transform_tensor(dev(e, x), plan=plan).cpu().numpy(), want)
    for tdt in (torch.float32, torch.bfloat16):                                   # narrower rows: hashed from what they hold
        xt = dev(e, x).to(tdt)
        assert np.array_equal(h.transform_tensor(xt).cpu().numpy(), lo.hash_rows(lo.quantize(xt.to(torch.float64).cpu().numpy(), mean), planes))
    # into rows of a Hamming key-frame store
    db = dlc.HammingKeyframeDatabase.empty(h.dim, capacity=16)
    first, _ = db.append(torch.zeros((9, h.dim), dtype=torch.uint8, device=e.device))
    view = h.transform_tensor(dev(e, x), out=db.rows[first:first + 9])
    assert np.array_equal(db.rows[:9, :h.dim].cpu().numpy(), want) and view.data_ptr() == db.rows.data_ptr()
    assert np.array_equal(db.distances(dev(e, want)).cpu().numpy(), lo.hamming(want, want))
    # save / load
    path = str(tmp_path / "lsh.npz")
    h.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["mean", "n_bits", "seed", "width"] and int(z["seed"]) == 5 and int(z["n_bits"]) == 200
        assert int(z["width"]) == 333 and np.array_equal(z["mean"], mean)
    again = dlc.Lsh.load(path)
    assert (again.n_bits, again.width, again.seed, again.center) == (200, 333, 5, True) and np.array_equal(again.transform(x), want)
    # int8 rows pass through as they are; a model that is not centred learns only the width
    raw = dlc.Lsh(n_bits=200, seed=5, center=False).fit(train)
    assert raw.mean is None and raw.width == 333
    qi = rng.randint(-128, 128, size=(9, 333)).astype(np.int8)
    assert np.array_equal(raw.transform(qi), lo.hash_rows(qi, planes))
    assert np.array_equal(raw.transform(x), lo.hash_rows(lo.quantize(x), planes))
    raw.save(path)
    again = dlc.Lsh.load(path)
    assert again.mean is None and not again.center and np.array_equal(again.transform(qi), lo.hash_rows(qi, planes))
    for bad in (lambda: h.transform(qi), lambda: h.transform(x[:, :-1]), lambda: dlc.Lsh(n_bits=0), lambda: dlc.Lsh(n_bits=8193),
                lambda: dlc.Lsh().transform(x), lambda: dlc.Lsh().save(path), lambda: dlc.Lsh(seed=-1)):
        with pytest.raises(ValueError):
            bad()


# ---- 5. HashedLoopClosureDetector --------------------------------------------------------------------------------------------
def stream(det, rows, batch):
    outs = [det.query_and_insert(rows[first:first + batch]) for first in range(0, len(rows), batch)]
    return [torch.cat(t).cpu().numpy() for t in zip(*outs)]


@pytest.fixture(scope="module")
def planted(dlc):
    base, again = lo.planted_stream(places=40, d=200, amplitude=0.25, seed=0)
    h = dlc.Lsh(n_bits=256, seed=0).fit(base)
    rows = np.concatenate([base, again])
    codes = lo.hash_rows(lo.quantize(rows, h.mean.cpu().numpy()), lo.planes(256, 200, 0))
    return h, rows, codes


@pytest.mark.parametrize("variant", [dict(), dict(sequence=4), dict(sequence=3, chains=True, suppress=2)])
def test_hashed_detector_is_the_ldb_detector_on_the_codes(dlc, planted, variant):
    h, rows, codes = planted
    want = stream(dlc.LdbLoopClosureDetector(h.dim, k=3, exclusion=10, capacity=16, **variant), torch.from_numpy(codes), 80)
    for batch in (1, 7):
        det = dlc.HashedLoopClosureDetector(h, k=3, exclusion=10, capacity=16, **variant)
        got = stream(det, rows, batch)
        assert len(det) == 80 and len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (batch, variant)
        assert np.array_equal(det.db.rows[:80, :h.dim].cpu().numpy(), codes)
    if not variant:                                                               # every revisit finds its place
        assert (want[1][40:, 0] == np.arange(40)).all()
        assert det.loops(torch.from_numpy(want[0][40:41]), torch.from_numpy(want[1][40:41]), 40)[0][:2] == (40, 0)
    s, i, *_ = det.query_and_insert(rows[:0])
    assert tuple(s.shape) == (0, 3) and len(det) == 80
    with pytest.raises(ValueError):
        dlc.HashedLoopClosureDetector(h, k=0)
    with pytest.raises(ValueError):
        dlc.HashedLoopClosureDetector(32)


# ---- 6. the CLI ------------------------------------------------------------------------------------------------------------
def run_module(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd." + module, os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_train_lsh_then_loop_closure(dlc, tmp_path):
    model = str(tmp_path / "lsh.npz")
    res = run_module("train_lsh", "--bits", "256", "--seed", "3", "--save", model)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout == "lsh\trows\t17\twidth\t75000\tbits\t256\tbytes\t32\tcentered\t1\n"
    with np.load(model) as z:
        assert int(z["seed"]) == 3 and int(z["n_bits"]) == 256 and int(z["width"]) == 75000
        assert z["mean"].shape == (75000,) and z["mean"].dtype == np.float64 and np.isfinite(z["mean"]).all()
    runs = [run_module("loop_closure", "--network", "sdav", "--metric", "cosine", "--hash", model, "--exclusion", "2", "--k", "2",
                       "--sequence", "2", "--batch", batch) for batch in ("4", "17")]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
        assert "frames\t17\tkey-frames\t17" in r.stderr
        lines = r.stdout.splitlines()
        assert lines and all(l.startswith("loop\t") and len(l.split("\t")) == 6 for l in lines)
        for l in lines:
            _, frame, _, match, _, dist = l.split("\t")
            assert 0 <= int(match) < int(frame) - 2 and 0 <= int(dist) <= 2 * 256
    assert runs[0].stdout == runs[1].stdout
    # a model of another width is refused with both widths
    other = str(tmp_path / "other.npz")
    dlc.Lsh(n_bits=64, center=False).fit(np.zeros((1, 123))).save(other)
    r = run_module("loop_closure", "--network", "sdav", "--metric", "cosine", "--hash", other)
    assert r.returncode == 2 and "--hash: its rows are 123 wide, the frame descriptor 75000" in r.stderr and r.stdout == ""
    r = run_module("train_lsh", "--bits", "8193", "--save", other)
    assert r.returncode == 2 and "--bits must be 1..8192" in r.stderr
