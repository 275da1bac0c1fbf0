"""DA / SDA training on the GPU (dlc_salt_pepper_mask_f64, dlc_da_corrupt_f64, dlc_da_train_step; DA, SDA, the
train_sdav command line) against the fp64 NumPy restatement in tests/da_oracle.py."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import da_oracle as od
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DATASET = os.path.join(GOLDEN, "datasets_test")


def close(a, b, rel):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= rel * max(1.0, np.abs(b).max())


@pytest.fixture(scope="module")
def frames():
    """The 17 frames of the test dataset, parsed (sorted order, Harris key-points)."""
    from deeploopcloser_amd.input import load_frames
    f = load_frames(os.path.join(DATASET, "*.ppm"), [30, 1681])
    assert len(f) == 17
    return f


@pytest.mark.parametrize("n", [1, 7, 50430, 504300, 750000])
@pytest.mark.parametrize("level", [0.0, 0.3, 1.0])
def test_salt_pepper_mask(n, level):
    import deeploopcloser_amd as dlc
    eng = dlc.default_engine()
    nz, mean, sd = od.salt_pepper_counts(n, level)
    zeros = torch.empty(n, dtype=torch.float64, device=eng.device)
    ones = torch.empty_like(zeros)
    eng.salt_pepper_mask(zeros, ones, nz, 11, 3)
    z, o = zeros.cpu().numpy(), ones.cpu().numpy()
    assert set(np.unique(z)) <= {0.0, 1.0} and set(np.unique(o)) <= {0.0, 1.0}
    assert int((z == 0).sum()) == nz                            # exactly int(n * level) zeros
    assert not np.any((o == 1) & (z == 1))                      # salt only where the zeros are
    assert abs(int(o.sum()) - mean) <= 5 * sd
    z2, o2 = torch.empty_like(zeros), torch.empty_like(zeros)
    eng.salt_pepper_mask(z2, o2, nz, 11, 3)
    assert np.array_equal(z2.cpu().numpy(), z) and np.array_equal(o2.cpu().numpy(), o)
    if n > 100 and nz > 0:                                      # another counter: other bits
        eng.salt_pepper_mask(z2, o2, nz, 11, 4)
        if nz < n:
            assert not np.array_equal(z2.cpu().numpy(), z)
        assert not np.array_equal(o2.cpu().numpy(), o)


def np_salt_pepper(rng, rows, cols, level=0.3):
    """(zeros, ones) [rows, cols] in NumPy: int(rows * cols * level) zeros, salt on a random half of them (rounded up)."""
    n = rows * cols
    at = rng.permutation(n)[:int(n * level)]
    zeros, ones = np.ones(n), np.zeros(n)
    zeros[at] = 0.0
    ones[at[:(len(at) + 1) // 2]] = 1.0
    return zeros.reshape(rows, cols), ones.reshape(rows, cols)


def raw_corrupt(eng, x, zeros, ones, rows, cols, out, ldo):
    """dlc_da_corrupt_f64 itself (Engine.da_corrupt only ever passes ldo = even_pitch(cols)); returns the status."""
    return eng.lib.dlc_da_corrupt_f64(eng.ctx, x.data_ptr(), zeros.data_ptr(), ones.data_ptr(), rows, cols, out.data_ptr(), ldo,
                                      eng._stream())


GUARD = 1024        # doubles of NaN in front of and behind `out`


@pytest.mark.parametrize("pad", [0, 1, 7])
@pytest.mark.parametrize("rows,cols", [(1, 1), (300, 1681), (300, 2500), (7, 37)])
def test_da_corrupt_any_pitch(rows, cols, pad):
    """x~ = zeros * x + ones at every pitch the header allows (ldo >= cols): bit for bit NumPy's, the columns
    cols .. ldo - 1 exactly 0.0 where NaN stood, and not one double written in front of out or behind rows * ldo."""
    import deeploopcloser_amd as dlc
    eng = dlc.default_engine()
    rng = np.random.RandomState(rows * 7 + cols + pad)
    x = rng.uniform(0, 1, size=(rows, cols))
    if rows * cols > 4:
        x.flat[rng.choice(rows * cols, 4, replace=False)] = [0.0, 1.0, -3.5, 1e-300]
    zeros, ones = np_salt_pepper(rng, rows, cols, 0.3 if rows * cols > 1 else 1.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    ldo = cols + pad
    buf = torch.full((GUARD + rows * ldo + GUARD,), float("nan"), dtype=torch.float64, device=eng.device)
    out = buf[GUARD:GUARD + rows * ldo]
    assert raw_corrupt(eng, dev(x), dev(zeros), dev(ones), rows, cols, out, ldo) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + rows * ldo:]).all(), "written outside rows * ldo"
    got = got[GUARD:GUARD + rows * ldo].reshape(rows, ldo)
    want = x * zeros + ones
    assert np.array_equal(got[:, :cols], want)
    assert np.array_equal(got[:, cols:], np.zeros((rows, pad)))
    assert np.any(want != x * zeros) or rows * cols == 1 and want[0, 0] == 1.0         # (there is salt in the case)


@pytest.mark.parametrize("rows,cols", [(1, 1), (300, 1681), (300, 2500), (7, 37)])
def test_da_corrupt_in_place(rows, cols):
    """out == x is allowed where ldo == cols (every element is read and written by the one thread that owns it; dlc.h
    says so); with a pitch of its own the rows of out would overwrite rows of x not yet read: refused, x untouched."""
    import deeploopcloser_amd as dlc
    from deeploopcloser_amd import _lib as L
    eng = dlc.default_engine()
    rng = np.random.RandomState(rows + cols)
    x = rng.uniform(0, 1, size=(rows, cols))
    zeros, ones = np_salt_pepper(rng, rows, cols, 0.3 if rows * cols > 1 else 1.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    buf = torch.full((GUARD + rows * (cols + 1) + GUARD,), float("nan"), dtype=torch.float64, device=eng.device)
    xd = buf[GUARD:GUARD + rows * cols]
    xd.copy_(dev(x).reshape(-1))
    assert raw_corrupt(eng, xd, dev(zeros), dev(ones), rows, cols, xd, cols + 1) == L.DLC_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().reshape(rows, cols), x)
    assert raw_corrupt(eng, xd, dev(zeros), dev(ones), rows, cols, xd, cols) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[GUARD:GUARD + rows * cols].reshape(rows, cols), x * zeros + ones)
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + rows * cols:]).all()


def test_salt_is_fair_and_apart_from_the_zeros():
    """The reference's sizes (n = 750 000, level 0.3) over 16 counters.  Every bound is 5 standard deviations of the
    distribution the header promises, computed here: the salt bits fair coins (binomial), the zeros of two counters two
    independent uniform subsets (their overlap hypergeometric: mean nz^2 / n), the salt bit independent of the parity of
    its index and of whether the next element is a zero (binomial within each group)."""
    import deeploopcloser_amd as dlc
    eng = dlc.default_engine()
    n, counters = 750000, 16
    nz, _, _ = od.salt_pepper_counts(n, 0.3)
    zeros = torch.empty(n, dtype=torch.float64, device=eng.device)
    ones = torch.empty_like(zeros)
    zs, salts = [], []
    for c in range(counters):
        eng.salt_pepper_mask(zeros, ones, nz, 11, c)
        z, o = zeros.cpu().numpy() == 0.0, ones.cpu().numpy() == 1.0
        assert int(z.sum()) == nz and not np.any(o & ~z)
        zs.append(z)
        salts.append(o)
    half_sd = lambda m: 5.0 * np.sqrt(m) / 2.0                    # 5 sd of Binomial(m, 1/2)
    pooled = dict(salt=0, parity=0, next_zero=0, next_zero_n=0)
    idx_odd = (np.arange(n) & 1) == 1
    for c, (z, o) in enumerate(zip(zs, salts)):
        s = int(o.sum())
        assert abs(s - nz / 2.0) <= half_sd(nz), (c, s)
        agree = int((o[z] == idx_odd[z]).sum())                   # salt bit == index parity, over the zeros
        assert abs(agree - nz / 2.0) <= half_sd(nz), (c, agree)
        nxt = np.zeros(n, dtype=bool)
        nxt[:-1] = z[1:]                                          # the next element is a zero
        for grp in (z & nxt, z & ~nxt):
            m, k = int(grp.sum()), int(o[grp].sum())
            assert abs(k - m / 2.0) <= half_sd(m), (c, m, k)
        pooled["salt"] += s
        pooled["parity"] += agree
        pooled["next_zero"] += int(o[z & nxt].sum())
        pooled["next_zero_n"] += int((z & nxt).sum())
    assert abs(pooled["salt"] - counters * nz / 2.0) <= half_sd(counters * nz)
    assert abs(pooled["parity"] - counters * nz / 2.0) <= half_sd(counters * nz)
    assert abs(pooled["next_zero"] - pooled["next_zero_n"] / 2.0) <= half_sd(pooled["next_zero_n"])
    # two counters' zero sets: hypergeometric overlap
    p = nz / float(n)
    mean, sd = nz * p, np.sqrt(nz * p * (1.0 - p) * (n - nz) / (n - 1.0))
    for a in range(counters):
        for b in range(a + 1, counters):
            ov = int((zs[a] & zs[b]).sum())
            assert abs(ov - mean) <= 5.0 * sd, (a, b, ov, mean, sd)
            # ... and their salt: where both drew a zero, the two salt bits agree half the time
            both = zs[a] & zs[b]
            eq = int((salts[a][both] == salts[b][both]).sum())
            assert abs(eq - ov / 2.0) <= half_sd(ov), (a, b, eq, ov)


SENTINEL = -12345.678


def test_c_abi_refusals():
    """Each documented refusal of dlc_da_train_step, dlc_da_train_workspace_bytes, dlc_salt_pepper_mask_f64 and
    dlc_da_corrupt_f64 returns its dlc_status and leaves every output as it was."""
    import deeploopcloser_amd as dlc
    from deeploopcloser_amd import _lib as L
    eng = dlc.default_engine()
    lib, ctx, st = eng.lib, eng.ctx, eng._stream()
    batch, p, k, n = 4, 5, 37, 21
    rows, kp = batch * p, eng.even_pitch(k)
    f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=eng.device)
    x, xt, w, be, bd, loss = f(rows, k), f(rows, kp), f(k, n), f(n), f(k), f(4)
    need = lib.dlc_da_train_workspace_bytes(batch, p, k, n)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=eng.device)

    def step(batch_=batch, x_=x, xt_=xt, w_=w, be_=be, bd_=bd, ws_=ws, ws_bytes=need):
        ptr = lambda t: t.data_ptr() if t is not None else None
        return lib.dlc_da_train_step(ctx, batch_, p, k, n, ptr(x_), ptr(xt_), ptr(w_), ptr(be_), ptr(bd_), 0.05, 1.0, 0.2, 0.1,
                                     loss.data_ptr(), ptr(ws_), ws_bytes, st)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all().item()) for t in (x, xt, w, be, bd, loss)) and not bool(ws.any().item())

    assert step(batch_=1) == L.DLC_ERR_BAD_SHAPE and untouched()
    assert step(batch_=0) == L.DLC_ERR_BAD_SHAPE and untouched()
    for null in ("x_", "xt_", "w_", "be_", "bd_"):
        assert step(**{null: None}) == L.DLC_ERR_BAD_ARG and untouched(), null
    assert step(ws_bytes=need - 1) == L.DLC_ERR_WORKSPACE and untouched()
    assert step(ws_=None) == L.DLC_ERR_WORKSPACE and untouched()
    assert b"workspace" in lib.dlc_last_error(ctx)
    for bad in ((1, p, k, n), (0, p, k, n), (-3, p, k, n), (batch, 0, k, n), (batch, p, 0, n), (batch, p, k, 0), (batch, p, k, -1)):
        assert lib.dlc_da_train_workspace_bytes(*bad) == 0, bad
    with pytest.raises(ValueError):
        eng.da_train_workspace(1, p, k, n)

    # dlc_salt_pepper_mask_f64
    m = 64
    z, o = f(m), f(m)
    mask = lambda z_, o_, n_, nz_: lib.dlc_salt_pepper_mask_f64(ctx, z_.data_ptr(), o_.data_ptr(), n_, nz_, 1, 2, st)
    clean = lambda *ts: (torch.cuda.synchronize(), all(bool((t == SENTINEL).all().item()) for t in ts))[1]
    assert mask(z, z, m, 3) == L.DLC_ERR_BAD_ARG and clean(z, o)                # zeros == ones
    assert mask(z, o, m, m + 1) == L.DLC_ERR_BAD_ARG and clean(z, o)            # n_zeros > n
    assert mask(z, o, m, -1) == L.DLC_ERR_BAD_ARG and clean(z, o)
    assert mask(z, o, 0, 0) == L.DLC_ERR_BAD_ARG and clean(z, o)
    big = (1 << 26) + 1                                                         # (tensors of that size: were the refusal
    zb = torch.empty(big, dtype=torch.float64, device=eng.device)               #  ever lost, nothing is written out of bounds)
    ob = torch.empty(big, dtype=torch.float64, device=eng.device)
    zb[:4096] = SENTINEL; ob[:4096] = SENTINEL
    zb[-4096:] = SENTINEL; ob[-4096:] = SENTINEL
    assert mask(zb, ob, big, big // 3) == L.DLC_ERR_BAD_SHAPE
    assert clean(zb[:4096], ob[:4096], zb[-4096:], ob[-4096:])
    del zb, ob
    assert mask(z, o, m, 19) == 0                                               # (the same call within the limits runs)
    torch.cuda.synchronize()
    assert int((z == 0).sum().item()) == 19

    # dlc_da_corrupt_f64
    out = f(rows, kp)
    zz, oo = torch.ones_like(x), torch.zeros_like(x)
    assert raw_corrupt(eng, x, zz, oo, rows, k, out, k - 1) == L.DLC_ERR_BAD_ARG and clean(out)
    assert raw_corrupt(eng, x, zz, oo, 0, k, out, kp) == L.DLC_ERR_BAD_ARG and clean(out)
    assert raw_corrupt(eng, x, zz, oo, rows, k, out, kp) == 0
    torch.cuda.synchronize()
    assert bool((out[:, :k] == SENTINEL).all().item()) and bool((out[:, k:] == 0).all().item())


@pytest.mark.parametrize("shape", [(4, 5, 37, 21), (10, 30, 1681, 2500), (10, 30, 2500, 2500)])
def test_da_step_vs_oracle(shape):
    import deeploopcloser_amd as dlc
    batch, p, k, n = shape
    da = dlc.DA([p, k], n, batch_size=batch, seed=5)
    rng = np.random.RandomState(k)
    x = rng.uniform(0, 1, size=(batch, p, k))
    w0 = rng.standard_normal((k, n)) * (0.4 if k < 100 else 0.02)
    b0, b1 = rng.standard_normal(n) * 0.1, rng.standard_normal(k) * 0.1
    da.set_weights(w0, b0, b1)
    zeros, ones = (m.cpu().numpy() for m in da.corruption_masks())
    assert zeros.shape == (batch * p, k) and int((zeros == 0).sum()) == int(batch * p * k * 0.3)
    (want, (w1, be1, bd1)) = od.sgd_step(x, zeros, ones, w0, b0, b1, lr=0.1, **dict(sparse_level=0.05, sparse_penalty=1.0,
                                                                                     consecutive_penalty=0.2))
    loss = da.train_step(x).cpu().numpy()
    assert close(loss, want, 1e-9), (loss, want)
    w, be, bd = da.get_weights()
    assert close(w, w1, 1e-9) and close(be, be1, 1e-9) and close(bd, bd1, 1e-9)
    assert da.global_step == 1
    with pytest.raises(ValueError):
        da.train_step(x[:batch - 1])                            # not batch_size frames: the masks' shape


def test_train_steps_replay_is_train_step():
    import deeploopcloser_amd as dlc
    rng = np.random.RandomState(1)
    x = rng.uniform(0, 1, size=(10, 30, 1681))
    a = dlc.DA([30, 1681], 64, seed=2)
    b = dlc.DA([30, 1681], 64, seed=2)
    masks = [m.cpu().numpy() for m in a.corruption_masks()]
    la = [a.train_step(x).cpu().numpy() for _ in range(5)][-1]
    lb = b.train_steps(x, 5).cpu().numpy()
    assert np.array_equal(la, lb)
    for u, v in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(u, v)
    assert a.global_step == b.global_step == 5
    for m, m1 in zip(masks, b.corruption_masks()):             # the static masks are left as drawn
        assert np.array_equal(m, m1.cpu().numpy())
    # a new learning rate between calls is honoured by the replayed path (a new capture)
    a.learning_rate = b.learning_rate = 0.05
    for _ in range(4):
        a.train_step(x)
    b.train_steps(x, 4)
    for u, v in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(u, v)


def test_da_fit_dataset_vs_oracle(frames, caplog):
    import deeploopcloser_amd as dlc
    da = dlc.DA([30, 1681], 48, batch_size=4, epochs=3, seed=7)
    w0, b0, b1 = da.get_weights()
    zeros, ones = (m.cpu().numpy() for m in da.corruption_masks())
    with caplog.at_level(logging.WARNING):
        da.fit_dataset(frames)
    assert da.global_step == 12                                 # 4 full batches x 3 epochs; the 17th frame is skipped
    assert any("Ignored last batch" in r.getMessage() for r in caplog.records)
    batches = [np.stack(frames[i:i + 4]) for i in range(0, 17, 4)]
    w, be, bd, steps = od.fit_batches(batches, zeros, ones, w0, b0, b1, 3, lr=0.1)
    assert steps == 12
    for got, want in zip(da.get_weights(), (w, be, bd)):
        assert close(got, want, 1e-8)


def test_sda_greedy_fit_and_transform(frames, tmp_path):
    import deeploopcloser_amd as dlc
    sda = dlc.SDA([30, 1681], [64, 32], batch_size=4, epochs=2, seed=3)
    sda.fit_dataset(frames)
    assert [l.global_step for l in sda.layers] == [8, 8]
    # layer 1 of the stack = a standalone DA of the same seed trained on layer 0's transform of the same frames
    h0 = sda.layers[0].transform_tensor(np.stack(frames)).cpu().numpy().reshape(17, 30, 64)
    da1 = dlc.DA([30, 64], 32, batch_size=4, epochs=2, layer_n=1, seed=3)
    da1.fit_dataset(list(h0))
    for got, want in zip(sda.layers[1].get_weights(), da1.get_weights()):
        assert close(got, want, 1e-9)
    # transform = the SDAV chain with the SDA's weights
    x = np.stack(frames)
    d = sda.transform(x)
    assert d.shape == (510, 32)
    net = dlc.SDAV(hidden_units=[64, 32])
    ws = sda.get_weights()
    net.set_weights([w for w, _, _ in ws], [b for _, b, _ in ws])
    assert close(d, net.transform(x), 1e-12)
    # persistence
    sda.save_weights(str(tmp_path / "s.npz"))
    other = dlc.SDA([30, 1681], [64, 32], batch_size=4, epochs=2, seed=99)
    other.load_weights(str(tmp_path / "s.npz"))
    assert np.array_equal(other.transform(x), d)


def test_train_sdav_cli(frames, tmp_path):
    import deeploopcloser_amd as dlc
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--dataset_dir", DATASET, "--dataset_ext", "ppm", "--hidden_units", "64", "32", "--batch_size", "4",
              "--epochs", "2"]
    prefix = str(tmp_path / "P")
    r = subprocess.run([sys.executable, "-m", "deeploopcloser_amd.train_sdav", "train"] + common + ["--save", prefix],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Layer:1 Batch:3 fit, Epoch:2/2, Loss:" in r.stderr
    saved = prefix + "-layer1.npz"
    assert os.path.exists(prefix + "-layer0.npz") and os.path.exists(saved)
    out = str(tmp_path / "d.npy")
    r = subprocess.run([sys.executable, "-m", "deeploopcloser_amd.train_sdav", "transform"] + common +
                       ["--load", saved, "--out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(out)
    assert d.shape == (510, 32)
    sda = dlc.SDA([30, 1681], [64, 32], batch_size=4, epochs=2)
    sda.load_weights(saved)
    assert close(d, sda.transform(np.stack(frames)), 1e-12)
