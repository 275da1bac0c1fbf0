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
