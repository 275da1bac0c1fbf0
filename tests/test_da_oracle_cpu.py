"""CPU checks of the DA / SDA training surface: the fp64 DA-step oracle (tests/da_oracle.py) against torch autograd and
central finite differences, its sparsity denominator by hand, the train_sdav / train_da command lines, and the DA / SDA
parameter validation (which runs before any device is touched)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import da_oracle as od
from conftest import ROOT

HYPER = dict(sparse_level=0.05, sparse_penalty=1.0, consecutive_penalty=0.2)


def setup(seed=0, batch=3, patches=4, k=7, n=5, level=0.3):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 1, size=(batch, patches, k))
    rows = batch * patches
    zeros = np.ones(rows * k)
    zeros[:int(rows * k * level)] = 0
    rng.shuffle(zeros)
    ones = ((1 - zeros).astype(int) & (rng.rand(rows * k) < 0.5).astype(int)).astype(float)
    w = rng.standard_normal((k, n)) * 0.5
    b0 = rng.standard_normal(n) * 0.1
    b1 = rng.standard_normal(k) * 0.1
    return x, zeros.reshape(rows, k), ones.reshape(rows, k), w, b0, b1


def torch_loss(x, zeros, ones, w, b0, b1, sparse_level, sparse_penalty, consecutive_penalty):
    """The reference's graph (DenoisingAutoencoderVariant.py:103-142) in torch: softmax cross entropy with the clean
    batch as labels and y as logits, cs over the 2-D h, cc over the frames."""
    batch, patches, k = x.shape
    x2 = x.reshape(batch * patches, k)
    xt = zeros * x2 + ones
    h = torch.sigmoid(xt @ w + b0)
    y = torch.sigmoid(h @ w.T + b1)
    cd = torch.mean(-(x2 * torch.log_softmax(y, dim=1)).sum(dim=1))
    cs = torch.mean(torch.abs(h - sparse_level).sum(dim=1))
    hb = h.reshape(batch, patches, -1)
    cc = torch.mean(torch.sqrt(((hb[:-1] - hb[1:]) ** 2).sum(dim=(1, 2))))
    return cd + sparse_penalty * cs + consecutive_penalty * cc, cd, cs, cc


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_matches_torch_autograd(seed):
    x, zeros, ones, w, b0, b1 = setup(seed)
    parts, grads = od.loss_and_grads(x, zeros, ones, w, b0, b1, **HYPER)
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=r) for a, r in
         ((x, False), (zeros, False), (ones, False), (w, True), (b0, True), (b1, True))]
    tparts = torch_loss(*t, **HYPER)
    tparts[0].backward()
    assert rel(parts, [p.item() for p in tparts]) <= 1e-12
    for g, tt in zip(grads, t[3:]):
        assert rel(g, tt.grad.numpy()) <= 1e-12


def test_oracle_matches_finite_differences():
    x, zeros, ones, w, b0, b1 = setup(2, batch=2, patches=3, k=5, n=4)
    _, grads = od.loss_and_grads(x, zeros, ones, w, b0, b1, **HYPER)
    eps = 1e-6
    for arr, g in zip((w, b0, b1), grads):
        num = np.zeros_like(arr)
        it = np.nditer(arr, flags=["multi_index"])
        for _ in it:
            i = it.multi_index
            old = arr[i]
            arr[i] = old + eps
            fp = od.loss_and_grads(x, zeros, ones, w, b0, b1, **HYPER)[0][0]
            arr[i] = old - eps
            fm = od.loss_and_grads(x, zeros, ones, w, b0, b1, **HYPER)[0][0]
            arr[i] = old
            num[i] = (fp - fm) / (2 * eps)
        assert np.abs(num - g).max() <= 1e-7 * max(1.0, np.abs(g).max())


def test_sparsity_term_divides_by_batch_times_patches():
    """cs = mean over the B*P rows of ||h - s||_1 (h is 2-D [B*P, N] in the DA), by hand: B = 2, P = 2, N = 3, so the
    B*N denominator of SDAV's layer 0 (6) would give another value than B*P (4)."""
    h = np.array([[0.25, 0.75, 0.05], [0.5, 0.0, 0.05], [1.0, 0.25, 0.05], [0.0, 0.5, 0.05]])
    x = np.full((4, 3), 1.0 / 3)
    y = np.full((4, 3), 0.5)
    _, _, cs, _ = od.loss_parts(x, h, y, 2, 0.05, 1.0, 0.2)
    l1 = (0.2 + 0.7) + (0.45 + 0.05) + (0.95 + 0.2) + (0.05 + 0.45)            # sum of |h - 0.05|: 3.05
    assert abs(cs - l1 / 4) < 1e-15
    assert abs(cs - l1 / 6) > 0.1


def test_salt_pepper_counts_truncate():
    assert od.salt_pepper_counts(10, 0.39)[0] == 3                # int(3.9): truncation, where SDAV's mask rounds
    assert od.salt_pepper_counts(750000, 0.3)[0] == 225000
    assert od.salt_pepper_counts(1, 0.3)[0] == 0


def run_cli(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", module] + list(args), cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=120)


@pytest.mark.parametrize("module", ["deeploopcloser_amd.train_sdav", "deeploopcloser_amd.train_da"])
def test_cli_help_and_required_flags(module):
    r = run_cli(module, "--help")
    assert r.returncode == 0 and "--dataset_dir" in r.stdout and "--key_points" in r.stdout
    r = run_cli(module, "train", "--dataset_ext", "ppm")
    assert r.returncode == 2 and "--dataset_dir" in r.stderr


def test_cli_empty_dataset_exits_nonzero(tmp_path):
    r = run_cli("deeploopcloser_amd.train_sdav", "train", "--dataset_dir", str(tmp_path), "--dataset_ext", "ppm")
    assert r.returncode != 0
    assert "Specified dataset is empty or could not find dataset" in r.stderr


def test_cli_defaults_are_the_references():
    """train-sdav.py:6-27 and DenoisingAutoencoderVariant.py:262-285, flag for flag."""
    from deeploopcloser_amd import train_da, train_sdav
    common = dict(input_shape=[30, 1681], batch_size=10, corruption_level=0.3, sparse_penalty=1.0, sparse_level=0.05,
                  consecutive_penalty=0.2, learning_rate=0.1, epochs=100, verbose=True)
    c = train_sdav.build_parser().parse_args(["train", "--dataset_dir", "d", "--dataset_ext", "ppm"])
    assert c.operation == "train" and c.dataset_dir == "d" and c.dataset_ext == "ppm"
    assert c.hidden_units == [2500, 2500, 2500, 2500, 2500]
    for k, v in common.items():
        assert getattr(c, k) == v, k
    assert (c.seed, c.key_points, c.save, c.load, c.out) == (0, "harris", None, None, None)
    c = train_da.build_parser().parse_args(["transform", "--dataset_dir", "d", "--dataset_ext", "ppm"])
    assert c.operation == "transform" and c.hidden_units == 2500
    for k, v in common.items():
        assert getattr(c, k) == v, k
    from deeploopcloser_amd._cli import dataset_pattern
    c = train_sdav.build_parser().parse_args(["train", "--dataset_dir", "a/b/", "--dataset_ext", ".ppm"])
    assert dataset_pattern(c) == "a/b/*.ppm"                     # train-sdav.py:42


def test_validation_runs_before_any_device():
    from deeploopcloser_amd import DA, SDA
    from deeploopcloser_amd.sda import validate_sda_params
    from deeploopcloser_amd.sdav import validate_da_params
    good = dict(sparse_level=0.05, sparse_penalty=1.0, consecutive_penalty=0.2, batch_size=10, learning_rate=0.1,
                epochs=100, corruption_level=0.3)
    # the reference's own defaults, which its v8n rules reject: layer_n = 0, an int sparse_penalty
    validate_da_params([30, 1681], 2500, layer_n=0, **good)
    validate_sda_params([30, 1681], [2500, 2500], **dict(good, sparse_penalty=1))
    bad = [dict(learning_rate=0), dict(learning_rate=-0.1), dict(sparse_level=0.0), dict(sparse_penalty=1.5),
           dict(consecutive_penalty=-0.1), dict(corruption_level=2), dict(batch_size=0), dict(epochs=0),
           dict(batch_size=2.5), dict(learning_rate="0.1"), dict(corruption_level=float("nan"))]
    for b in bad:
        with pytest.raises(ValueError):
            DA([30, 1681], 2500, **dict(good, **b))
        with pytest.raises(ValueError):
            SDA([30, 1681], [2500, 2500], **dict(good, **b))
    with pytest.raises(ValueError):
        DA([30, 1681], 2500, layer_n=-1)
    with pytest.raises(ValueError):
        DA([30, 1681], 0)
    with pytest.raises(ValueError):
        SDA([30, 1681], [2500])                                   # at least two layers (:57)
    with pytest.raises(ValueError):
        SDA([30, 1681], [2500, 0])
    with pytest.raises(ValueError):
        SDA([30], [2500, 2500])
