"""NumPy fp64 restatement of one DA training step and of the DA's salt-and-pepper corruption (test infrastructure; the
package never imports it).

Follows src/sdav/network/DenoisingAutoencoderVariant.py: corruption :182-202 (x~ = zeros * x + ones, masks over the
whole flat batch [batch_size*P, K], drawn once), forward :103-119 (h = sigmoid(x~ W + b0), y = sigmoid(h W^T + b1),
tied decoder), loss :121-142, plain SGD on W, b0, b1 :144-148.  The labels of the cross entropy are the CLEAN batch and
are data (no gradient flows into them); h is 2-D [B*P, N], so the sparsity term's mean runs over B*P rows.
"""
import numpy as np


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def salt_pepper_counts(n, level):
    """(zeros, expected salt count, its standard deviation) of the reference's masks over n elements: int(n * level)
    zeros (a truncation), each of them salt with probability 1/2."""
    nz = int(n * level)
    return nz, nz / 2.0, np.sqrt(nz) / 2.0


def corrupt(x2d, zeros, ones):
    return x2d * zeros + ones


def loss_parts(x, h, y, batch, sparse_level, sparse_penalty, consecutive_penalty):
    """(loss, cd, cs, cc) of :121-142.  x [R, K] the labels, h [R, N], y [R, K]."""
    ymax = y.max(axis=1, keepdims=True)
    logsm = y - ymax - np.log(np.exp(y - ymax).sum(axis=1, keepdims=True))
    cd = np.mean(-(x * logsm).sum(axis=1))
    cs = np.mean(np.abs(h - sparse_level).sum(axis=1))           # h 2-D: L1 over the units, mean over B*P rows
    hb = h.reshape(batch, -1)
    cc = np.mean(np.sqrt(((hb[:-1] - hb[1:]) ** 2).sum(axis=1)))
    return cd + sparse_penalty * cs + consecutive_penalty * cc, cd, cs, cc


def loss_and_grads(x, zeros, ones, w, b0, b1, sparse_level=0.05, sparse_penalty=1.0, consecutive_penalty=0.2):
    """x [B, P, K]; zeros / ones [B*P, K].  -> ((loss, cd, cs, cc), (gW, gb0, gb1))."""
    batch, patches, k = x.shape
    if batch < 2:
        raise ValueError("a training batch needs at least 2 frames (the consecutive-frame term)")
    rows = batch * patches
    x2 = x.reshape(rows, k)
    xt = corrupt(x2, zeros, ones)
    h = sigmoid(xt @ w + b0)
    y = sigmoid(h @ w.T + b1)
    parts = loss_parts(x2, h, y, batch, sparse_level, sparse_penalty, consecutive_penalty)

    ymax = y.max(axis=1, keepdims=True)
    sm = np.exp(y - ymax)
    sm /= sm.sum(axis=1, keepdims=True)
    d_y = (sm * x2.sum(axis=1, keepdims=True) - x2) / rows
    d_z2 = d_y * y * (1 - y)
    d_h = d_z2 @ w + sparse_penalty * np.sign(h - sparse_level) / rows
    hb = h.reshape(batch, patches, -1)
    diff = hb[:-1] - hb[1:]
    nrm = np.sqrt((diff ** 2).sum(axis=(1, 2)))
    gcc = diff / nrm[:, None, None] * (consecutive_penalty / (batch - 1))
    d_hb = np.zeros_like(hb)
    d_hb[:-1] += gcc
    d_hb[1:] -= gcc
    d_h += d_hb.reshape(rows, -1)
    d_z1 = d_h * h * (1 - h)
    g_w = d_z2.T @ h + xt.T @ d_z1
    return parts, (g_w, d_z1.sum(axis=0), d_z2.sum(axis=0))


def sgd_step(x, zeros, ones, w, b0, b1, lr=0.1, **hyper):
    """One step: ((loss, cd, cs, cc) before the update, (W, b0, b1) after it)."""
    parts, (gw, gb0, gb1) = loss_and_grads(x, zeros, ones, w, b0, b1, **hyper)
    return parts, (w - lr * gw, b0 - lr * gb0, b1 - lr * gb1)


def fit_batches(batches, zeros, ones, w, b0, b1, epochs, lr=0.1, **hyper):
    """DA.fit_dataset (:210-243) over [B, P, K] batches: `epochs` steps per full batch, a short batch ends the fit.
    -> (W, b0, b1, steps)."""
    steps = 0
    for b in batches:
        if b.shape[0] != zeros.shape[0] // b.shape[1]:
            break
        for _ in range(epochs):
            _, (w, b0, b1) = sgd_step(b, zeros, ones, w, b0, b1, lr=lr, **hyper)
            steps += 1
    return w, b0, b1, steps
