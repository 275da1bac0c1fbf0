"""NumPy restatement of the sign-random-projection hash, written from the text of include/dlc.h (dlc_lsh_quantize_i8,
dlc_lsh_hash_i8) and of lsh.lsh_planes: the generator in Python integers, the quantisation in fp64, the hash as an
int64 product, a comparison and np.packbits.  test_lsh_cpu.py pins it against per-element loops; test_gpu_lsh.py
compares the library with it exactly."""
import numpy as np

M64 = (1 << 64) - 1
MAX_BITS, MAX_D, CHUNK, SPLIT_MAX_ROWS = 8192, 131071, 8192, 64
AUTO, ONE_PASS, SPLIT = 0, 1, 2


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def planes(n_bits, d, seed=0):
    """int8 [n_bits, d] of +-1: bit d % 64 of word(t, d // 64) = mix64(mix64(seed) + t * W + j), W = ceil(d / 64)."""
    w = (d + 63) // 64
    base = mix64(seed & M64)
    out = np.empty((n_bits, d), dtype=np.int8)
    for t in range(n_bits):
        for j in range(w):
            word = mix64((base + t * w + j) & M64)
            for c in range(64 * j, min(d, 64 * j + 64)):
                out[t, c] = 1 if (word >> (c % 64)) & 1 else -1
    return out


def row_bytes(bits):
    return 16 * ((bits + 127) // 128) if 1 <= bits <= MAX_BITS else 0


def quantize(x, mean=None):
    """x [rows, D] (any float type NumPy converts exactly to float64) -> int8 [rows, D]."""
    t = np.asarray(x, dtype=np.float64)
    if mean is not None:
        t = t - np.asarray(mean, dtype=np.float64)
    out = np.zeros(t.shape, dtype=np.int8)
    for r in range(t.shape[0]):
        m = np.abs(t[r]).max()
        if not np.isfinite(t[r]).all() or m == 0:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            s = np.float64(127.0) / m
            p = np.clip(np.rint(t[r] * s), -127.0, 127.0)        # np.rint: ties to even
        out[r] = np.where(t[r] == 0, 0.0, p).astype(np.int8)
    return out


def sums(q, pl):
    return np.asarray(q, dtype=np.int64) @ np.asarray(pl, dtype=np.int64).T


def hash_rows(q, pl):
    """q int8 [rows, D], pl int8 [bits, D] -> uint8 [rows, row_bytes(bits)]."""
    on = (sums(q, pl) > 0).astype(np.uint8)
    full = np.zeros((on.shape[0], 8 * row_bytes(pl.shape[0])), dtype=np.uint8)
    full[:, :on.shape[1]] = on
    return np.packbits(full, axis=1, bitorder="little")


def auto_plan(rows, d):
    """The AUTO rule stated in include/dlc.h."""
    return SPLIT if rows <= SPLIT_MAX_ROWS and d > CHUNK else ONE_PASS


def hamming(a, b):
    """int64 [len(a), len(b)] between packed rows."""
    x = a[:, None, :] ^ b[None, :, :]
    return np.unpackbits(x, axis=2).sum(axis=2).astype(np.int64)


def planted_stream(places=40, d=200, amplitude=0.25, seed=0):
    """(places [places, d], revisits [places, d]): uniform places in [0, 1), revisit i = place i + uniform noise in
    [-amplitude, amplitude)."""
    rng = np.random.RandomState(seed)
    base = rng.uniform(0.0, 1.0, size=(places, d))
    return base, base + rng.uniform(-amplitude, amplitude, size=(places, d))
