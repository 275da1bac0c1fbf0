"""The rectangular cnn_vtl distance for the tests of dlc_cnnvtl_distance_rows: oracle.distance.bitwise_diff summed per
(query, db row) pair, and the row limits of include/dlc.h (lim(r) = clamp(limit0 + r * limit_step, 0, N))."""
import numpy as np


def distance_rows(q, db):
    """[Q, N] int64 distances through oracle.distance.bitwise_diff, a query at a time."""
    from oracle import distance as od
    q, db = np.asarray(q, np.int8), np.asarray(db, np.int8)
    out = np.empty((q.shape[0], db.shape[0]), dtype=np.int64)
    step = max(1, (1 << 24) // max(1, db.shape[1]))
    for r in range(q.shape[0]):
        for lo in range(0, db.shape[0], step):
            out[r, lo:lo + step] = od.bitwise_diff(q[r][None, :], db[lo:lo + step]).sum(axis=1)
    return out


def limits(rows, n, limit0, limit_step):
    return np.clip(limit0 + np.arange(rows, dtype=np.int64) * limit_step, 0, n)


def offered(rows, n, limit0, limit_step):
    """[rows, n] bool: the cells a call with these limits writes."""
    return np.arange(n)[None, :] < limits(rows, n, limit0, limit_step)[:, None]


def random_bytes(rng, shape):
    """int8 values over the whole range, with -128, -1, 0 and 127 planted."""
    x = rng.randint(-128, 128, size=shape).astype(np.int8)
    flat = x.reshape(-1)
    edge = np.array([-128, -1, 0, 127], dtype=np.int8)
    at = rng.permutation(flat.size)[:min(flat.size, 4 * max(1, flat.size // 16))]
    flat[at] = edge[np.arange(at.size) % 4]
    return x
