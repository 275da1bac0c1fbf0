"""NumPy restatement of the VLAD / k-means definitions of include/dlc.h (dlc_vlad_assign, dlc_vlad_encode,
dlc_kmeans_step): a loop over h for DIST, a loop over the patches for the residuals, the block sums in row order and a
recursive TREE.  fp64, every operation rounded on its own (NumPy never contracts).  Test infrastructure only."""
import numpy as np

KMEANS_BLOCK = 1024
NORM_NONE, NORM_INTRA = 0, 1


def tree(v):
    """TREE over axis 0 of v: padded with -0.0 to a power of two, halves added recursively."""
    v = np.asarray(v, dtype=np.float64)
    c = v.shape[0]
    P = 1
    while P < c:
        P <<= 1
    if P > c:
        v = np.concatenate([v, np.full((P - c,) + v.shape[1:], -0.0)], axis=0)

    def T(u):
        if u.shape[0] == 1:
            return u[0]
        half = u.shape[0] // 2
        return T(u[:half]) + T(u[half:])
    with np.errstate(all="ignore"):
        return T(v)


def tree_pairwise(v):
    """The same TREE folded bottom-up, neighbour with neighbour (test_vlad_cpu.py shows the two equal): for long inputs."""
    v = np.asarray(v, dtype=np.float64)
    P = 1
    while P < v.shape[0]:
        P <<= 1
    v = np.concatenate([v, np.full((P - v.shape[0],) + v.shape[1:], -0.0)], axis=0)
    with np.errstate(all="ignore"):
        while v.shape[0] > 1:
            v = v[0::2] + v[1::2]
    return v[0]


def dist_matrix(x, c):
    """DIST of every (row, word): [rows, K].  One serial chain in h."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    d = np.zeros((x.shape[0], c.shape[0]))
    with np.errstate(all="ignore"):
        for h in range(x.shape[1]):
            t = x[:, h, None] - c[None, :, h]
            q = t * t
            d = d + q
    return d


def assign(x, c):
    """(a int32 [rows], dist [rows]): the lowest word whose distance is not NaN and <= every other non-NaN one; -1 and
    NaN for a row whose distances are all NaN."""
    d = dist_matrix(x, c)
    a = np.full(d.shape[0], -1, dtype=np.int32)
    best = np.full(d.shape[0], np.nan)
    with np.errstate(all="ignore"):
        for k in range(d.shape[1]):
            col = d[:, k]
            take = ~np.isnan(col) & ((a < 0) | (col < best))
            best = np.where(take, col, best)
            a = np.where(take, np.int32(k), a)
    return a, best


def vlad_encode(x, c, P, norm):
    """(out [frames, K * H], a [frames * P]) of rows x [frames * P, H]."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    K, H = c.shape
    frames = x.shape[0] // P
    a, _ = assign(x, c)
    out = np.zeros((frames, K, H))
    with np.errstate(all="ignore"):
        for f in range(frames):
            seen = [False] * K
            for p in range(P):
                n = f * P + p
                k = int(a[n])
                if k < 0:
                    continue
                r = x[n] - c[k]
                out[f, k] = out[f, k] + r if seen[k] else r
                seen[k] = True
        if norm == NORM_INTRA:
            for f in range(frames):
                nk = np.sqrt(tree((out[f] * out[f]).T))            # [K]
                for k in range(K):
                    out[f, k] = 0.0 if nk[k] == 0.0 else out[f, k] / nk[k]
    return out.reshape(frames, K * H), a


def kmeans_step(x, c_in, prev_assign=None):
    """(c_out, a, counts int64 [K], inertia, changed) of one Lloyd step."""
    x, c_in = np.asarray(x, dtype=np.float64), np.asarray(c_in, dtype=np.float64)
    rows, (K, H) = x.shape[0], c_in.shape
    a, d = assign(x, c_in)
    nb = (rows + KMEANS_BLOCK - 1) // KMEANS_BLOCK
    S = np.full((nb, K, H), -0.0)
    inert = np.zeros(nb)
    counts = np.zeros(K, dtype=np.int64)
    with np.errstate(all="ignore"):
        for n in range(rows):
            k = int(a[n])
            if k < 0:
                continue
            b = n // KMEANS_BLOCK
            S[b, k] = S[b, k] + x[n]                               # (-0.0 + x = x: starts from the first member's value)
            inert[b] = inert[b] + d[n]
            counts[k] += 1
        Sk = tree(S)
        c_out = c_in.copy()
        for k in range(K):
            if counts[k] > 0:
                c_out[k] = Sk[k] / float(counts[k])
        inertia = float(tree(inert))
    changed = rows if prev_assign is None else int((np.asarray(prev_assign) != a).sum())
    return c_out, a, counts, inertia, changed


def planted_scene(places=40, patches=30, types=12, dim=64, sigma=0.15, sigma_revisit=0.03, seed=0):
    """(db [places, patches, dim], queries [places, patches, dim]): every place holds `patches` noisy copies of landmark
    types; the revisit is the same patches + a little noise IN PERMUTED ORDER."""
    rng = np.random.RandomState(seed)
    landmarks = rng.standard_normal((types, dim))
    kinds = rng.randint(0, types, size=(places, patches))
    db = landmarks[kinds] + sigma * rng.standard_normal((places, patches, dim))
    q = np.empty_like(db)
    for i in range(places):
        q[i] = db[i][rng.permutation(patches)] + sigma_revisit * rng.standard_normal((patches, dim))
    return db, q


def lloyd(x, K, iters, seed):
    """Codebook of Vlad.fit's rule: the rows at sorted(RandomState(seed).choice(rows, K, replace=False)), then Lloyd steps
    until nothing changes or `iters` is reached."""
    x = np.asarray(x, dtype=np.float64)
    c = x[np.sort(np.random.RandomState(seed).choice(x.shape[0], K, replace=False))].copy()
    prev = None
    for _ in range(iters):
        c, prev, _, _, changed = kmeans_step(x, c, prev)
        if changed == 0:
            break
    return c


def cosine_hits(db_rows, q_rows):
    """How many queries have their own index as the cosine arg-max."""
    def unit(m):
        n = np.linalg.norm(m, axis=1, keepdims=True)
        return m / np.where(n == 0, 1.0, n)
    s = unit(q_rows) @ unit(db_rows).T
    return int((s.argmax(axis=1) == np.arange(q_rows.shape[0])).sum())
