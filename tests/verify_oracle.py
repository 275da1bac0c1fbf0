"""NumPy / Python-int restatement of the geometric verification of include/dlc.h (dlc_verify_pairs): DIST is
vlad_oracle's loop over h, the arg-mins are loops in ascending index with strict <, and the geometry runs in Python
ints, which cannot overflow -- `peak` records the largest magnitude any intermediate reached, so that the int64 bound of
the definition can be checked.  Test infrastructure only."""
import numpy as np

import vlad_oracle as vo

SIMILARITY, TRANSLATION = 0, 1
MAX_COORD = 8191
MAX_PATCHES = 64


def dist_table(q, d):
    """D[p][j] = DIST(q_p, d_j), [P, P]: one serial chain in h per cell."""
    return vo.dist_matrix(q, d)


def argmin_low(v):
    """The lowest index whose value is not NaN and <= every other non-NaN one; -1 if all are NaN."""
    best, bd = -1, 0.0
    for o, x in enumerate(v):
        if x == x and (best < 0 or x < bd):
            best, bd = o, x
    return best


def present(pt):
    return 0 <= int(pt[0]) <= MAX_COORD and 0 <= int(pt[1]) <= MAX_COORD


def matches(D, q_pts, d_pts, mutual):
    """match [P]: m(p) for p in M, else -1."""
    P = D.shape[0]
    m = [argmin_low(D[p]) for p in range(P)]
    r = [argmin_low(D[:, j]) for j in range(P)]
    out = np.full(P, -1, dtype=np.int32)
    for p in range(P):
        if m[p] < 0 or (mutual and r[m[p]] != p):
            continue
        if present(q_pts[p]) and present(d_pts[m[p]]):
            out[p] = m[p]
    return out


class Peak:
    """The largest |intermediate| of the integer geometry."""
    def __init__(self):
        self.value = 0

    def __call__(self, *vs):
        for v in vs:
            self.value = max(self.value, abs(v))
        return vs[-1]


def geometry(a, b, model, tol, S, peak=None):
    """(inliers, (hs, ht), flags) over the compacted matches a[i] -> b[i] (lists of (x, y) Python ints); hs, ht index
    the compacted list (-1: none).  peak: a Peak that sees every intermediate (slower)."""
    see = peak if peak is not None else (lambda *vs: vs[-1])
    n = len(a)
    best, best_h, best_flags = 0, (-1, -1), [False] * n
    if model == SIMILARITY:
        hyps = [(s, t) for s in range(n) for t in range(s + 1, n)]
    else:
        hyps = [(s, -1) for s in range(n)]
    for s, t in hyps:
        (asx, asy), (bsx, bsy) = a[s], b[s]
        if model == SIMILARITY:
            ux, uy = a[t][0] - asx, a[t][1] - asy
            vx, vy = b[t][0] - bsx, b[t][1] - bsy
            uu, vv = see(ux * ux, uy * uy, ux * ux + uy * uy), see(vx * vx, vy * vy, vx * vx + vy * vy)
            if uu <= 0 or vv <= 0:
                continue
            if S > 0 and not (see(256 * vv) <= see(S * S * uu) and see(256 * uu) <= see(S * S * vv)):
                continue
            bound = see(tol * tol * uu)
            flags = []
            for (aix, aiy), (bix, biy) in zip(a, b):
                dax, day, dbx, dby = aix - asx, aiy - asy, bix - bsx, biy - bsy
                re = (dbx * ux - dby * uy) - (vx * dax - vy * day)
                im = (dbx * uy + dby * ux) - (vx * day + vy * dax)
                if peak is not None:
                    peak(dbx * ux, dby * uy, vx * dax, vy * day, dbx * ux - dby * uy, vx * dax - vy * day, re,
                         dbx * uy, dby * ux, vx * day, vy * dax, dbx * uy + dby * ux, vx * day + vy * dax, im,
                         re * re, im * im, re * re + im * im)
                flags.append(re * re + im * im <= bound)
        else:
            sx, sy = bsx - asx, bsy - asy
            flags = []
            for (aix, aiy), (bix, biy) in zip(a, b):
                ex, ey = (bix - aix) - sx, (biy - aiy) - sy
                flags.append(see(ex * ex, ey * ey, ex * ex + ey * ey) <= tol * tol)
        cnt = sum(flags)
        if cnt > best:
            best, best_h, best_flags = cnt, (s, t), flags
    return best, best_h, best_flags


def verify_pair(q, q_pts, d, d_pts, model=SIMILARITY, tol=3, S=32, mutual=1, peak=None, D=None):
    """One pair: q, d [P, H] fp64, q_pts, d_pts [P, 2] ints -> dict(inliers, n_matches, hyp (2 ints), mask (int),
    match int32 [P], dist [P, P])."""
    D = dist_table(q, d) if D is None else D
    match = matches(D, q_pts, d_pts, mutual)
    M = [p for p in range(len(match)) if match[p] >= 0]
    a = [(int(q_pts[p][0]), int(q_pts[p][1])) for p in M]
    b = [(int(d_pts[match[p]][0]), int(d_pts[match[p]][1])) for p in M]
    inliers, (hs, ht), flags = geometry(a, b, model, int(tol), int(S), peak)
    mask = 0
    for i, f in enumerate(flags):
        if f:
            mask |= 1 << M[i]
    return dict(inliers=inliers, n_matches=len(M), hyp=(M[hs] if hs >= 0 else -1, M[ht] if ht >= 0 else -1), mask=mask,
                match=match, dist=D)


def absent_pair(P):
    """What a pair whose candidate id is < 0 or >= N writes (its dist slot is left alone: None)."""
    return dict(inliers=0, n_matches=0, hyp=(-1, -1), mask=0, match=np.full(P, -1, dtype=np.int32), dist=None)


def verify_pairs(q_desc, q_pts, db_desc, db_pts, cand, **kw):
    """q_desc [Q, P, H], q_pts [Q, P, 2], db_desc [N, P, H], db_pts [N, P, 2], cand [Q, k] -> a [Q][k] list of dicts."""
    N, P = db_desc.shape[0], db_desc.shape[1]
    return [[verify_pair(q_desc[r], q_pts[r], db_desc[c], db_pts[c], **kw) if 0 <= c < N else absent_pair(P)
             for c in (int(v) for v in cand[r])] for r in range(cand.shape[0])]


# ---- planted scenes -------------------------------------------------------------------------------------------------------
def gaussian_similarity(pts, g, shift):
    """pts [P, 2] ints under z -> g * z + shift in Gaussian integers: g = (gr, gi), shift = (sx, sy)."""
    x, y = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
    return np.stack([g[0] * x - g[1] * y + shift[0], g[1] * x + g[0] * y + shift[1]], axis=1).astype(np.int32)


def distinct_points(rng, P, width, height):
    """P distinct integer points in [0, width) x [0, height)."""
    flat = rng.choice(width * height, P, replace=False)
    return np.stack([flat % width, flat // width], axis=1).astype(np.int32)


def planted_scene(seed, P=30, H=16, g=(0, 1), shift=(300, 20), outliers=10, width=240, height=192):
    """(q [P, H], q_pts, d [P, H], d_pts, planted set of query patches): the candidate's descriptors are a permuted copy of
    the query's, its points the query's under the exact integer similarity -- but for `outliers` matches, whose candidate
    point is a random one instead (none of them on its true image, so the planted set is exact)."""
    rng = np.random.RandomState(seed)
    q = rng.standard_normal((P, H))
    q_pts = distinct_points(rng, P, width, height)
    perm = rng.permutation(P)                                  # candidate patch perm[p] is the query's patch p
    d = np.empty_like(q)
    d[perm] = q
    true = gaussian_similarity(q_pts, g, shift)
    assert true.min() >= 0 and true.max() <= MAX_COORD
    d_pts = np.empty_like(true)
    d_pts[perm] = true
    bad = rng.choice(P, outliers, replace=False)
    for p in bad:
        while True:
            cand = np.array([rng.randint(0, MAX_COORD + 1), rng.randint(0, MAX_COORD + 1)], dtype=np.int32)
            if not (cand == true[p]).all():
                break
        d_pts[perm[p]] = cand
    return q, q_pts, d, d_pts, sorted(set(range(P)) - set(int(p) for p in bad))
