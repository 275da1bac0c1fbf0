"""CPU checks of the sequence search: the NumPy oracle (tests/sequence_oracle.py) against a literal loop over the
definition in include/dlc.h, the slope table, and what the search is for -- a planted revisit that a single-frame nearest
neighbour gets wrong every time."""
import math
import struct

import numpy as np
import pytest

import sequence_oracle as so


def order_key(x):
    """Total order of the doubles as dlc_topk_rows_f64 ranks them: by the number, -0.0 below +0.0."""
    return (x, math.copysign(1.0, x))


def literal(m, L, offsets, n, limit0, limit_step, lower, row0, k):
    """dlc_sequence_topk cell by cell, slope by slope, element by element (Python floats / ints)."""
    rows = m.shape[0]
    is_int = m.dtype == np.int64
    lim = [min(max(limit0 + r * limit_step, 0), n) for r in range(rows)]
    empty_s = -1 if is_int else (math.inf if lower else -math.inf)
    S = [[None] * n for _ in range(rows)]
    V = [[-1] * n for _ in range(rows)]
    for r in range(rows):
        for j in range(n):
            for v, off in enumerate(offsets):
                total, ok = None, r - (L - 1) >= 0 and j < lim[r]
                for s in range(L):
                    if not ok:
                        break
                    c = j - int(off[s])
                    if not 0 <= c < lim[r - s]:
                        ok = False
                        break
                    e = int(m[r - s, c]) if is_int else float(m[r - s, c])
                    total = e if s == 0 else total + e
                if not ok or (not is_int and math.isnan(total)):
                    continue
                if is_int:
                    total = (total + 2 ** 63) % 2 ** 64 - 2 ** 63                     # int64 wraps
                merit = total if is_int else order_key(total)
                if S[r][j] is None:
                    better = True
                else:
                    cur = S[r][j] if is_int else order_key(S[r][j])
                    better = merit < cur if lower else merit > cur
                if better:
                    S[r][j], V[r][j] = total, v
    out_s = np.full((rows - row0, k), empty_s, np.int64 if is_int else np.float64)
    out_i = np.full((rows - row0, k), -1, np.int64)
    out_v = np.full((rows - row0, k), -1, np.int32)
    dense = np.full((rows - row0, n), -1 if is_int else np.nan, np.int64 if is_int else np.float64)
    for r in range(row0, rows):
        cells = [j for j in range(n) if S[r][j] is not None]
        for j in cells:
            dense[r - row0, j] = S[r][j]
        merit = (lambda j: S[r][j]) if is_int else (lambda j: order_key(S[r][j]))
        cells.sort(key=lambda j: (merit(j), j) if lower else (tuple(-c for c in merit(j)) if not is_int else -merit(j), j))
        for t, j in enumerate(cells[:k]):
            out_s[r - row0, t], out_i[r - row0, t], out_v[r - row0, t] = S[r][j], j, V[r][j]
    return out_s, out_i, out_v, dense


def random_table(rng, slopes, L, top):
    t = np.sort(rng.randint(0, top + 1, size=(slopes, L)), axis=1).astype(np.int32)
    t[:, 0] = 0
    return t


@pytest.mark.parametrize("seed", range(40))
def test_oracle_equals_the_literal_definition(seed):
    rng = np.random.RandomState(seed)
    rows, n = int(rng.randint(1, 9)), int(rng.randint(1, 12))
    L = int(rng.randint(1, 5))
    offsets = random_table(rng, int(rng.randint(1, 4)), L, int(rng.randint(0, 5)))
    kind = seed % 4
    if kind == 0:
        m = rng.randint(-3, 4, size=(rows, n)).astype(np.int64)                       # ties everywhere
        if seed % 8 == 0:
            m[rng.randint(0, rows), rng.randint(0, n)] = np.iinfo(np.int64).max        # a sum that wraps
    elif kind == 1:
        m = rng.randint(-2, 3, size=(rows, n)).astype(np.float64)                     # ties, and -0.0 among the zeros
        m[rng.rand(rows, n) < 0.2] = -0.0
    elif kind == 2:
        m = rng.standard_normal((rows, n))
        for val in (np.nan, np.inf, -np.inf):
            m[rng.rand(rows, n) < 0.12] = val
    else:
        m = rng.standard_normal((rows, n)).astype(np.float32)
    limit0, step = [(n, 0), (-2, 1), (1, 1), (n + 3, -1), (0, 0), (3, 2)][seed % 6]
    lower, row0, k = bool(seed % 2), int(rng.randint(0, rows)), int(rng.randint(1, 6))
    es, ei, ev, ed = literal(m, L, offsets, n, limit0, step, lower, row0, k)
    gs, gi, gv = so.sequence_topk(m, k, L, offsets, n, limit0, step, lower, row0)
    gd, gdv = so.sequence_scores(m, L, offsets, n, limit0, step, lower, row0)
    assert so.same_bits(gs, es) and np.array_equal(gi, ei) and np.array_equal(gv, ev)
    assert so.same_bits(gd, ed) and np.array_equal(gdv >= 0, ~np.isnan(ed) if ed.dtype == np.float64 else gdv >= 0)


def test_oracle_orders_signed_zeros_and_keeps_their_bits():
    m = np.array([[0.0, -0.0, 0.0, -0.0]])
    s, i, v = so.sequence_topk(m, 4, 1, [[0]])
    assert list(i[0]) == [0, 2, 1, 3]
    assert [struct.pack(">d", x)[0] for x in s[0]] == [0, 0, 0x80, 0x80]               # -0.0 + nothing is still -0.0
    s, i, v = so.sequence_topk(m, 4, 1, [[0]], lower_is_better=True)
    assert list(i[0]) == [1, 3, 0, 2]


def test_slope_offsets():
    from deeploopcloser_amd.sequence import slope_offsets
    t = slope_offsets(10)
    assert t.dtype == np.int32 and t.tolist() == [[0, 1, 2, 2, 3, 4, 5, 6, 6, 7], [0, 1, 2, 3, 4, 5, 5, 6, 7, 8],
                                                  [0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 1, 2, 3, 4, 6, 7, 8, 9, 10],
                                                  [0, 1, 2, 4, 5, 6, 7, 8, 10, 11]]
    assert slope_offsets(1).tolist() == [[0]]
    assert slope_offsets(2).tolist() == [[0, 1]]                                      # five velocities, one distinct row
    assert slope_offsets(4, 1.0, 1.0).tolist() == [[0, 1, 2, 3]]
    t = slope_offsets(64)
    assert t.shape == (5, 64) and (t[:, 0] == 0).all() and (np.diff(t, axis=1) >= 0).all() and t.max() == 76
    with pytest.raises(ValueError):
        slope_offsets(0)
    with pytest.raises(ValueError):
        slope_offsets(5, v_step=0.0)


def test_planted_revisit_single_frame_fails_sequence_finds_it():
    """260 int8 frames (D = 64, seed 7): frames 200-259 revisit frames 50-109 with 24 bytes changed, and a 6-byte-changed
    alias of every revisiting frame sits at a scattered older index.  Under the reference's distance the single-frame
    arg-min is the alias every time; the sequence arg-min (L = 10, five slopes, exclusion 30) is the true place for every
    frame whose line lies inside the revisit (51 of them: the first 9 reach back before it)."""
    from deeploopcloser_amd.sequence import slope_offsets
    from oracle import distance as od
    x, true, alias = so.planted_revisit()
    dist = np.array([[od.calculate_distance(a, b) for b in x] for a in x], dtype=np.int64)
    L, exclusion = 10, 30
    d1, i1, _ = so.sequence_topk(dist, 1, 1, [[0]], limit0=-exclusion, limit_step=1, lower_is_better=True)
    single = i1[200:260, 0]
    assert int((single == true).sum()) == 0 and np.array_equal(single, alias)
    ds, is_, vs = so.sequence_topk(dist, 1, L, slope_offsets(L), limit0=-exclusion, limit_step=1, lower_is_better=True)
    seq = is_[200 + L - 1:260, 0]
    assert seq.size == 51 and int((seq == true[L - 1:]).sum()) == 51
    assert (vs[200 + L - 1:260, 0] == 2).all()                                        # the line of velocity 1.0
