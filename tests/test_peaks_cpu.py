"""The NumPy restatement of dlc_peak_topk_rows (tests/peaks_oracle.py) pinned on its own, without a GPU: a hand-worked
row, the all-equal row, OpenSeqSLAM's two minima, and the edge rules of the definition in include/dlc.h."""
import numpy as np
import pytest

import peaks_oracle as po
import sequence_oracle as so


def picks(row, k, suppress, **kw):
    s, i = po.peak_topk_rows(np.asarray(row)[None, :], k, suppress, **kw)
    return s[0].tolist(), i[0].tolist()


def by_definition(row, k, suppress, lim=None, lower_is_better=False, absent=None):
    """The definition read literally, one pick at a time: the best offered cell that is more than `suppress` columns
    from every earlier pick (a scan of the whole row per pick, no sort)."""
    row = np.asarray(row)
    lim = row.size if lim is None else lim
    key = so.merit_keys(row[:lim], lower_is_better)
    taken = []
    for _ in range(k):
        best = None
        for j in range(lim):
            if (row.dtype != np.int64 and np.isnan(row[j])) or (absent is not None and row[j] == absent):
                continue
            if any(abs(j - p) <= suppress for p in taken):
                continue
            if best is None or key[j] > key[best]:                 # (a later equal key does not replace: ties -> lower j)
                best = j
        if best is None:
            break
        taken.append(best)
    return taken


def test_hand_worked_row():
    """Two places, columns 100 (10) and 300 (8), each with shoulders that fall by 1 per column down to 4 and 2 at
    distance 6; everything else is 0.5."""
    row = po.hand_worked_row()
    assert row[100] == 10.0 and row[94] == 4.0 and row[106] == 4.0 and row[300] == 8.0 and row[294] == 2.0 and row[93] == 0.5
    s, i = picks(row, 5, 0)                                        # the plain top-5: one place and its neighbours
    assert i == [100, 99, 101, 98, 102] and s == [10.0, 9.0, 9.0, 8.0, 8.0]
    s, i = picks(row, 4, 5)                                        # both places, then the first cells outside the window
    assert i == [100, 300, 94, 106] and s == [10.0, 8.0, 4.0, 4.0]
    # suppress = 6 covers both places whole (their shoulders end at distance 6): the third pick is the first 0.5
    s, i = picks(row, 4, 6)
    assert i == [100, 300, 0, 7] and s == [10.0, 8.0, 0.5, 0.5]
    # with the weaker place's shoulders one column longer -- 293 and 307 hold 8 - 7 = 1 -- the third pick is 293 (1)
    s, i = picks(po.hand_worked_row(reach_b=7), 4, 6)
    assert i == [100, 300, 293, 307] and s == [10.0, 8.0, 1.0, 1.0]
    for w in (0, 5, 6, 150, 250):
        assert picks(row, 6, w)[1][:len(by_definition(row, 6, w))] == by_definition(row, 6, w)


@pytest.mark.parametrize("w", [0, 1, 5, 63])
def test_all_equal_row(w):
    """Ties go to the lower column, so the picks walk the row in steps of W + 1."""
    n, k = 300, 8
    for value, lower in ((3.0, False), (3.0, True), (-0.0, False)):
        s, i = picks(np.full(n, value), k, w, lower_is_better=lower)
        want = [t * (w + 1) for t in range(k) if t * (w + 1) < n]
        assert i[:len(want)] == want and i[len(want):] == [-1] * (k - len(want))
        assert all(np.array_equal(np.float64(v).view(np.uint64), np.float64(value).view(np.uint64)) for v in s[:len(want)])
    s, i = picks(np.full(n, 7, np.int64), k, w, lower_is_better=True)
    assert i[:3] == [0, w + 1, 2 * (w + 1)] and s[:3] == [7, 7, 7]


def test_k2_is_openseqslam_min_value_and_min_value_2nd():
    """OpenSeqSLAM (doFindMatches): [min_value, min_idx] = min(scores); window = max(1, min_idx - R/2) : min(n, min_idx +
    R/2); not_window = setxor(1 : n, window); min_value_2nd = min(scores(not_window))."""
    rng = np.random.RandomState(4)
    for n, r_window in ((50, 10), (200, 10), (30, 20), (12, 10), (9, 20)):
        for _ in range(20):
            scores = rng.randint(1, 40, size=n).astype(np.float64) + rng.rand(n).round(1)
            min_idx = int(np.argmin(scores))
            window = np.arange(max(0, min_idx - r_window // 2), min(n, min_idx + r_window // 2 + 1))
            not_window = np.setxor1d(np.arange(n), window)
            s, i = picks(scores, 2, r_window // 2, lower_is_better=True)
            assert s[0] == scores.min() and i[0] == min_idx
            if not_window.size:
                assert s[1] == scores[not_window].min() and i[1] == not_window[np.argmin(scores[not_window])]
            else:
                assert s[1] == np.inf and i[1] == -1


def test_nan_inf_and_signed_zero():
    nan, inf = np.nan, np.inf
    row = np.array([1.0, nan, inf, -inf, 0.0, -0.0, 5.0, nan, inf])
    s, i = picks(row, 9, 0)
    assert i == [2, 8, 6, 0, 4, 5, 3, -1, -1]                       # +inf twice (lower column first), +0.0 above -0.0, no NaN
    assert s[:7] == [inf, inf, 5.0, 1.0, 0.0, -0.0, -inf] and np.signbit(s[5]) and not np.signbit(s[4])
    assert s[7:] == [-inf, -inf]
    s, i = picks(row, 9, 0, lower_is_better=True)
    assert i == [3, 5, 4, 0, 6, 2, 8, -1, -1] and s[7:] == [inf, inf]
    # a NaN inside a window neither is picked nor shields its neighbours; a pick's window still counts from the pick
    assert picks(np.array([nan, 9.0, nan, 8.0, 7.0]), 3, 1)[1] == [1, 3, -1]
    assert picks(np.array([nan, nan]), 2, 0) == ([-inf, -inf], [-1, -1])
    # fp32 rows are converted exactly
    s32, i32 = picks(np.array([1.5, -0.0, 0.0, np.nan], np.float32), 3, 0)
    assert i32 == [0, 2, 1] and s32 == [1.5, 0.0, -0.0] and np.signbit(s32[2])


def test_absent_value_of_int64_rows():
    row = np.array([5, -1, 9, -1, 9, 3], np.int64)
    assert picks(row, 6, 0) == ([9, 9, 5, 3, -1, -1], [2, 4, 0, 5, 1, 3])              # -1 is a value like any other
    assert picks(row, 6, 0, absent=-1) == ([9, 9, 5, 3, -1, -1], [2, 4, 0, 5, -1, -1])
    assert picks(row, 6, 0, absent=-1, lower_is_better=True) == ([3, 5, 9, 9, -1, -1], [5, 0, 2, 4, -1, -1])
    assert picks(row, 6, 0, lower_is_better=True)[1] == [1, 3, 5, 0, 2, 4]
    assert picks(row, 3, 1, absent=9) == ([5, 3, -1], [0, 5, 3])
    big = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0], np.int64)
    assert picks(big, 3, 0)[1] == [0, 2, 1] and picks(big, 3, 0, lower_is_better=True)[1] == [1, 2, 0]


def test_limits_clip_the_rows():
    m = np.arange(40, dtype=np.float64).reshape(4, 10)
    m[:, 7:] = 1000.0                                               # would win wherever a limit lets it in
    s, i = po.peak_topk_rows(m, 3, 1, limit0=-2, limit_step=4)      # lim = 0, 2, 6, 10
    assert i.tolist() == [[-1, -1, -1], [1, -1, -1], [5, 3, 1], [7, 9, 5]]
    assert s[0].tolist() == [-np.inf] * 3 and s[2].tolist() == [25.0, 23.0, 21.0] and s[3].tolist() == [1000.0, 1000.0, 35.0]
    s, i = po.peak_topk_rows(m, 2, 0, n=5, limit0=3, limit_step=1)  # n caps the limits: lim = 3, 4, 5, 5
    assert i.tolist() == [[2, 1], [3, 2], [4, 3], [4, 3]]
    s, i = po.peak_topk_rows(m.astype(np.int64), 2, 0, limit0=0, limit_step=0)
    assert (s == -1).all() and (i == -1).all() and s.dtype == np.int64


def test_suppress_zero_is_a_stable_argsort():
    rng = np.random.RandomState(9)
    for lower in (False, True):
        row = rng.randint(0, 8, size=500).astype(np.float64)        # mass ties
        s, i = picks(row, 128, 0, lower_is_better=lower)
        order = np.argsort(row if lower else -row, kind="stable")[:128]
        assert i == order.tolist() and s == row[order].tolist()


def test_windows_clipped_at_the_rows_ends():
    """A pick at column 0 and one at lim - 1: their windows end at the row's ends, and cells past lim are not there."""
    row = np.array([9.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 50.0, 60.0])
    assert picks(row, 4, 2, limit0=8) == ([9.0, 8.0, 4.0, -np.inf], [0, 7, 4, -1])
    assert picks(row, 3, 7, limit0=8) == ([9.0, -np.inf, -np.inf], [0, -1, -1])         # 7 is within 7 of 0
    assert picks(row, 3, 6, limit0=8) == ([9.0, 8.0, -np.inf], [0, 7, -1])
    for w in (8, 1 << 40, (1 << 63) - 1):
        assert picks(row, 3, w, limit0=8) == ([9.0, -np.inf, -np.inf], [0, -1, -1])
    rng = np.random.RandomState(11)
    for _ in range(30):
        row = rng.randint(0, 6, size=rng.randint(1, 60)).astype(np.float64)
        w, lim, lower = int(rng.randint(0, 12)), int(rng.randint(0, row.size + 1)), bool(rng.randint(2))
        want = by_definition(row, 7, w, lim, lower)
        got = picks(row, 7, w, limit0=lim, lower_is_better=lower)[1]
        assert got[:len(want)] == want and got[len(want):] == [-1] * (7 - len(want))


def test_two_place_scene_has_two_places():
    """The detectors' scene (test_gpu_peaks.py), checked here on the sequence sums (L = 4) of the cnn_vtl distance in
    NumPy: at every revisiting frame the three best key-frames are one place and its neighbours; of three picks more than
    5 apart the first two are the two places."""
    from oracle import distance as od
    from deeploopcloser_amd import slope_offsets
    x = po.two_place_scene(0, lambda rng, c: rng.randint(-128, 128, size=c).astype(np.int8), 64)
    seq, _ = so.sequence_scores(od.distance_matrix(x), 4, slope_offsets(4), limit0=-10, limit_step=1, lower_is_better=True)
    kw = dict(limit0=-10, limit_step=1, lower_is_better=True, absent=-1)
    plain, apart = po.peak_topk_rows(seq, 3, 0, **kw)[1], po.peak_topk_rows(seq, 3, 5, **kw)[1]
    for t in range(96, 120):
        a, b = 20 + t - 90, 55 + t - 90
        assert plain[t, 0] == a and all(abs(j - a) <= 2 for j in plain[t]) and b not in plain[t]
        assert apart[t, 0] == a and apart[t, 1] == b
