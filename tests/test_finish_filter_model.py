"""The filtered selection of the cosine top-k finish (include/dlc.h, "the filtered selection"), as a NumPy model.

finish_topk_body (csrc/cosine_topk.hip) picks the kt half tiles with the largest maxima, and then the kg groups with the
largest maxima inside them, by FILTER, THEN RANK: a threshold T that at least kt keys reach is found cheaply, only the keys
>= T are ranked, and the best key below T joins the bound of what is left behind.  The model below restates the kernel's
data layout (8 waves, 64 lanes, lane l of wave w holds the half tiles lo_w + l + 64 j) and both of its paths on integer
keys, and holds them against a stable sort of all keys:

  * the selected half tiles, in order (key descending, index ascending);
  * the rest bound: the (kt+1)-th largest key, 0 when there is none.

No GPU is needed; tests/test_gpu_finish_select.py holds the kernels to the same statement (DLC_SELECT_SERIAL).
"""
import numpy as np
import pytest

WAVES, LANES, LV, GPH = 8, 64, 16, 16


def reference(keys, kt):
    """Stable sort: the kt best non-zero keys (larger key, then lower index) and the key of the next one (0: none)."""
    order = np.lexsort((np.arange(keys.size), -keys.astype(np.int64)))
    order = order[keys[order] != 0]
    rest = int(keys[order[kt]]) if order.size > kt else 0
    return order[:kt].tolist(), rest


def wave_kth_largest(v, kt):
    """wave_kth_largest_u32: the largest T with at least kt of the 64 values >= T, bit by bit from the top; 0 if none."""
    t = 0
    for b in range(31, -1, -1):
        c = t | (1 << b)
        if int((v >= c).sum()) >= kt:
            t = c
    return t


def layout(keys):
    """[wave, lane, j] -> half-tile index (or -1) as the kernel deals them."""
    nh = keys.size
    chunk = (nh + WAVES - 1) // WAVES
    assert chunk <= LANES * LV
    e = np.full((WAVES, LANES, LV), -1, dtype=np.int64)
    for w in range(WAVES):
        lo, hi = w * chunk, min(nh, (w + 1) * chunk)
        idx = lo + np.arange(LANES)[:, None] + LANES * np.arange(LV)[None, :]
        e[w] = np.where(idx < hi, idx, -1)
    return e


def rank(cands, keys, kt):
    """rank_select(..., plus_one): the candidates by (key descending, index ascending); the kt best and the next key."""
    cands = [c for c in cands if keys[c] != 0]
    cands.sort(key=lambda c: (-int(keys[c]), c))
    return cands[:kt], (int(keys[cands[kt]]) if len(cands) > kt else 0)


def serial_select(keys, kt):
    """The general path: every wave hands in the kt best of its slice one by one; the survivors are ranked."""
    e = layout(keys)
    handed, rest = [], 0
    for w in range(WAVES):
        mine = [int(i) for i in e[w].ravel() if i >= 0 and keys[i] != 0]
        mine.sort(key=lambda c: (-int(keys[c]), c))
        handed += mine[:kt]
        if len(mine) > kt:
            rest = max(rest, int(keys[mine[kt]]))
    sel, nxt = rank(handed, keys, kt)
    return sel, max(rest, nxt)


def filtered_select(keys, kt, cap):
    """The register path.  Returns (selected, rest bound, posted count, fell back)."""
    e = layout(keys)
    kv = np.where(e >= 0, keys[np.maximum(e, 0)], 0).astype(np.int64)           # [wave, lane, j]
    lane_max = kv.max(axis=2)
    t = max([wave_kth_largest(lane_max[w], kt) for w in range(WAVES)] + [1])
    posted = e[(kv >= t) & (e >= 0)].tolist()
    if len(posted) > cap:
        sel, rest = serial_select(keys, kt)
        return sel, rest, len(posted), True
    unposted = int(kv[kv < t].max()) if np.any(kv < t) else 0
    sel, nxt = rank(posted, keys, kt)
    return sel, max(unposted, nxt), len(posted), False


def check(keys, kg):
    keys = np.asarray(keys, dtype=np.int64)
    kt = min(kg, keys.size)
    want = reference(keys, kt)
    got = filtered_select(keys, kt, kg * GPH)
    assert (got[0], got[1]) == want
    assert serial_select(keys, kt) == want
    return got[2], got[3]


def gaussian_maxima(rng, nh):
    """Keys ordered like the maxima of 128 Gaussians (the benchmark's half tiles), unique with probability 1."""
    v = rng.standard_normal((nh, 128)).max(axis=1)
    return (v * 1e6).astype(np.int64) + 10_000_000


@pytest.mark.parametrize("nh", [1, 23, 24, 25, 129, 185, 547, 1000, 7813, 8192])
@pytest.mark.parametrize("kg", [5, 24, 64])
def test_random_keys(nh, kg):
    rng = np.random.RandomState(nh * 7 + kg)
    posted, fell_back = check(gaussian_maxima(rng, nh), kg)
    # (kt = 64 is every lane of a wave: the bound is the SMALLEST lane maximum, and with 16 values per lane more keys pass
    # it than there are slots -- the general path answers, as the model says it must)
    assert not fell_back or (kg == 64 and nh >= 7813)
    assert posted >= min(kg, nh)


def test_posted_count_at_the_benchmark_shape():
    """7813 half tiles, kt = 24: a wave's 24th largest lane maximum leaves a few hundred keys at most, well inside the
    kg * 16 = 384 slots."""
    rng = np.random.RandomState(1)
    counts = [check(gaussian_maxima(rng, 7813), 24)[0] for _ in range(20)]
    assert 24 <= min(counts) and max(counts) <= 384


@pytest.mark.parametrize("nh", [24, 400, 8192])
def test_all_equal_keys(nh):
    """Identical rows: every key passes the threshold; above the capacity the general path runs.  The lowest indices win."""
    keys = np.full(nh, 12345, dtype=np.int64)
    posted, fell_back = check(keys, 24)
    assert posted == nh and fell_back == (nh > 24 * GPH)


def test_kt_plus_one_equal_keys_at_the_boundary():
    """kt + 1 half tiles tie for the last places: the lower indices are selected and the rest bound IS the tied key."""
    rng = np.random.RandomState(3)
    kg = 24
    keys = rng.randint(1, 1000, size=3000).astype(np.int64)
    where = rng.choice(3000, kg + 1 + 10, replace=False)
    keys[where[:10]] = 5000 + np.arange(10)                  # ten clear winners
    keys[where[10:]] = 4000                                  # kg + 1 tied keys for the kg - 10 places that are left
    sel, rest, _, fell_back = filtered_select(keys, kg, kg * GPH)
    assert not fell_back and rest == 4000
    assert sel[10:] == sorted(where[10:].tolist())[:kg - 10]
    check(keys, kg)


@pytest.mark.parametrize("nonzero", [0, 1, 23])
def test_fewer_than_kt_keys(nonzero):
    """Key 0 is "no half tile" (a maximum of -inf): nothing is left behind and the list is short."""
    rng = np.random.RandomState(nonzero)
    keys = np.zeros(2000, dtype=np.int64)
    keys[rng.choice(2000, nonzero, replace=False)] = rng.randint(1, 1 << 31, size=nonzero)
    check(keys, 24)
    sel, rest, posted, _ = filtered_select(keys, 24, 24 * GPH)
    assert len(sel) == nonzero and rest == 0 and posted == nonzero


@pytest.mark.parametrize("where", ["one_wave", "one_lane", "first_eighth_of_a_wave"])
def test_the_top_sits_in_one_wave_or_one_lane(where):
    """The local bound counts LANES: when one lane (half tiles = l mod 64 of one slice) or one wave holds the whole top,
    the bound comes from another wave or falls low, more keys are posted, and the answer is the same."""
    rng = np.random.RandomState(11)
    nh, kg = 7813, 24
    keys = rng.randint(1, 100_000, size=nh).astype(np.int64)
    chunk = (nh + WAVES - 1) // WAVES
    if where == "one_wave":
        idx = 3 * chunk + rng.choice(chunk, 40, replace=False)
    elif where == "one_lane":
        idx = 2 * chunk + 5 + LANES * np.arange(LV)                              # lane 5 of wave 2: its 16 values
    else:
        idx = 6 * chunk + np.arange(40)
    keys[idx] = 1_000_000 + rng.permutation(idx.size)
    posted, fell_back = check(keys, kg)
    assert posted >= kg
    if where == "one_lane":
        assert not fell_back


def test_more_posted_keys_than_slots_falls_back():
    """A low threshold with many keys above it: one lane of every wave holds 16 large keys (no wave has kt lanes with a
    large maximum), everything else is equal -- every key is posted, the capacity overflows and the general path answers."""
    nh, kg = 7813, 24
    keys = np.full(nh, 777, dtype=np.int64)
    chunk = (nh + WAVES - 1) // WAVES
    for w in range(WAVES):
        keys[w * chunk + 9 + LANES * np.arange(LV)[: (3 if w else LV)]] = 900_000 + w
    posted, fell_back = check(keys, kg)
    assert fell_back and posted > kg * GPH


# ---- level 2: the kg2 best group keys among the 16 groups of each selected half tile
def pack(score_key, group):
    return (int(score_key) << 32) | (~int(group) & 0xffffffff)


@pytest.mark.parametrize("case", ["random", "equal", "few_half_tiles", "ragged_last", "one_rich_half_tile", "empty_half_tile"])
def test_level2_filter(case):
    rng = np.random.RandomState(len(case))
    kg = 24
    kt = 24
    if case == "few_half_tiles":
        kt = 1                                                   # 16 groups, kg2 = 16 > kt: no threshold
    g = np.zeros((kt, GPH), dtype=object)
    for t in range(kt):
        for j in range(GPH):
            sk = 4242 if case == "equal" else int(rng.randint(1, 1 << 31))
            if case == "one_rich_half_tile" and t == 7:
                sk = (1 << 31) + j                               # the whole top-16 in one half tile
            g[t, j] = pack(sk, (t * 37 % 500) * GPH + j)
    if case == "ragged_last":
        g[kt - 1, 3:] = 0                                        # groups past the last one of the shard
    if case == "empty_half_tile":
        g[5, :] = 0                                              # a selected slot without a half tile
    sel, rest, posted = level2_filtered(g, kg)                   # (python ints: 64-bit compares without overflow)
    want = level2_reference(g, kg)
    assert (sel, rest) == want
    if case == "random":
        assert posted < kt * GPH // 2                            # the filter does filter


def level2_filtered(gk, kg):
    """gk [kt, 16] packed 64-bit group keys (score key << 32 | ~group; 0 = no group) -> (slots in rank order, rest bound,
    keys ranked): T2 = the smallest row maximum of the score keys where kt >= kg2, 0 otherwise."""
    kt = gk.shape[0]
    m2 = kt * GPH
    kg2 = min(kg, m2)
    flat = [int(x) for x in gk.ravel()]
    hi = [x >> 32 for x in flat]
    row_max = [max(hi[t * GPH:(t + 1) * GPH]) for t in range(kt)]
    t2 = min(row_max) if kt >= kg2 else 0
    posted = [c for c in range(m2) if flat[c] != 0 and hi[c] >= t2]
    unposted = max([hi[c] for c in range(m2) if flat[c] == 0 or hi[c] < t2] + [0])
    posted.sort(key=lambda c: -flat[c])
    nxt = hi[posted[kg2]] if len(posted) > kg2 else 0
    return posted[:kg2], max(unposted, nxt), len(posted)


def level2_reference(gk, kg):
    flat = [int(x) for x in gk.ravel()]
    kg2 = min(kg, len(flat))
    order = sorted([c for c in range(len(flat)) if flat[c] != 0], key=lambda c: -flat[c])
    return order[:kg2], (flat[order[kg2]] >> 32 if len(order) > kg2 else 0)
