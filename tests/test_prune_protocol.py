"""The pruned score pass of dlc_cosine_topk (include/dlc.h, "the pruned score pass"), as a NumPy model on the CPU.

Per query the score pass keeps bkt[NB] (the largest half-tile key seen in class `half tile % NB`, 0 = none) and thr (the
kt-th largest of some snapshot of bkt, 0 while fewer than kt classes are filled).  A half tile's epilogue always stores
its maximum, raises its class with an atomic max when its key is above the threshold it saw, and stores its group maxima
and hint only when its key is AT OR ABOVE that threshold.  The selection afterwards reads group maxima and hints of the
kt half tiles with the largest keys (ties: the lower index) and nothing else.

The model drives random interleavings of epilogues and refreshes, lets every read be stale (a threshold read returns any
value thr has held so far, a refresh reads every class at its own random past time), drops class updates and threshold
publications at random, and asserts what the kernels rely on:

  * the written set contains the selection's kt half tiles;
  * every threshold ever published is <= the true kt-th largest key and <= thr_final (the kt-th largest of the final
    classes), and every half tile with key >= thr_final was written -- the exhaustive pass's rule;
  * kt > NB takes the off route: everything is written.
"""
import numpy as np
import pytest

NB = 64


def f32_key(x):
    """The library's monotone ordering key of an fp32 score (larger float -> larger key); -inf counts as none (0)."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isneginf(x), np.uint32(0), k).astype(np.uint32)


def kth_largest_bitwise(v, kt):
    """wave_kth_largest_u32: bit by bit from the top, the largest T with at least kt values >= T (0: fewer than kt non-zero)."""
    t = 0
    for b in range(31, -1, -1):
        c = t | (1 << b)
        if int((v.astype(np.uint64) >= c).sum()) >= kt:
            t = c
    return t


def selection(keys, kt):
    """The finish's level 1: the kt half tiles with the largest keys, ties to the lower index; key 0 is never taken."""
    order = np.lexsort((np.arange(len(keys)), -keys.astype(np.int64)))
    return [int(e) for e in order[:kt] if keys[e] != 0]


def run_protocol(keys, kg, rng, p_refresh=0.1, p_drop=0.2, p_stale=0.5, nb=NB):
    """One launch.  Returns (written half tiles, thresholds published, final classes, kt)."""
    nh = len(keys)
    kt = min(kg, nh)
    if kg > nb:                                               # the off route: the call does not prune
        return set(range(nh)), [], None, kt
    hist = [[0] for _ in range(nb)]                           # every value each class has held, in time order
    thr_hist = [0]
    written = set()
    for ht in rng.permutation(nh):
        seen = thr_hist[rng.randint(len(thr_hist))] if rng.rand() < p_stale else thr_hist[-1]
        k = int(keys[ht])
        if k > seen and rng.rand() >= p_drop:                 # the class's atomic max (or a lost update)
            b = ht % nb
            hist[b].append(max(hist[b][-1], k))
        if k >= seen:
            written.add(int(ht))
        if rng.rand() < p_refresh:
            snap = np.array([h[rng.randint(len(h))] if rng.rand() < p_stale else h[-1] for h in hist], dtype=np.uint32)
            t = kth_largest_bitwise(snap, kt)
            if t and rng.rand() >= p_drop:
                thr_hist.append(max(thr_hist[-1], t))         # published with an atomic max: thr only rises
    final = np.array([h[-1] for h in hist], dtype=np.uint32)
    return written, thr_hist, final, kt


def half_tile_maxima(kind, nh, rng):
    if kind == "random":
        return rng.standard_normal(nh).astype(np.float32) * 0.02
    if kind == "ties":                                        # few distinct values: the kt-th place sits inside a tie
        return rng.choice(np.float32([0.01, 0.02, 0.03, 0.04]), nh)
    if kind == "all_equal":
        return np.full(nh, 0.125, dtype=np.float32)
    if kind == "negative":
        return -np.abs(rng.standard_normal(nh)).astype(np.float32)
    if kind == "with_neg_inf":                                # half tiles without a score (key 0) among real ones
        v = rng.standard_normal(nh).astype(np.float32)
        v[rng.rand(nh) < 0.5] = -np.inf
        return v
    raise AssertionError(kind)


def test_key_is_monotone_and_kth_largest_is_exact():
    rng = np.random.RandomState(0)
    x = np.sort(np.concatenate([rng.standard_normal(200).astype(np.float32), np.float32([0.0, -0.0, np.inf, -1e-30, 1e-30])]))
    k = f32_key(x).astype(np.int64)
    assert np.all(np.diff(k)[np.diff(x) > 0] > 0) and np.all(np.diff(k) >= 0)
    assert f32_key(np.float32(-np.inf)) == 0
    for _ in range(50):
        v = rng.randint(0, 1 << 32, NB, dtype=np.uint64).astype(np.uint32)
        v[rng.rand(NB) < rng.rand()] = 0
        if rng.rand() < 0.3:
            v[:] = rng.choice(v, 3)[rng.randint(0, 3, NB)]    # heavy ties
        for kt in (1, 2, 5, 24, 63, 64):
            want = int(np.sort(v)[::-1][kt - 1])
            assert kth_largest_bitwise(v, kt) == want, (kt, want)


@pytest.mark.parametrize("kind", ["random", "ties", "all_equal", "negative", "with_neg_inf"])
@pytest.mark.parametrize("nh,kg", [(129, 24), (157, 5), (1000, 24), (30, 24), (20, 24), (133, 64)])
def test_written_set_holds_the_selection(kind, nh, kg):
    rng = np.random.RandomState(nh * 7 + kg)
    for trial in range(12):
        keys = f32_key(half_tile_maxima(kind, nh, rng))
        knobs = dict(p_refresh=rng.choice([0.02, 0.2, 1.0]), p_drop=rng.choice([0.0, 0.3, 0.9]), p_stale=rng.choice([0.0, 0.5, 1.0]))
        written, thr_hist, final, kt = run_protocol(keys, kg, rng, **knobs)
        sel = selection(keys, kt)
        assert set(sel) <= written, (kind, trial, knobs)
        nz = np.sort(keys[keys != 0])[::-1]
        true_t = int(nz[kt - 1]) if len(nz) >= kt else 0       # the true kt-th largest key (0: fewer than kt half tiles score)
        thr_final = kth_largest_bitwise(final, kt)
        assert max(thr_hist) <= thr_final <= true_t, (kind, trial, knobs)
        assert all(int(ht) in written for ht in np.nonzero(keys >= max(thr_final, 1))[0]), (kind, trial, knobs)
        if knobs["p_drop"] == 0.0 and knobs["p_stale"] == 0.0:
            # nothing lost, nothing stale: the classes end as the per-class maxima, whatever the order of the launch
            want = np.zeros(NB, dtype=np.uint32)
            np.maximum.at(want, np.arange(nh) % NB, keys)
            # (a key is only posted when above the threshold seen, so a class may stay below its maximum -- never above)
            assert np.all(final <= want)
            assert thr_final <= kth_largest_bitwise(want, kt)


def test_pruning_prunes_in_the_model():
    """Not a safety property, but the point: with fresh reads and a refresh per epilogue most half tiles are skipped."""
    rng = np.random.RandomState(3)
    keys = f32_key(half_tile_maxima("random", 4000, rng))
    written, _, _, kt = run_protocol(keys, 24, rng, p_refresh=1.0, p_drop=0.0, p_stale=0.0)
    assert set(selection(keys, kt)) <= written and len(written) < 1000


def test_more_groups_than_classes_takes_the_off_route():
    rng = np.random.RandomState(4)
    keys = f32_key(half_tile_maxima("random", 133, rng))
    written, thr_hist, final, kt = run_protocol(keys, 132, rng)
    assert written == set(range(133)) and thr_hist == [] and final is None and kt == 132


def _align(x):
    return (x + 255) // 256 * 256


def test_library_states_the_room_behind_the_workspace():
    """dlc_cosine_topk_prune_bytes: q * (64 classes + 1 threshold) uint32 behind dlc_cosine_topk_workspace_bytes (which does
    not change) on the plans that prune, 0 elsewhere: kg = k + 4 > 64, the <= 16384-row plan, split-K, the bandwidth
    kernel, the spread re-score, shards of more than 24576 half tiles."""
    from deeploopcloser_amd import _lib
    lib = _lib.load()
    for q, n, d, k in [(256, 1_000_000, 4096, 20), (5, 16385, 64, 20), (256, 16640, 128, 20), (37, 20001, 448, 1),
                       (64, 63744, 512, 60)]:
        assert lib.dlc_cosine_topk_prune_bytes(q, n, d, k) == _align(q * (NB + 1) * 4), (q, n, d, k)
    for q, n, d, k in [(300, 17000, 64, 128), (64, 63744, 512, 61), (256, 1000, 4096, 20), (8, 9000, 4096, 20),
                       (2, 100_000, 64, 20), (8, 20000, 75008, 20), (256, 24577 * 128, 64, 20), (256, 1000, 4096, 0)]:
        assert lib.dlc_cosine_topk_prune_bytes(q, n, d, k) == 0, (q, n, d, k)
    assert lib.dlc_cosine_topk_prune_bytes(256, 24576 * 128, 64, 20) > 0
