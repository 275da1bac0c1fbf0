"""The NumPy restatement of dlc_contrast_rows (tests/contrast_oracle.py) pinned on its own, without a GPU: worked values,
the edge rules of the definition in include/dlc.h, and the scene the normalisation exists for -- a planted revisit behind
a band of key-frames that resembles every revisiting frame."""
import math

import numpy as np
import pytest

import contrast_oracle as co
import sequence_oracle as so


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_hand_worked_row():
    """x = 1 2 4 8 16 at radius 1, every step written out in Python floats."""
    x = [1.0, 2.0, 4.0, 8.0, 16.0]
    want = []
    for j in range(5):
        w = x[max(0, j - 1):min(5, j + 2)]
        s = w[0]
        for v in w[1:]:
            s = s + v
        mean = s / float(len(w))
        q = (w[0] - mean) * (w[0] - mean)
        for v in w[1:]:
            q = q + (v - mean) * (v - mean)
        want.append((x[j] - mean) / math.sqrt(q / float(len(w) - 1)))
    got = co.contrast_rows(np.array([x]), 1)
    assert got.shape == (1, 5) and got.dtype == np.float64
    assert np.array_equal(bits(got[0]), bits(want))
    # the first cell by hand: window (1, 2), mean 1.5, q = 0.25 + 0.25, sd = sqrt(0.5 / 1)
    assert got[0, 0] == -0.5 / math.sqrt(0.5) and got[0, 4] == 4.0 / math.sqrt(32.0)
    # int64 and fp32 inputs are converted first
    assert np.array_equal(bits(co.contrast_rows(np.array([x], dtype=np.int64), 1)), bits(got))
    assert np.array_equal(bits(co.contrast_rows(np.array([x], dtype=np.float32), 1)), bits(got))


def test_constant_stretch_is_zero():
    x = np.array([[3.0, 1.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 2.0, 9.0]])
    got = co.contrast_rows(x, 2)
    assert np.array_equal(bits(got[0, 4:7]), bits([0.0, 0.0, 0.0]))        # windows 2..6, 3..7, 4..8: all 7
    assert got[0, 3] != 0.0 and got[0, 7] != 0.0


def test_fewer_than_two_cells_is_zero():
    assert np.array_equal(bits(co.contrast_rows(np.array([[5.0]]), 3)), bits([[0.0]]))
    # a row that offers one cell: its window is clipped at the limit, not at n
    got = co.contrast_rows(np.array([[5.0, 6.0, 7.0], [5.0, 6.0, 7.0]]), 1, limit0=1, limit_step=1)
    assert np.array_equal(bits(got[0, :1]), bits([0.0])) and np.isnan(got[0, 1:]).all()
    assert np.array_equal(bits(got[1, :2]), bits([-0.5 / math.sqrt(0.5), 0.5 / math.sqrt(0.5)])) and np.isnan(got[1, 2])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_poisons_exactly_its_windows(bad):
    rng = np.random.RandomState(1)
    x = rng.standard_normal((2, 40))
    x[0, 17] = bad
    x[1, 0] = bad
    got = co.contrast_rows(x, 3)
    nan = np.isnan(got)
    want = np.zeros((2, 40), bool)
    want[0, 14:21] = True                                                  # the cells within 3 of column 17
    want[1, 0:4] = True
    assert np.array_equal(nan, want)


def test_the_sum_starts_from_the_first_element():
    """A row of -0.0: every window's sum is -0.0 (begun at +0.0 it would be +0.0), and the row normalises to 0.0."""
    x = np.full((1, 6), -0.0)
    s, cnt = co.window_sums(x, [6], 2)
    assert np.array_equal(bits(s), bits(np.full((1, 6), -0.0))) and cnt.tolist() == [[3, 4, 5, 5, 4, 3]]
    assert np.array_equal(bits(co.contrast_rows(x, 2)), bits(np.zeros((1, 6))))
    s, cnt = co.window_sums(np.array([[-0.0, -0.0, 1.0]]), [2], 1)         # clipped at the limit: 1.0 is never added
    assert np.array_equal(bits(s[0, :2]), bits([-0.0, -0.0])) and cnt.tolist() == [[2, 2, 0]]


def test_limits_clip_the_windows():
    rng = np.random.RandomState(2)
    x = rng.randint(0, 4096, size=(9, 30)).astype(np.int64)
    got = co.contrast_rows(x, 5, limit0=20, limit_step=-2)
    lim = so.limits(9, 30, 20, -2)
    for r in range(9):
        alone = co.contrast_rows(x[r:r + 1, :lim[r]], 5) if lim[r] else np.zeros((1, 0))
        assert np.array_equal(bits(got[r, :lim[r]]), bits(alone[0])) and np.isnan(got[r, lim[r]:]).all()
    x[:, 7] = x[:, 7] + (1 << 60)                                          # rounds on conversion, the same way everywhere
    assert np.array_equal(bits(co.contrast_rows(x, 2)), bits(co.contrast_rows(x.astype(np.float64), 2)))


@pytest.mark.parametrize("seed", range(5))
def test_planted_revisit_behind_a_confuser_band(seed):
    """The scene of tests/test_gpu_contrast.py on the oracles alone: the plain sequence search puts every scored
    revisiting frame's best match inside the band; over the normalised rows it is the revisited frame, every time."""
    from deeploopcloser_amd.sequence import slope_offsets
    from oracle import distance as od
    x, true = co.confuser_band_scene(seed)
    d = od.distance_matrix(x)
    offs = slope_offsets(10)
    _, plain, _ = so.sequence_topk(d, 1, 10, offs, limit0=-30, limit_step=1, lower_is_better=True)
    assert all(70 <= plain[f, 0] <= 109 for f in range(159, 180))
    z = co.contrast_rows(d, 5, limit0=-30, limit_step=1)
    _, found, _ = so.sequence_topk(z, 1, 10, offs, limit0=-30, limit_step=1, lower_is_better=True)
    assert np.array_equal(found[159:180, 0], true[9:])
