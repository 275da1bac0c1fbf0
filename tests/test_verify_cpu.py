"""CPU checks of the geometric verification: the oracle (tests/verify_oracle.py, the NumPy / Python-int restatement of
include/dlc.h's definition that the GPU and host-kernel tests compare against) checked against itself on scenes whose
answer is known, the int64 bound of the definition, the bindings, GeometricVerifier.apply on plain tensors and the CLI's
argument errors.  No GPU."""
import ctypes as C
import re
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import verify_oracle as vfo

RANDOM_SEED = 0                                            # of the five unrelated point sets below


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def test_dist_is_symmetric_bit_for_bit():
    rng = np.random.RandomState(1)
    q, d = rng.standard_normal((30, 100)), rng.standard_normal((30, 100))
    d[3] = q[7]
    q[5, 2], d[9, 0] = np.nan, np.inf
    a, b = vfo.dist_table(q, d), vfo.dist_table(d, q).T
    finite = ~np.isnan(a)
    assert np.array_equal(np.isnan(b), ~finite) and np.array_equal(bits(a)[finite], bits(b)[finite])
    assert a[7, 3] == 0.0 and np.isnan(a[5]).all() and np.isinf(a[:5, 9]).all()


def test_argmin_rules():
    nan = float("nan")
    assert vfo.argmin_low([3.0, 1.0, 1.0, 2.0]) == 1                         # ties go low
    assert vfo.argmin_low([nan, nan]) == -1
    assert vfo.argmin_low([nan, float("inf")]) == 1                          # +inf can win
    D = np.array([[1.0, 1.0, 5.0], [0.5, 2.0, 5.0], [nan, nan, nan]])
    pts = np.array([[1, 1], [2, 2], [3, 3]])
    # row 0 -> column 0 (tie, low), row 1 -> column 0; column 0 -> row 1: only patch 1 survives the cross-check
    assert vfo.matches(D, pts, pts, mutual=1).tolist() == [-1, 0, -1]
    assert vfo.matches(D, pts, pts, mutual=0).tolist() == [0, 0, -1]
    gone = pts.copy()
    gone[0] = (-1, -1)
    assert vfo.matches(D, pts, gone, mutual=0).tolist() == [-1, -1, -1]      # the candidate's point 0 is absent
    gone[0] = (8192, 5)
    assert vfo.matches(D, gone, pts, mutual=0).tolist() == [-1, 0, -1]       # the query's point 0 is absent


# multiplication by i, 2, 1 + i and 1; a translation hypothesis explains the pure shift only
@pytest.mark.parametrize("g,model", [((0, 1), vfo.SIMILARITY), ((2, 0), vfo.SIMILARITY), ((1, 1), vfo.SIMILARITY),
                                     ((1, 0), vfo.SIMILARITY), ((1, 0), vfo.TRANSLATION)])
def test_planted_scene_is_recovered_exactly(g, model):
    """30 points in 240 x 192 under an exact Gaussian-integer similarity, descriptors permuted copies, a third (10) of the
    matches sent to random points: with tol = 0 the count is the planted 20 and the mask the planted set."""
    q, q_pts, d, d_pts, planted = vfo.planted_scene(seed=5, g=g, outliers=10)
    got = vfo.verify_pair(q, q_pts, d, d_pts, model=model, tol=0, S=32, mutual=1)
    assert got["n_matches"] == 30 and got["inliers"] == 20 == len(planted)
    assert got["mask"] == sum(1 << p for p in planted)
    want = (planted[0], planted[1]) if model == vfo.SIMILARITY else (planted[0], -1)
    assert got["hyp"] == want                                               # the first hypothesis among equals
    if g == (2, 0) and model == vfo.SIMILARITY:                              # a scale of 2 is outside [1, 1]
        assert vfo.verify_pair(q, q_pts, d, d_pts, model=model, tol=0, S=16, mutual=1)["inliers"] <= 2


def test_unrelated_point_sets_stay_at_a_handful():
    """Five draws of 30 matched patches whose candidate points are unrelated to the query's: at most 4 of 30 agree with
    any similarity within 3 pixels (scale within [1/2, 2])."""
    worst = 0
    for draw in range(5):
        rng = np.random.RandomState(RANDOM_SEED + draw)
        q = rng.standard_normal((30, 8))
        q_pts, d_pts = vfo.distinct_points(rng, 30, 240, 192), vfo.distinct_points(rng, 30, 240, 192)
        got = vfo.verify_pair(q, q_pts, q.copy(), d_pts, model=vfo.SIMILARITY, tol=3, S=32, mutual=1)
        assert got["n_matches"] == 30
        worst = max(worst, got["inliers"])
    print("unrelated point sets: at most %d of 30 inliers" % worst)
    assert 2 <= worst <= 4


def test_int64_bound_at_the_corners():
    """Points at the corners of [0, 8191]^2 with tol = 255: every intermediate of the definition stays below 2^57 -- the
    oracle's Python ints record the peak -- so the int64 of the kernel cannot overflow."""
    corners = np.array([[0, 0], [8191, 0], [0, 8191], [8191, 8191]])
    idx = np.array([(i, j) for i in range(4) for j in range(4)])
    q_pts, d_pts = corners[idx[:, 0]], corners[idx[:, 1]]
    q = np.arange(16, dtype=np.float64)[:, None] * np.ones((1, 2))
    peak = vfo.Peak()
    for model in (vfo.SIMILARITY, vfo.TRANSLATION):
        for S in (0, 256):
            got = vfo.verify_pair(q, q_pts, q.copy(), d_pts, model=model, tol=255, S=S, mutual=1, peak=peak)
            assert got["n_matches"] == 16 and got["inliers"] >= 2 - model
    # reached here: 5 * 8191^4, 2^54.3; the bound of the definition: |re|, |im| <= 4 * 8191^2, so re^2 + im^2 < 2^57
    assert 1 << 54 < peak.value < 1 << 57 < 1 << 63


def test_bindings_exist_with_the_right_arity():
    from deeploopcloser_amd import _lib
    assert _lib.DLC_ABI_VERSION == 20
    ret, args = _lib.SIGNATURES["dlc_verify_pairs"]
    assert ret is C.c_int and len(args) == 27
    ret, args = _lib.SIGNATURES["dlc_verify_pairs_workspace_bytes"]
    assert ret is C.c_size_t and len(args) == 3
    header = open(os.path.join(ROOT, "include", "dlc.h")).read()
    proto = re.search(r"int dlc_verify_pairs\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert len(proto.split(",")) == 27
    assert "#define DLC_VERIFY_MAX_PATCHES %d\n" % _lib.DLC_VERIFY_MAX_PATCHES in header
    assert (_lib.DLC_VERIFY_SIMILARITY, _lib.DLC_VERIFY_TRANSLATION) == (vfo.SIMILARITY, vfo.TRANSLATION)
    lib = _lib.load()
    w = lib.dlc_verify_pairs_workspace_bytes(32, 5, 30)
    assert w >= 32 * 5 * 30 * 30 * 8 and w % 256 == 0
    for refused in ((0, 5, 30), (1, 0, 30), (1, _lib.DLC_MAX_K + 1, 30), (1, 5, 0), (1, 5, 65), (1 << 40, 5, 30)):
        assert lib.dlc_verify_pairs_workspace_bytes(*refused) == 0, refused


def test_apply_on_hand_made_tensors():
    import deeploopcloser_amd as dlc
    for name in ("GeometricVerifier", "verify_candidates"):
        assert name in dlc.__all__ and getattr(dlc.verification, name) is getattr(dlc, name)
    v = dlc.GeometricVerifier(patches=4, width=3, min_inliers=2)
    s = torch.tensor([[5.0, 4.0, 3.0, 2.0], [9.0, 8.0, float("-inf"), float("-inf")], [1.0, 0.5, 0.25, 0.125]], dtype=torch.float64)
    i = torch.tensor([[7, 8, 6, 9], [3, 1, -1, -1], [2, 4, 0, 1]])
    a = torch.tensor([[False, True, False, True], [True, True, True, True], [False, False, False, False]])
    gs, gi = v.apply(s, i, fill=float("-inf"), accept=a)
    ninf = float("-inf")
    assert gs.tolist() == [[4.0, 2.0, ninf, ninf], [9.0, 8.0, ninf, ninf], [ninf] * 4] and gs.dtype == torch.float64
    assert gi.tolist() == [[8, 9, -1, -1], [3, 1, -1, -1], [-1] * 4]
    # a distance detector's lists: the fill is its own empty slot, and companions move with their slots
    d = torch.tensor([[10, 20, 30]])
    gd, gi, extra = dlc.verification.keep_accepted(torch.tensor([[False, True, True]]), d, torch.tensor([[5, 6, 7]]), -1,
                                                   torch.tensor([[1, 12, 9]]))
    assert gd.tolist() == [[20, 30, -1]] and gi.tolist() == [[6, 7, -1]] and extra.tolist() == [[12, 9, 1]]
    with pytest.raises(ValueError):
        v.apply(s, i)
    for bad in (dict(patches=0), dict(patches=65), dict(width=0), dict(capacity=0), dict(min_inliers=-1), dict(model="affine"),
                dict(tol=256), dict(tol=-1), dict(tol=1.5), dict(max_scale=0.5), dict(max_scale=17)):
        with pytest.raises(ValueError):
            dlc.GeometricVerifier(**bad)


@pytest.mark.parametrize("argv", [
    ["--verify", "6"],                                                       # the default network is cnn_vtl
    ["--network", "cnn_vtl", "--verify", "6"],
    ["--network", "seqslam", "--metric", "sad", "--verify", "6"],
    ["--fuse", "sad,distance", "--verify", "6"],
    ["--network", "sdav", "--verify", "6", "--verify-tol", "256"],
    ["--network", "sdav", "--verify", "6", "--verify-tol", "-1"],
    ["--network", "sdav", "--verify", "-1"],
    ["--network", "sdav", "--verify", "6", "--verify-max-scale", "0.5"],
    ["--network", "sdav", "--verify", "6", "--verify-model", "affine"],
    ["--network", "sdav", "--verify-tol", "3"],                              # the options need --verify
    ["--network", "sdav", "--metric", "similarity", "--sequence", "3", "--chains", "--verify", "6"],
])
def test_cli_argument_errors(argv, capsys, tmp_path):
    from deeploopcloser_amd import loop_closure
    with pytest.raises(SystemExit) as err:
        loop_closure.main([str(tmp_path)] + argv)                            # (refused before the dataset is looked at)
    assert err.value.code == 2
    assert "verify" in capsys.readouterr().err
