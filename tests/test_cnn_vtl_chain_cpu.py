"""The reference side of tests/test_gpu_cnn_vtl_f16x2_chain.py, held to what that file demands of the GPU -- without one.

  A0  every copy-network case the GPU file runs is EXACT in the CPU emulation of the f16x2 layer
      (conv_precision_bounds.emulate_conv_split): max |emulated - expected| = 0 at every layer, so that a failing == on
      the GPU is a finding about the chain, never about the premise;
  A3  the case list reaches every branch of the epilogue's min / max fold with a frame's unique minimum and with its
      unique maximum (one layer, and the last of three), keys accumulate over layers, the plants sit in frames' first,
      last and lonely rows and in partial column tiles, the expected bytes take all 256 values, and each of three modelled defects of the fold changes some
      case's expected bytes;
  the helpers themselves: expected_bytes is oracle.cnn_vtl.quantize_int8 where that is defined and 0 in its three
  written-out cases, fold_branch agrees with its vector form, the fold model without a defect is the plain min / max."""
import numpy as np
import pytest
import torch

import cnn_chain_oracle as O
import conv_precision_bounds as CB
from oracle import cnn_vtl as ocnn


def test_copy_networks_are_exact_in_the_emulation():
    names = []
    for name, x, layers in O.copy_cases():
        names.append(name)
        feats = O.expected_features(x, layers)
        h, w = x.shape[1:3]
        for l, (L, xin, g, wt) in enumerate(zip(layers, O.layer_inputs(x, layers, feats), O.layer_geometry(layers, h, w),
                                                  O.layer_weights(layers))):
            assert np.array_equal(xin, np.rint(xin)) and np.abs(xin).max() <= 255, (name, l)     # the premise
            assert np.array_equal(L.bias, np.rint(L.bias)), (name, l)
            geom = (g[0], g[1], g[4], g[5], g[6], g[7], g[8])
            got = CB.emulate_conv_split(torch.tensor(xin), torch.tensor(wt), torch.tensor(L.bias), geom, g[9])
            assert got.shape == feats[l].shape, (name, l)
            assert float((got - torch.tensor(feats[l])).abs().max()) == 0.0, (name, l)
            assert np.array_equal(feats[l], ocnn.conv2d_nhwc(xin, wt, L.bias, L.stride, "SAME", L.relu)), (name, l)
    assert len(names) == len(set(names)) == len(O.A1_CASES) + 45 + 2 + len(O.A3_NAMES) + 1 + len(O.A4_INDEPENDENCE)


def test_expected_bytes_is_the_oracle_formula_and_its_written_out_cases():
    x, layers, cols, feats = O.a3_case("three layers, 42 rows in the last")
    d = O.concat_features(feats)
    inside = (cols >= 0) & (cols < d.shape[1])
    got = O.expected_bytes(feats, cols)
    assert got.dtype == np.int8 and got.shape == (x.shape[0], cols.size)
    assert np.array_equal(got[:, inside], ocnn.quantize_int8(d)[:, cols[inside]])
    assert (~inside).sum() == 2 and not got[:, ~inside].any()
    assert sorted(cols[inside].tolist())[::1] != cols[inside].tolist() and len(set(cols.tolist())) < cols.size   # unsorted, repeats
    seg = np.array([[1.0, 2.0, 4.0], [3.0, 3.0, 3.0], [-1e-310, 0.0, 1e-310], [-1e300, 0.0, 1e300]])
    assert O.expected_bytes([seg], [0, 1, 2, 3, -1]).tolist() == [[0, 85, -1, 0, 0], [0] * 5, [0] * 5, [0, 127, -1, 0, 0]]


def test_fold_branch_forms_agree():
    for rpf, M in ((1, 600), (9, 630), (42, 546), (130, 650), (616, 1848), (130, 130), (5, 37)):
        br = O.fold_branches(rpf, M)
        assert [O.BRANCHES[b] for b in br] == [O.fold_branch(m, rpf, M) for m in range(M)]
    assert O.fold_branch(0, 130, 650) == "wave" and O.fold_branch(129, 130, 650) == "row" and O.fold_branch(150, 130, 650) == "block"
    assert O.fold_branch(629, 9, 630) == "block" and O.fold_branch(620, 9, 630) == "row"       # the clipped last block is one frame's
    assert O.fold_branch(645, 130, 650) == "wave"                                               # ... and the clipped last wave


def test_a3_cases_reach_every_branch_and_plant():
    O.assert_a3_coverage()
    for name in O.A3_NAMES:
        print(O.a3_summary(name))


def test_a3_expected_bytes_take_all_256_values():
    seen = set()
    for name in O.A3_NAMES:
        _, _, cols, feats = O.a3_case(name)
        seen |= set(np.unique(O.expected_bytes(feats, cols)).tolist())
    assert seen == set(range(-128, 128))


@pytest.mark.parametrize("defect", [{"drop": "row"}, {"drop": "block"}, {"drop": "wave"}, {"whole_column_groups_only": True}],
                         ids=["no row pass", "no block pass", "no wave pass", "whole 64-column groups only"])
def test_modelled_fold_defects_change_expected_bytes(defect):
    changed = []
    for name in O.A3_NAMES:
        _, _, cols, feats = O.a3_case(name)
        d = O.concat_features(feats)
        mn, mx = O.fold_model(feats)
        assert np.array_equal(mn, d.min(axis=1)) and np.array_equal(mx, d.max(axis=1)), name     # the model itself
        good = O.expected_bytes(feats, cols)
        assert np.array_equal(good, O.expected_bytes(feats, cols, (mn, mx)))
        bad = O.expected_bytes(feats, cols, O.fold_model(feats, **defect))
        if not np.array_equal(good, bad):
            changed.append((name, int((good != bad).sum())))
    print(defect, "changes", changed)
    assert changed
    # a defect in a frame-spanning branch must show in the LAST layer of a three-layer network too
    if defect.get("drop") in ("row", "block") or "whole_column_groups_only" in defect:
        assert any(n.startswith("three layers") for n, _ in changed)
    assert all(k >= 50 for _, k in changed), "losing a planted extremum must move many bytes"


def test_c_cases_have_their_rows():
    for case in O.C_CASES:
        segs, cols = O.c_case(*case)
        d = np.concatenate(segs, axis=1)
        assert len(segs) == case[0] and d.shape[0] == case[1]
        assert cols.min() == -1 and cols.max() == d.shape[1]
        exp = O.expected_bytes(segs, cols)
        mag = np.abs(d).max(axis=1)
        assert not exp[mag < 1e-300].any()
        if d.shape[1] > 1:
            r = np.nonzero((mag >= 1.0) & (d.max(axis=1) > d.min(axis=1)))[0]
            assert all({0, -1} <= set(exp[i].tolist()) for i in r), case
    assert {s.shape[1] for c in O.C_CASES for s in O.c_case(*c)[0]} == set(O.C_WIDTHS)
