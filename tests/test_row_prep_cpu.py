"""tests/row_prep_oracle.py on the CPU: the interval argument (four fp64 emulations of the normalisation, each with its own
summation order, land inside the interval of every element), the conditions on ambiguous elements the GPU tests rely on, and
that each modelled defect of a kernel is seen.  The HIP kernels are held to the same oracle in tests/test_gpu_row_prep.py."""
import numpy as np
import pytest

import row_prep_oracle as rp

DIMS = (1, 2, 3, 63, 64, 65, 100, 511, 513, 1023, 1025, 4097, 5003, 8193, 16385, 20483, 75000)
ROWS = 5
CASES = {}                                          # d -> what case(d) met: each d is computed once per session


def data(d, src, kind):
    return rp.draw(np.random.RandomState(1000 * d + 10 * (src is np.float64) + (kind == "n100")), kind, ROWS, d, src)


def case(d):
    """fp32 and fp64 sources, N(0, 1) and N(100, 1) rows, centred and not, both stored types, 5 rows each, at this d: the
    first element of an emulated order outside its interval (None if none), the elements, the ambiguous ones, those in
    cases that are not centred, and the elements a single rounding fp64 -> 16 bit gets wrong."""
    if d in CASES:
        return CASES[d]
    met = {"outside": None, "elements": 0, "ambiguous": 0, "ambiguous_not_centred": 0, "single_rounding_seen": 0}
    for src in (np.float32, np.float64):
        for kind in ("n01", "n100"):
            x = data(d, src, kind)
            for center in (False, True):
                for st in rp.KINDS:
                    lo, hi = rp.interval(x, center, st)
                    for order in rp.ORDERS:
                        bits = rp.emulate(x, center, st, order)
                        outside, amb = rp.verdict(bits, lo, hi, st)
                        if outside.any() and met["outside"] is None:
                            met["outside"] = (src.__name__, kind, center, st, order, rp.first_outside(outside, lo, hi, bits, st))
                    met["elements"] += amb.size
                    met["ambiguous"] += int(amb.sum())
                    met["ambiguous_not_centred"] += 0 if center else int(amb.sum())
                    once = rp.emulate(x, center, st, "pairwise", "single_rounding")
                    met["single_rounding_seen"] += int(rp.verdict(once, lo, hi, st)[0].sum())
    CASES[d] = met
    return met


@pytest.mark.parametrize("d", DIMS)
def test_every_summation_order_lies_inside_the_interval(d):
    """Forward, reverse, pairwise and 256-lane fp64 evaluations are inside every element's interval; no element of a case
    that is not centred is ambiguous."""
    met = case(d)
    assert met["outside"] is None, met["outside"]
    assert met["ambiguous_not_centred"] == 0


def test_ambiguous_share_and_the_double_rounding_contract():
    """Over the committed seeds, every d (computed here where an earlier test has not): at most 1e-5 of the elements are
    ambiguous, none where the row is not centred -- and a kernel that rounded fp64 -> 16 bit ONCE is caught on at least one
    element of the same data (the double rounding is the kernel's contract)."""
    met = [case(d) for d in DIMS]
    total = {k: sum(m[k] for m in met) for k in ("elements", "ambiguous", "ambiguous_not_centred", "single_rounding_seen")}
    print(total)
    assert total["ambiguous_not_centred"] == 0
    assert total["ambiguous"] <= 1e-5 * total["elements"]
    assert total["single_rounding_seen"] >= 1


def test_single_rounding_differs_on_a_built_element():
    """One element built for it: just above a midpoint of two bf16 values by less than half an fp32 spacing.  fp32 takes
    it to the midpoint, the tie goes to the even neighbour BELOW; a single rounding goes up."""
    z = np.array([[1.0 + 2.0 ** -8 + 2.0 ** -30]])
    assert rp.decode(rp.round_twice(z, "bf16"), "bf16")[0, 0] == 1.0
    assert rp.decode(rp.round_once(z, "bf16"), "bf16")[0, 0] == 1.0 + 2.0 ** -7
    z = np.array([[1.0 + 2.0 ** -11 + 2.0 ** -30]])
    assert rp.decode(rp.round_twice(z, "f16"), "f16")[0, 0] == 1.0
    assert rp.decode(rp.round_once(z, "f16"), "f16")[0, 0] == 1.0 + 2.0 ** -10
    # and where nothing is near a tie the two agree, subnormal fp16 values included
    z = np.random.RandomState(0).standard_normal((4, 1000)) * np.array([[1.0], [1e-3], [3e-6], [1e-7]])
    for st in rp.KINDS:
        assert np.array_equal(rp.round_once(z, st), rp.round_twice(z, st))


def test_stored_format_helpers_agree_with_torch():
    import torch
    f = (np.random.RandomState(3).standard_normal(20000) * np.exp(np.random.RandomState(4).uniform(-20, 3, 20000))).astype(np.float32)
    f[:4] = (0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8)            # two ties: to even, down and up
    for st, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        want = torch.from_numpy(f).to(tdt)
        bits = rp.f32_to_bits(f, st)
        assert np.array_equal(bits, want.view(torch.int16).numpy().view(np.uint16))
        assert np.array_equal(rp.decode(bits, st), want.double().numpy())


@pytest.mark.parametrize("d", (3, 65, 513, 1025, 4097, 5003))
@pytest.mark.parametrize("defect", ("skip_last_square", "mean_over_ldd", "tail_prev_inv", "odd_last_zero"))
def test_modelled_defects_are_seen(d, defect):
    """Each defect on each source type and stored type (centred for the mean's divisor): at least one element outside its
    interval, and where the defect touches named elements only (the tail, the last one) it is seen THERE."""
    for src in (np.float32, np.float64):
        vw = 16 // np.dtype(src).itemsize
        if defect == "tail_prev_inv" and d % vw == 0:
            continue
        x = data(d, src, "n01")
        center = defect == "mean_over_ldd"
        for st in rp.KINDS:
            lo, hi = rp.interval(x, center, st)
            bits = rp.emulate(x, center, st, "lanes256", defect)
            outside, _ = rp.verdict(bits, lo, hi, st)
            assert outside.any(), (src, st)
            if defect == "odd_last_zero":
                assert outside[:, -1].all() and not outside[:, :-1].any()
            if defect == "tail_prev_inv":
                assert outside[:, d - d % vw:].any() and not outside[:, :d - d % vw].any()


def test_what_the_old_allowance_let_through():
    """The case of the issue: a tail element of size ~0.001 in a row whose largest element is ~0.06, off by 23 %.  One ulp of
    the row's largest element allows it; its interval does not."""
    x = data(1025, np.float32, "n01")
    lo, hi = rp.interval(x, False, "bf16")
    bits = rp.emulate(x, False, "bf16", "forward")
    ref = rp.decode(bits, "bf16")
    e = int(np.argmin(np.abs(np.abs(ref[0]) - 1e-3)))
    bad = bits.copy()
    bad[0, e] = rp.f32_to_bits(np.array([ref[0, e] * 1.23], dtype=np.float32), "bf16")[0]
    assert abs(rp.decode(bad, "bf16")[0, e] - ref[0, e]) <= 2.0 ** -8 * np.abs(ref[0]).max()
    outside, _ = rp.verdict(bad, lo, hi, "bf16")
    assert outside[0, e] and outside.sum() == 1


def test_zero_rows_and_the_equal_row_width():
    x = np.zeros((2, 70), dtype=np.float32)
    x[1] = 3.0
    lo, hi = rp.interval(x, False, "bf16")
    assert np.all(lo[0] == 0) and np.all(hi[0] == 0) and np.all(lo[1] == hi[1])
    one = np.array([[5.0], [-0.3]])
    lo, hi = rp.interval(one, True, "f16")                       # d = 1 centred: exactly zero
    assert np.all(lo == 0) and np.all(hi == 0)
    assert np.array_equal(rp.emulate(one, True, "f16", "forward"), np.zeros((2, 1), dtype=np.uint16))
    lo, hi = rp.interval(x, True, "bf16")                        # d > 1 centred, all equal: no statement
    assert np.all(lo[1] == -np.inf) and np.all(hi[1] == np.inf) and np.all(lo[0] == -np.inf)
    others = np.arange(1, 4097)
    vo = 1.0 / np.sqrt(others)
    for st, mant in (("bf16", 8), ("f16", 11)):
        closest, largest = rp.equal_row_widths(st)
        gains = rp.decode(rp.round_twice(vo, st), st) / vo - 1.0
        for d in (closest, largest):
            assert 0.3 * 2.0 ** -mant < gains[d - 1] <= 2.0 ** -mant      # rounds UP, by close to the most a rounding adds
            assert np.sqrt(d) * rp.decode(rp.round_twice(vo[d - 1:d], st), st)[0] <= 1.005   # dlc.h's precondition holds
        assert gains[largest - 1] == gains.max()
        print(st, "closest above a midpoint: d = %d (+%.3g), largest stored norm: d = %d (+%.3g)"
              % (closest, gains[closest - 1], largest, gains[largest - 1]))


def test_reduction_references():
    bits = rp.f32_to_bits(np.array([[3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32), "f16")
    assert rp.stored_norms(bits, "f16").tolist() == [5.0, 0.0]
    assert rp.tau_scale_reference([0.0, 1.0, 1.01, 2.02], 8.0).tolist() == [1.0, 8.0 / 1.01, 8.0, 16.0]
    assert rp.tau_scale_reference([1.0, 2.0], None).tolist() == [1.0, 2.0 * 1.005 / 1.01]
