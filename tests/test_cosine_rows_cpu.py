"""CPU checks that pin the tests' restatement of the cosine path's score (tests/cosine_rows_oracle.py: the chain of
rescore8_f64 and f64_key) -- against exact integer products, against oracle.cosine within the chain's own rounding bound,
against oracle.cosine.order_key -- and what the sequence search on the key rows is for: a planted revisit whose
single-frame best match is an alias every time.  Plus the parts of the feature that need no GPU: the C entry's refusal of
a null context and the argument checks of LoopClosureDetector(sequence=L)."""
import numpy as np
import pytest
import torch

from oracle import cosine as ocos
import cosine_rows_oracle as cro
import sequence_oracle as so

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("d", [8, 64, 520, 1032, 4096])
def test_chain_is_exact_on_small_integers(d):
    """Operands k * 2^-7, |k| <= 128: exact in bf16 and fp16, every partial sum an integer multiple of 2^-14 below 2^53 --
    nothing rounds in any order, so the chain must equal the int64 product."""
    rng = np.random.RandomState(d)
    qi, xi = rng.randint(-128, 129, size=(5, d)), rng.randint(-128, 129, size=(9, d))
    qi[0, 0], xi[0, 0] = 128, -128
    q, x = qi * 2.0 ** -7, xi * 2.0 ** -7
    for dt in DTYPES:
        assert np.array_equal(cro.stored(q, dt), q) and np.array_equal(cro.stored(x, dt), x)
    got = cro.chain_scores(q, x)
    assert np.array_equal(got, (qi.astype(np.int64) @ xi.astype(np.int64).T) * 2.0 ** -14)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d", [8, 64, 520, 1032, 4096])
def test_chain_is_within_its_rounding_bound_of_the_oracle(d, dt):
    """Every product is exact; a score passes through at most d / 64 + 6 additions of the chain and the butterfly (the
    oracle's matmul through at most d), each off by at most 2^-53 of a partial sum that is at most sum |q x|: the two
    together stay below d * 2^-53 * sum |q x| with room to spare."""
    rng = np.random.RandomState(d + 1)
    q = cro.stored(ocos.l2_normalize(rng.standard_normal((6, d))), dt)
    x = cro.stored(ocos.l2_normalize(rng.standard_normal((11, d))), dt)
    got, ref = cro.chain_scores(q, x), ocos.scores(q, x)
    bound = d * 2.0 ** -53 * (np.abs(q) @ np.abs(x).T)
    assert (np.abs(got - ref) <= bound).all()
    assert np.array_equal(cro.chain_scores(q[2:3], x[4:9]), got[2:3, 4:9])      # a pair's value is the pair's alone


def test_keys_are_the_oracles_order_key():
    rng = np.random.RandomState(3)
    s = np.concatenate([rng.uniform(-1.01, 1.01, 4000), [0.0, -0.0, 1.0, -1.0, 0.5 * 2.0 ** -40, 1.5 * 2.0 ** -40,
                                                          2.5 * 2.0 ** -40, -0.5 * 2.0 ** -40, 3e5, -3e5]])
    keys = cro.f64_key(s)
    assert keys.dtype == np.int64 and np.array_equal(keys, np.rint(ocos.order_key(s) * 2.0 ** 40).astype(np.int64))
    assert cro.f64_key(np.array([0.5, 1.5, 2.5, -0.5]) * 2.0 ** -40).tolist() == [0, 2, 2, 0]      # half to even
    odd = cro.f64_key(np.array([np.nan, -np.inf, -1e30, np.inf, 1e30, -3.9e18 * 2.0 ** -40]))
    assert odd.tolist() == [cro.INT64_MIN + 1] * 3 + [cro.INT64_MAX] * 2 + [int(-3.9e18)]


def test_oracle_limits():
    assert cro.limits(4, 10, -1, 1).tolist() == [0, 0, 1, 2]
    assert cro.limits(3, 10, 12, -3).tolist() == [10, 9, 6]
    assert cro.offered(3, 4, 1, 1).tolist() == [[True, False, False, False], [True, True, False, False],
                                                [True, True, True, False]]
    assert cro.rank_by_key(np.array([[3, 9, 9, -1]]), 3).tolist() == [[1, 2, 0]]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dim", [64, 72])
def test_planted_revisit_single_frame_fails_sequence_finds_it(dim, dt):
    """260 normal frames (seed 7): frames 200-259 revisit frames 50-109 (+ 0.6 N(0, 1)), and an alias of every revisiting
    frame (+ 0.25 N(0, 1)) sits at a scattered older index.  On the key rows of the stored descriptors the single-frame
    arg-max is the alias every time; the sequence arg-max (L = 10, five slopes, exclusion 30) is the true place for every
    frame whose line lies inside the revisit (51 of them)."""
    from deeploopcloser_amd.sequence import slope_offsets
    x, true, alias = cro.planted_revisit_float(dim=dim)
    rows = cro.stored(ocos.l2_normalize(x), dt)
    scores = cro.chain_scores(rows, rows)
    keys = cro.f64_key(scores)
    L, exclusion = 10, 30
    _, i1, _ = so.sequence_topk(keys, 1, 1, [[0]], limit0=-exclusion, limit_step=1)
    single = i1[200:260, 0]
    assert int((single == alias).sum()) == 60
    _, is_, _ = so.sequence_topk(keys, 1, L, slope_offsets(L), limit0=-exclusion, limit_step=1)
    seq = is_[200 + L - 1:260, 0]
    assert seq.size == 51 and int((seq == true[L - 1:]).sum()) == 51
    # no two distinct scores of a row share a key: ranking the keys is ranking the scores
    for r in range(scores.shape[0]):
        assert np.unique(scores[r]).size == np.unique(keys[r]).size, r


def test_score_rows_rejects_a_null_context_without_a_device():
    from deeploopcloser_amd import _lib
    lib = _lib.load()
    assert lib.dlc_cosine_score_rows(None, _lib.DLC_BF16, None, 1, 8, None, 1, 8, 8, 1, 0, None, None, 1, None) == \
        _lib.DLC_ERR_BAD_ARG


@pytest.mark.parametrize("kwargs", [dict(sequence=0), dict(sequence=65), dict(slopes=[[0]]),
                                    dict(sequence=4, slopes=[[0, 1, 2]]), dict(sequence=4, slopes=[[0, 1, 2, 3, 4]]),
                                    dict(sequence=2, slopes=[0, 1]), dict(sequence=2, slopes=np.zeros((17, 2), np.int32))])
def test_detector_sequence_argument_checks(monkeypatch, kwargs):
    from deeploopcloser_amd import engine, loop_closure, matching

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    for module in (engine, matching):
        monkeypatch.setattr(module, "default_engine", no_engine)
    with pytest.raises(ValueError):
        loop_closure.LoopClosureDetector(64, **kwargs)
