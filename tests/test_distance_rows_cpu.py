"""Host-side parts of the rectangular cnn_vtl distance (dlc_cnnvtl_distance_rows): the tests' oracle against the
reference-made matrices, the C entry point's refusal of a null context, and the argument checks of
CnnVtlLoopClosureDetector(sequence=L) -- none of them needs a GPU."""
import itertools

import numpy as np
import pytest

from deeploopcloser_amd import _lib
import distance_rows_oracle as dro


@pytest.mark.parametrize("name", ["n7_d2243", "n9_d37", "n3_d1"])
def test_oracle_rows_equal_the_reference_matrix(golden, name):
    z = golden("distance.npz")
    desc, matrix = z[name + "/desc"], z[name + "/matrix"]          # matrix: computed by the reference module itself
    n = desc.shape[0]
    full = dro.distance_rows(desc, desc)
    assert full.dtype == np.int64 and np.array_equal(full, matrix)
    for size in range(1, n + 1):                                    # every subset of the rows as queries
        for rows in itertools.combinations(range(n), size):
            rows = list(rows)
            assert np.array_equal(dro.distance_rows(desc[rows], desc), matrix[rows]), (name, rows)


def test_oracle_limits():
    assert dro.limits(4, 10, -1, 1).tolist() == [0, 0, 1, 2]
    assert dro.limits(3, 10, 12, -3).tolist() == [10, 9, 6]
    assert dro.offered(3, 4, 1, 1).tolist() == [[True, False, False, False], [True, True, False, False],
                                                [True, True, True, False]]
    x = dro.random_bytes(np.random.RandomState(0), (5, 16))
    assert x.dtype == np.int8 and {-128, -1, 0, 127} <= set(x.reshape(-1).tolist())


def test_distance_rows_rejects_a_null_context_without_a_device():
    lib = _lib.load()
    assert lib.dlc_cnnvtl_distance_rows(None, None, 1, 16, None, 1, 16, 16, 1, 0, None, 1, None) == _lib.DLC_ERR_BAD_ARG


@pytest.mark.parametrize("kwargs", [dict(sequence=0), dict(sequence=65), dict(slopes=[[0]]),
                                    dict(sequence=4, slopes=[[0, 1, 2]]), dict(sequence=4, slopes=[[0, 1, 2, 3, 4]]),
                                    dict(sequence=2, slopes=[0, 1]), dict(sequence=2, slopes=np.zeros((17, 2), np.int32))])
def test_detector_sequence_argument_checks(monkeypatch, kwargs):
    from deeploopcloser_amd import distance, engine, loop_closure

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    for module in (engine, distance):
        monkeypatch.setattr(module, "default_engine", no_engine)
    with pytest.raises(ValueError):
        loop_closure.CnnVtlLoopClosureDetector(64, **kwargs)
