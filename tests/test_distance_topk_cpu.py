"""Host-side parts of the cnn_vtl k-nearest search (dlc_cnnvtl_distance_topk): the workspace arithmetic, the
detector's argument checks and the CLI's refusal of the distance metric outside cnn_vtl -- none of them needs a GPU."""
import pytest

from deeploopcloser_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_workspace_bytes(lib):
    ws = lib.dlc_cnnvtl_distance_topk_workspace_bytes
    for bad in [(1, 100, 16, 0), (1, 100, 16, _lib.DLC_MAX_K + 1), (1, 100, 16, -3), (0, 100, 16, 5), (1, 0, 16, 5),
                (1, 100, 0, 5), (-1, 100, 16, 5)]:
        assert ws(*bad) == 0, bad
    # [Q][slabs][k] 8-byte keys, 256-byte aligned; the slab count never exceeds the db's tiles nor the scan's target
    for q, n, d, k in [(1, 1, 1, 1), (1, 1_000_000, 2243, 20), (32, 1_000_000, 2243, 20), (256, 1_000_000, 2243, 128),
                       (300, 70001, 65, 128), (7, 19, 4, 20)]:
        w = ws(q, n, d, k)
        assert w > 0 and w % 256 == 0
        assert w >= q * k * 8                                        # at least one list per query
        assert w <= ((q * 1024 * k * 8 + 255) // 256) * 256          # at most 1024 slabs per query tile
        assert ws(q, n, d, k) == w                                   # pure arithmetic
    # one list per 256-row tile until the target is reached: a single-query search over 1 000 rows has 4 of them
    assert ws(1, 1000, 64, 1) == ((1 * 4 * 1 * 8 + 255) // 256) * 256
    assert ws(1, 1000, 64, 20) < ws(1, 1000, 64, 40)


def test_distance_topk_rejects_bad_arguments_without_a_device(lib):
    # a null context is refused before anything touches a device
    assert lib.dlc_cnnvtl_distance_topk(None, None, 1, 16, None, 1, 16, 16, 1, 0, 1, None, None, None, 0, None) \
        == _lib.DLC_ERR_BAD_ARG


@pytest.mark.parametrize("kwargs", [dict(k=0), dict(k=_lib.DLC_MAX_K + 1), dict(exclusion=-1), dict(max_distance=-1),
                                    dict(dim=0), dict(capacity=0)])
def test_detector_argument_checks(kwargs):
    from deeploopcloser_amd.loop_closure import CnnVtlLoopClosureDetector
    args = dict(dim=64)
    args.update(kwargs)
    with pytest.raises(ValueError):
        CnnVtlLoopClosureDetector(**args)


def test_cli_refuses_distance_metric_for_sdav(capsys, monkeypatch):
    from deeploopcloser_amd import engine, loop_closure

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(engine, "default_engine", no_engine)
    with pytest.raises(SystemExit) as e:
        loop_closure.main(["unused_dir", "--network", "sdav", "--metric", "distance"])
    assert e.value.code == 2
    assert "--metric distance needs --network cnn_vtl" in capsys.readouterr().err

