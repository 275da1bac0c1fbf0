"""The streaming detectors' refusals, pinned: one table of (detector, keyword arguments) -> the exact ValueError message.
Every case is refused before a store or an engine is created, so neither a GPU nor the built library is needed; the three
cases a detector ACCEPTS (suppress without sequence, where it is served) go on to the loader, and what they raise there,
if anything, is no ValueError."""
import pytest

NEEDS = {"contrast": "contrast needs sequence=L", "chains": "chains needs sequence=L", "slopes": "slopes needs sequence=L",
         "steps": "steps needs sequence=L", "track": "track needs sequence=L (L = 1 searches the frame scores themselves)",
         "suppress": "suppress needs sequence=L (L = 1 ranks by the frame scores themselves)"}
K_RANGE = "k=%d outside 1..128"
FUSED_MEMBERS = [("sad", 64), ("distance", 64)]

# detector -> (the arguments it cannot do without, its threshold keyword, has it track=, does it serve suppress alone)
DETECTORS = {
    "LoopClosureDetector": (dict(dim=64), "threshold", True, False),
    "SdavLoopClosureDetector": (dict(score_source=None), "threshold", True, False),
    "CnnVtlLoopClosureDetector": (dict(dim=64), "max_distance", True, False),
    "SeqSlamLoopClosureDetector": (dict(dim=64), "max_difference", True, True),
    "LdbLoopClosureDetector": (dict(dim=64), "max_distance", True, True),
    "FusedLoopClosureDetector": (dict(members=FUSED_MEMBERS), "threshold", False, True),
}


def _table():
    rows = []
    for name, (_, limit, track, suppress_alone) in DETECTORS.items():
        sdav = name == "SdavLoopClosureDetector"
        rows += [(name, dict(k=0), "k must be >= 1" if sdav else K_RANGE % 0),
                 (name, dict(k=129, sequence=4), K_RANGE % 129),
                 (name, dict(exclusion=-1), "exclusion must be >= 0"),
                 (name, dict(contrast=5), NEEDS["contrast"]),
                 (name, dict(chains=True), NEEDS["chains"]),
                 (name, dict(slopes=[[0]]), NEEDS["slopes"]),
                 (name, dict(steps=(0, 1)), NEEDS["steps"]),
                 (name, dict(sequence=0), "sequence=0 outside 1..64"),
                 (name, dict(sequence=65), "sequence=65 outside 1..64"),
                 (name, dict(sequence=4, steps=(3, 2)), "steps=(3, 2): need (d_min, d_max) with 0 <= d_min <= d_max <= 8"),
                 (name, dict(sequence=4, steps=(0, 1), slopes=[[0, 0, 0, 0]]), "steps and slopes exclude each other"),
                 (name, dict(sequence=4, contrast=33), "contrast=33 outside 1..32"),
                 (name, dict(sequence=4, suppress=-1), "suppress=-1 outside 0..2^63-1"),
                 (name, dict(sequence=4, slopes=[[0, 0, 0]]), "slopes must be an int32 table [1..16, 4]")]
        if not sdav:
            rows.append((name, dict(k=129), K_RANGE % 129))
        if track:
            rows += [(name, dict(track={}), NEEDS["track"]),
                     (name, dict(sequence=2, track={"x": 1}), "track must be a dict of steps, jump, gate, null_score, history")]
        if suppress_alone:
            rows.append((name, dict(suppress=-1), "suppress=-1 outside 0..2^63-1"))
        else:
            rows.append((name, dict(suppress=2), NEEDS["suppress"]))
        if limit != "threshold":
            rows += [(name, {limit: -1}, "%s must be >= 0 (or None)" % limit),
                     (name, dict(dim=0), "dim and capacity must be positive"),
                     (name, dict(capacity=0), "dim and capacity must be positive")]
    name = "SeqSlamLoopClosureDetector"
    rows += [(name, dict(shift=-1), "shift=-1 must be >= 0"),
             (name, dict(shift=2), "shift needs width, the thumbnail's columns"),
             (name, dict(shift=2, width=10), "dim=64 is not a multiple of width=10"),
             (name, dict(shift=2, width=0), "dim=64 is not a multiple of width=0"),
             (name, dict(shift=8, width=8), "shift=8 outside 0..min(8, width - 1 = 7)"),
             (name, dict(shift=9, width=16), "shift=9 outside 0..min(8, width - 1 = 15)")]
    name = "FusedLoopClosureDetector"
    kinds = "cosine, distance, sad"
    rows += [(name, dict(members=[]), "0 members outside 1..8"),
             (name, dict(members=[("sad", 64)] * 9), "9 members outside 1..8"),
             (name, dict(capacity=0), "capacity must be positive"),
             (name, dict(norm="l2"), "norm='l2' is none of zscore, minmax, none"),
             (name, dict(weights=[1.0]), "weights must be 2 finite numbers"),
             (name, dict(weights=[1.0, float("inf")]), "weights must be 2 finite numbers"),
             (name, dict(weights=[1.0, float("nan")]), "weights must be 2 finite numbers"),
             (name, dict(members=[("orb", 64), ("sad", 64)]), "a member is (kind, dim[, options]) with kind one of " + kinds),
             (name, dict(members=[("sad",)]), "a member is (kind, dim[, options]) with kind one of " + kinds),
             (name, dict(members=[("distance", 64, {"shift": 1})]), "member distance takes the options (none)"),
             (name, dict(members=[("cosine", 64, {"x": 1})]), "member cosine takes the options dtype, center"),
             (name, dict(members=[("sad", 64, {"dtype": "f16"})]), "member sad takes the options shift, width"),
             (name, dict(members=[("sad", 64, {"shift": 2})]),
              "sad: shift needs width, the thumbnail's columns, with dim a multiple of it"),
             (name, dict(members=[("sad", 64, {"shift": 2, "width": 10})]),
              "sad: shift needs width, the thumbnail's columns, with dim a multiple of it"),
             (name, dict(members=[("sad", 64, {"shift": 8, "width": 8})]), "sad: shift=8 outside 0..min(8, width - 1 = 7)")]
    return rows


TABLE = _table()


@pytest.mark.parametrize("name,kwargs,message", TABLE, ids=["%s-%d" % (r[0], n) for n, r in enumerate(TABLE)])
def test_refusal(name, kwargs, message):
    import deeploopcloser_amd as dlc
    args = dict(DETECTORS[name][0])
    args.update(kwargs)
    with pytest.raises(ValueError) as err:
        getattr(dlc, name)(**args)
    assert str(err.value) == message


def test_the_hashed_detector_wants_a_model():
    import deeploopcloser_amd as dlc
    with pytest.raises(ValueError) as err:
        dlc.HashedLoopClosureDetector(object())
    assert str(err.value) == "lsh must be an lsh.Lsh"


@pytest.mark.parametrize("name", [n for n, d in DETECTORS.items() if d[3]])
def test_suppress_alone_is_accepted_where_it_is_served(name):
    """SeqSlam, Ldb and Fused serve suppress=W without sequence=L: the constructor goes on to its store, and whatever
    that raises where there is no library or no GPU, it is no ValueError."""
    import deeploopcloser_amd as dlc
    try:
        det = getattr(dlc, name)(suppress=2, capacity=64, **DETECTORS[name][0])
    except ValueError as err:
        pytest.fail("%s(suppress=2) refused: %s" % (name, err))
    except Exception:
        return
    assert det.suppress == 2 and det.sequence is None
