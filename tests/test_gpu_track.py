"""GPU place tracking (dlc_track_rows, dlc_track_backtrace, Engine.track_rows / track_backtrace, tracking.PlaceTracker,
track= on the detectors, the CLI) against the NumPy restatement of the recursion (tests/track_oracle.py).  Every comparison
is exact: places, columns and back-pointers by value, fp64 values by bit pattern, absent marks by position."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import sequence_oracle as so
import track_oracle as to

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
# eight numbers, sums of which are exact in fp64 in any order (tests/test_gpu_elastic.py): ties everywhere
EIGHT_F = np.array([-2.0, -0.5, -0.0, 0.0, 0.25, 1.0, 1.5, 3.0])
EIGHT_I = np.array([-3, -2, -1, 0, 1, 2, 3, 5], dtype=np.int64)
PLANS = ("resident", "rows")
NP_DTYPES = {"f64": np.float64, "f32": np.float32, "i64": np.int64}


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


def data(rng, dtype, kind, rows, n):
    if kind == "eight":
        m = (EIGHT_I if dtype == "i64" else EIGHT_F)[rng.randint(0, 8, size=(rows, n))]
    elif dtype == "i64":
        m = rng.randint(-10 ** 6, 10 ** 6, size=(rows, n))
    else:
        m = rng.standard_normal((rows, n))                            # unrounded: every sum rounds
        m[rng.rand(rows, n) < 0.02] = np.nan
    return m.astype(NP_DTYPES[dtype])


def winning(dtype, lower):
    if dtype == "i64":
        return -(1 << 40) if lower else (1 << 40)
    return -1e30 if lower else 1e30


def penalties(dtype, kind):
    """(jump, gate, null_score): exact beside the eight numbers (so that moves, jumps and the no-loop state tie)."""
    if dtype == "i64":
        return (1, 1, 2) if kind == "eight" else (300000, 200000, 150000)
    return (0.5, 0.25, 1.0) if kind == "eight" else (1.3, 0.7, 0.9)


class Raw:
    """One traversal through the C ABI itself: state and outputs in buffers wider than n, sentinel-filled, the score rows
    inside a buffer whose padding and whose cells past a row's limit hold values that would win."""

    def __init__(self, dlc, dtype, cap, pad=3):
        from deeploopcloser_amd import _lib
        self.e, self.lib, self.dtype, self.pad = dlc.default_engine(), _lib, dtype, pad
        self.is_int = dtype == "i64"
        self.code = {"f64": _lib.DLC_F64, "f32": _lib.DLC_F32, "i64": _lib.DLC_I64}[dtype]
        self.out_dt = torch.int64 if self.is_int else torch.float64
        dev = self.e.device
        self.V = torch.full((cap + pad,), SENTINEL, dtype=torch.int64, device=dev)
        self.V[:cap] = to.I64_MIN if self.is_int else torch.tensor(float("nan"), dtype=torch.float64).view(torch.int64)
        self.head = torch.zeros(4, dtype=torch.int64, device=dev)

    def call(self, m, steps, pen, n, limit0, step, lower, plan, expect=None):
        """m [rows, n] NumPy -> dict of NumPy outputs (the oracle's names); the words no cell owns are checked here."""
        e, lib, dev = self.e, self.lib, self.e.device
        rows, pad = m.shape[0], self.pad
        lim = so.limits(rows, n, n if limit0 is None else limit0, step)
        m = m.copy()
        m[np.arange(n)[None, :] >= lim[:, None]] = winning(self.dtype, lower)
        buf = torch.full((rows, n + pad), winning(self.dtype, lower), dtype=torch.from_numpy(m[:1, :1]).dtype, device=dev)
        buf[:, :n] = torch.from_numpy(m).to(dev)
        i64 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int64, device=dev)
        place, g, G, U, dense = i64(rows + 1), i64(rows + 1), i64(rows + 1), i64(rows + 1), i64(rows, n + pad)
        backU = torch.full((rows + 1,), 0x5A, dtype=torch.int8, device=dev)
        back = torch.full((rows, n + pad), 0x5A, dtype=torch.int8, device=dev)
        plan_code = {"resident": lib.DLC_TRACK_RESIDENT, "rows": lib.DLC_TRACK_ROWS, "auto": lib.DLC_TRACK_AUTO}[plan]
        need = e.lib.dlc_track_rows_workspace_bytes(rows, n, plan_code)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = e.lib.dlc_track_rows(e.ctx, self.code, p(buf), rows, n, n + pad, n if limit0 is None else limit0, step, steps[0],
                                  steps[1], int(lower), float(pen[0]), float(pen[1]), float(pen[2]), plan_code, p(self.V),
                                  p(self.head), p(place), p(g), p(G), p(U), p(backU), p(back), n + pad, p(dense), n + pad, p(ws),
                                  need, None)
        torch.cuda.synchronize()
        if expect is not None:
            assert rc == expect
            for t in (place, g, G, U, dense):
                assert bool((t == SENTINEL).all()), "an error wrote"
            assert bool((back == 0x5A).all()) and bool((backU == 0x5A).all())
            return None
        assert rc == lib.DLC_OK, e.lib.dlc_last_error(e.ctx)
        for t in (place, g, G, U):
            assert int(t[rows]) == SENTINEL
        assert int(backU[rows]) == 0x5A and bool((back[:, n:] == 0x5A).all()) and bool((dense[:, n:] == SENTINEL).all())
        assert bool((self.V[-pad:] == SENTINEL).all())
        typed = lambda t: t.cpu().numpy().view(np.int64 if self.is_int else np.float64)
        return dict(place=place[:rows].cpu().numpy(), g=g[:rows].cpu().numpy(), G=typed(G[:rows]), U=typed(U[:rows]),
                    backU=backU[:rows].cpu().numpy(), back=back[:, :n].cpu().numpy(), dense=typed(dense[:, :n].contiguous()))

    def state(self, n):
        v = self.V[:n].cpu().numpy()
        return (v if self.is_int else v.view(np.float64)), self.head.cpu().numpy()


def same(got, want, what=""):
    for name in want:
        assert so.same_bits(got[name], want[name]), (what, name)


def same_state(raw, state, n, what=""):
    v, head = raw.state(n)
    assert so.same_bits(v, state.V[:n]), (what, "V")
    assert int(head[0]) > 0 and int(head[0]) == state.seen and int(head[3]) == state.g, (what, "head")
    for word, value in ((1, state.U), (2, state.G)):                  # U and G as bits; any NaN is the absent mark
        assert so.same_bits(head[word:word + 1].view(state.dtype), value), (what, "head", word)


SWEEP_N = (1, 63, 64, 65, 200, 1030, 2049)
STEPS = ((0, 2), (1, 3), (0, 0), (0, 8), (2, 2), (1, 1), (3, 8))


@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32", "i64"])
@pytest.mark.parametrize("n", SWEEP_N)
def test_both_plans_against_the_oracle(dlc, n, dtype, lower):
    """All three dtypes in both senses at every n of the sweep; data: the eight exactly summable numbers and unrounded
    values; limits: fixed, and growing by one per row from a limit0 at or below zero; every call in both plans."""
    rows = 40 if n <= 200 else 24
    steps = STEPS[(SWEEP_N.index(n) + lower) % len(STEPS)]
    rng = np.random.RandomState(n * 7 + lower)
    for kind in ("eight", "noise"):
        m = data(rng, dtype, kind, rows, n)
        pen = penalties(dtype, kind)
        for limit0, step in ((None, 0), (-3 if n > 1 else 0, 1), (max(1, n - 5), 0)):
            state = to.State(n, dtype == "i64")
            want = to.track_rows(m, state, steps, *pen, n, limit0, step, lower)
            for plan in PLANS:
                raw = Raw(dlc, dtype, n)
                same(raw.call(m, steps, pen, n, limit0, step, lower, plan), want, (kind, limit0, plan))
                same_state(raw, state, n, (kind, limit0, plan))
    if n >= 63:
        assert (want["place"] >= 0).any()


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("dtype,lower,null_score", [("f64", False, 0.9), ("i64", True, None), ("f32", True, -0.4)])
def test_rows_split_over_calls_with_carried_state(dlc, dtype, lower, null_score, plan):
    """One call against the same rows 1, 3 and 7 at a time: the outputs, V and head are the oracle's either way."""
    rng = np.random.RandomState(3)
    rows, n, steps = 29, 333, (0, 2)
    m = data(rng, dtype, "noise", rows, n)
    pen = (1.3, 0.7) if dtype != "i64" else (300000, 200000)
    pen += (np.nan if null_score is None else null_score,)
    state = to.State(n, dtype == "i64")
    want = to.track_rows(m, state, steps, *pen, n, 300, 2, lower)
    for batch in (rows, 1, 3, 7):
        raw, parts = Raw(dlc, dtype, n), []
        for lo in range(0, rows, batch):
            parts.append(raw.call(m[lo:lo + batch], steps, pen, n, 300 + 2 * lo, 2, lower, plan))
        same({name: np.concatenate([p[name] for p in parts]) for name in want}, want, batch)
        same_state(raw, state, n, batch)
    if null_score is None:
        assert (want["backU"] == to.ABSENT).all() and (want["place"] == want["g"]).all()


@pytest.mark.parametrize("dtype", ["f64", "i64"])
def test_resident_equals_rows_at_the_largest_resident_n(dlc, dtype):
    from deeploopcloser_amd import _lib
    n, rows, steps = _lib.DLC_TRACK_RESIDENT_MAX, 3, (0, 8)
    rng = np.random.RandomState(9)
    m = data(rng, dtype, "eight", rows, n)
    pen = penalties(dtype, "eight")
    outs = []
    for plan in PLANS + ("auto",):
        raw = Raw(dlc, dtype, n)
        outs.append((raw.call(m, steps, pen, n, n - 2, 1, False, plan), raw.state(n)))
    for o, (v, head) in outs[1:]:
        same(o, outs[0][0])
        assert so.same_bits(v, outs[0][1][0]) and np.array_equal(head, outs[0][1][1])
    state = to.State(n, dtype == "i64")
    same(outs[0][0], to.track_rows(m, state, steps, *pen, n, n - 2, 1, False))
    assert so.same_bits(outs[0][1][0], state.V)


def test_resident_above_its_maximum_is_unsupported(dlc):
    from deeploopcloser_amd import _lib
    e = dlc.default_engine()
    n = _lib.DLC_TRACK_RESIDENT_MAX + 1
    assert e.lib.dlc_track_rows_workspace_bytes(3, n, _lib.DLC_TRACK_RESIDENT) == 0
    assert e.lib.dlc_track_rows_workspace_bytes(3, n, _lib.DLC_TRACK_AUTO) > 0
    m = np.zeros((2, n))
    raw = Raw(dlc, "f64", n)
    raw.call(m, (0, 2), (1.0, 1.0, 1.0), n, None, 0, False, "resident", expect=_lib.DLC_ERR_UNSUPPORTED)
    assert b"RESIDENT" in e.lib.dlc_last_error(e.ctx) and bool((raw.head == 0).all())
    want = to.track_rows(m, to.State(n, False), (0, 2), 1.0, 1.0, 1.0)
    same(raw.call(m, (0, 2), (1.0, 1.0, 1.0), n, None, 0, False, "auto"), want)          # AUTO takes the ROWS plan there
    with pytest.raises(ValueError):
        e.track_rows(torch.zeros((2, n), dtype=torch.float64, device=e.device), *e.track_state(n, torch.float64), plan="resident")


def test_bad_arguments_write_nothing(dlc):
    from deeploopcloser_amd import _lib
    m = np.zeros((4, 50))
    raw = Raw(dlc, "f64", 50)
    for steps, pen in (((3, 2), (1, 1, 1)), ((-1, 2), (1, 1, 1)), ((0, 9), (1, 1, 1)), ((0, 2), (-1, 1, 1)), ((0, 2), (1, np.inf, 1)),
                       ((0, 2), (np.nan, 1, 1)), ((0, 2), (1, -0.5, 1))):
        raw.call(m, steps, pen, 50, None, 0, False, "auto", expect=_lib.DLC_ERR_BAD_ARG)
    raw = Raw(dlc, "i64", 50)
    for pen in ((0.5, 1, 1), (1, 1, 1.5), (1, 2.0 ** 54, 1)):
        raw.call(m.astype(np.int64), (0, 2), pen, 50, None, 0, False, "auto", expect=_lib.DLC_ERR_BAD_ARG)
    e = dlc.default_engine()
    t = torch.zeros((4, 50), dtype=torch.float64, device=e.device)
    V, head = e.track_state(50, t.dtype)
    for kw in (dict(steps=(2, 1)), dict(plan="fast"), dict(n=51), dict(jump=-1.0)):
        with pytest.raises(ValueError):
            e.track_rows(t, V, head, **kw)
    with pytest.raises(ValueError):
        e.track_rows(t, V[:20], head)
    with pytest.raises(ValueError):
        e.track_rows(t.long(), V, head)
    assert bool((head == 0).all()) and bool(V.isnan().all())


@pytest.mark.parametrize("plan", PLANS)
def test_n_grows_between_calls(dlc, plan):
    rng = np.random.RandomState(12)
    widths, steps, pen = (50, 77, 77, 300), (0, 2), (0.5, 0.25, 1.0)
    raw, state = Raw(dlc, "f64", widths[-1]), to.State(widths[0], False)
    for i, n in enumerate(widths):
        m = data(rng, "f64", "eight", 5, n)
        want = to.track_rows(m, state, steps, *pen, n, n - 4, 1, False)
        same(raw.call(m, steps, pen, n, n - 4, 1, False, plan), want, n)
        same_state(raw, state, n, n)
    assert bool((raw.V[widths[-1]:] == SENTINEL).all())


def test_backtrace_from_every_kind_of_end(dlc):
    """150 rows (the wave takes 64 at a time): from every column, from nowhere, from the filtered place and from an
    absent cell, with and without a no-loop state."""
    e = dlc.default_engine()
    rng = np.random.RandomState(21)
    rows, n = 150, 23
    for null_score, lower in ((1.0, False), (np.nan, True)):
        m = data(rng, "f64", "eight", rows, n)
        m[:, -1] = np.nan                                              # an end that is absent
        if not np.isnan(null_score):
            m[70] = np.nan                                             # a row through which only nowhere leads
        o = to.track_rows(m, to.State(n, False), (0, 2), 0.5, 0.25, null_score, lower_is_better=lower)
        back, backU, g = (torch.from_numpy(o[name]).to(e.device) for name in ("back", "backU", "g"))
        wide = torch.full((rows, n + 5), to.ABSENT, dtype=torch.int8, device=e.device)
        wide[:, :n] = back
        last = torch.from_numpy(o["place"][-1:]).to(e.device)
        for end in list(range(n)) + [-1, to.END_FILTERED]:
            want = to.backtrace(o["back"], o["backU"], o["g"], end, o["place"][-1])
            for b in (back, wide[:, :n]):
                got = e.track_backtrace(b, backU, g, end, last)
                assert np.array_equal(got.cpu().numpy(), want), end
        assert (to.backtrace(o["back"], o["backU"], o["g"], n - 1) == to.NO_PATH).all()
        if np.isnan(null_score):
            assert (to.backtrace(o["back"], o["backU"], o["g"], 3) >= 0).all()
        else:
            assert to.backtrace(o["back"], o["backU"], o["g"], 3)[70] == -1
    for bad in (dict(end=n), dict(end=-3), dict(end=to.END_FILTERED, place_last=None)):
        with pytest.raises(ValueError):
            e.track_backtrace(back, backU, g, **bad)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_traversal(dlc, seed):
    """tests/test_track_cpu.py's traversal on the device: the oracle's labelling bit for bit, at most 2 frames from the truth."""
    m, truth = to.planted_traversal(seed)
    want = to.track_places(m, (0, 2), 4.0, 4.0, 2.0)
    got = dlc.track_places(m, (0, 2), 4.0, 4.0, 2.0)
    assert all(isinstance(a, np.ndarray) and so.same_bits(a, b) for a, b in zip(got, want))
    assert int((got[1] != truth).sum()) <= 2
    t = dlc.track_places(torch.from_numpy(m).to(dlc.default_engine().device), (0, 2), 4.0, 4.0, 2.0, plan="rows")
    assert all(isinstance(a, torch.Tensor) and so.same_bits(a.cpu().numpy(), b) for a, b in zip(t, want))


def test_place_tracker_and_a_detector_against_track_places(dlc):
    """PlaceTracker fed in uneven batches, with n growing, and CnnVtlLoopClosureDetector(track=) over its own distance
    rows: both are track_places on the full matrix."""
    rng = np.random.RandomState(31)
    x = rng.randint(-128, 128, size=(60, 64)).astype(np.int8)
    x[40:55] = x[5:20]                                                 # a revisit
    x[40:55, :6] += 1
    dist = dlc.DistanceCalculator.distance_matrix(x)                   # int64, lower is better
    quiet = int(np.median(dist))
    opts = dict(steps=(0, 2), jump=quiet // 2, gate=quiet // 2, null_score=quiet // 2)
    kw = dict(lower_is_better=True, limit0=-10, limit_step=1)
    place, path, G, U = to.track_places(dist, **opts, **kw)
    assert (path[42:55] == np.arange(7, 20)).all() and (path[:40] == -1).all()
    got = dlc.track_places(dist, **opts, **kw)
    assert all(so.same_bits(a, b) for a, b in zip(got, (place, path, G, U)))
    tracker, f, places = dlc.PlaceTracker(lower_is_better=True, **opts), 0, []
    for b in (1, 2, 9, 1, 40, 7):
        n = f + b                                                      # the columns the batch's last frame may see
        places.append(tracker.update(dist[f:f + b, :n], limit0=f - 10, limit_step=1)[0])
        f += b
    assert f == 60 and np.array_equal(np.concatenate(places), place) and np.array_equal(tracker.path(), path)
    assert np.array_equal(tracker.path(end=-1), to.backtrace(*full_history(dist, opts, kw), -1))
    tracker.reset()
    assert tracker.frames == 0 and len(tracker.path()) == 0
    for batch in (7, 32):
        det = dlc.CnnVtlLoopClosureDetector(64, k=3, exclusion=10, capacity=64, sequence=1, track=opts)
        plain = dlc.CnnVtlLoopClosureDetector(64, k=3, exclusion=10, capacity=64, sequence=1)
        for lo in range(0, 60, batch):
            a, b = det.query_and_insert(x[lo:lo + batch]), plain.query_and_insert(x[lo:lo + batch])
            assert len(a) == 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])      # the lists are unchanged
        assert det.tracker is not None and plain.tracker is None
        assert np.array_equal(det.tracker.path().cpu().numpy(), path), batch
    with pytest.raises(ValueError):
        dlc.CnnVtlLoopClosureDetector(64, track=opts)                  # needs sequence=L
    with pytest.raises(ValueError):
        dlc.CnnVtlLoopClosureDetector(64, sequence=1, track=dict(speed=3))


def full_history(dist, opts, kw):
    o = to.track_rows(dist, to.State(dist.shape[1], True), opts["steps"], opts["jump"], opts["gate"], opts["null_score"],
                      None, kw["limit0"], kw["limit_step"], kw["lower_is_better"])
    return o["back"], o["backU"], o["g"]


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cli_track(dlc):
    common = ("--network", "seqslam", "--metric", "sad", "--exclusion", "2", "--k", "2", "--batch", "4", "--sequence", "2")
    plain, res = run_cli(*common), run_cli(*common, "--track", "0:0:1000000", "--track-steps", "0:8")
    assert plain.returncode == 0 and res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    tracked = [l.split("\t") for l in lines if l.startswith("track\t")]
    assert [l for l in lines if not l.startswith("track\t")] == plain.stdout.splitlines()   # without the flag stdout is unchanged
    assert "track" not in plain.stdout
    # a no-loop score no difference reaches and free transitions: every frame with an older key-frame is placed
    assert [int(l[1]) for l in tracked] == list(range(3, 17)) and all(0 <= int(l[2]) < int(l[1]) - 2 for l in tracked)
