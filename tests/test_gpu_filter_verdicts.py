"""The int8 arg-min filter's verdicts on the GPU against the exact integer model (filter_oracle.py), with == on integers:

  * sim_rows_kernel + gram_i8_kernel + pair_score_amin_kernel through Engine.sdav_similarity_matrix: stats[0] (arg-mins
    evaluated directly) == the model's undecided cells, direct_pairs == the model's pair map over the whole [N, N] array;
    and on three-frame data sets (sentinel frame, i, j) for the frame pairs with a cell at the window's edge, where a flip
    cannot cancel in a total;
  * stream_argmin_kernel<1>, stream_argmin_kernel<2> and the strip form of gram_i8_kernel through the stream queries: stats[0]
    of every query / batch == the model's count for those frames.

The data (filter_oracle.sharp_data, the shapes and parameters of filter_oracle.SHAPES) put a fifth of the cells inside the
window and dozens of cells exactly at gap W and W + 1; test_filter_oracle_cpu.py shows on the CPU that a kernel which lost a
digit product or a k-step of one accumulator class, or rounded or truncated where it must floor, changes these counts.

Shapes (N, P, H): (16, 30, 1) a single column; (20, 16, 63), (16, 32, 64), (40, 7, 65) either side of one 64-byte k-step, P a
full group / 32 / odd; (60, 2, 255), (44, 30, 256), (24, 13, 257) Kp padding 256 / 256 / 512, a last k-step that is all data
and one with a single column, 1320 rows across the 128-row tiles and the 1024-column block; (24, 30, 2500) the workload's
width, 40 k-steps; (300, 1, 64) P == 1, never undecided.
"""
import numpy as np
import pytest
import torch

import filter_oracle as fo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()


_SCORE = {}


def device_data(eng, key):
    """(x on the device, its distinctive score and column range, the model's verdicts), once per shape."""
    if key not in _SCORE:
        x, m, r = fo.shape_model(key)
        ds = torch.tensor(x, dtype=torch.float64).to(eng.device)     # (a copy: the cached array is read-only)
        score, rng = eng.distinctive_score(ds, 0.5, 0.2, with_range=True)
        _SCORE[key] = (ds, score, rng, r)
    return _SCORE[key]


def same_matrix(a, b):
    """Bit-equal score matrices (+inf, the score of identical patches, compares equal to itself)."""
    return torch.equal(a.isinf(), b.isinf()) and torch.equal(torch.nan_to_num(a, posinf=1e300), torch.nan_to_num(b, posinf=1e300)) \
        and not bool(a.isnan().any())


def matrix_call(eng, ds, score, **kw):
    n = ds.shape[0]
    stats = torch.full((2,), -7, dtype=torch.int64, device=eng.device)
    pairs = torch.full((n, n), 9, dtype=torch.uint8, device=eng.device)
    out, out_i = eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, no_host_sync=True, stats=stats, direct_pairs=pairs, **kw)
    return out.clone(), out_i.clone(), stats.tolist(), pairs.cpu().numpy()


def check_matrix(eng, ds, score, rng, r, what):
    n, p, h = ds.shape
    f_ref, i_ref = (t.clone() for t in eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, force_f64=True))
    row_bytes = n * p * 8
    for kw in ({}, {"range": rng}, {"chunk_bytes": max(1 << 16, 3 * p * row_bytes)}):
        out, out_i, (direct, why), pairs = matrix_call(eng, ds, score, **kw)
        assert why == 0, (what, kw.keys(), why)
        assert direct == r.total, (what, list(kw), direct, r.total)
        assert np.array_equal(pairs, r.pair_map), (what, list(kw), np.argwhere(pairs != r.pair_map)[:8].tolist())
        assert not np.tril(pairs).any()
        assert same_matrix(out, f_ref) and torch.equal(out_i, i_ref), (what, list(kw))


@pytest.mark.parametrize("shape", tuple(fo.SHAPES), ids=str)
def test_matrix_call_verdicts(eng, shape):
    ds, score, rng, r = device_data(eng, shape)
    if shape[1] == 1:
        assert r.total == 0
    check_matrix(eng, ds, score, rng, r, "matrix")
    print(fo.summary_line(r, "matrix"))


@pytest.mark.parametrize("shape", fo.PAIR_SHAPES, ids=str)
def test_matrix_call_verdicts_per_frame_pair(eng, shape):
    """Every frame pair with a cell at gap W or W + 1 (at most 60 of them), alone with the sentinel frame."""
    ds, score, rng, r = device_data(eng, shape)
    pairs = fo.boundary_pairs(r)
    assert len(pairs) >= 10
    for i, j in pairs:
        frames = fo.subset_frames(i, j)
        sub = ds[frames].contiguous()
        _, _, (direct, why), pm = matrix_call(eng, sub, score)
        assert why == 0 and direct == fo.subset_count(r, frames), (shape, i, j, direct, fo.subset_count(r, frames))
        assert np.array_equal(pm, r.pair_map[np.ix_(frames, frames)]), (shape, i, j)
    print(fo.summary_line(r, "matrix, %d frame pairs in three-frame calls" % len(pairs)))


class Stream:
    """A stream over (0, 1) with every frame of ds resident, the sentinel frame first."""

    def __init__(self, eng, ds, score):
        self.eng, self.ds, self.score = eng, ds, score
        self.n, self.p, self.h = ds.shape
        self.state = eng.sdav_stream_state(self.n, self.p, self.h, lo=0.0, hi=1.0)
        eng.sdav_stream_append(self.state, ds, 0, self.n, score)
        self.stats = torch.full((2,), -7, dtype=torch.int64, device=eng.device)

    def _taken(self):
        direct, why = self.stats.tolist()
        self.stats.fill_(-7)
        assert why == 0
        return direct

    def query(self, f):
        row = self.eng.sdav_stream_query(self.state, self.ds, f, self.score, 10.0, -10.0, stats=self.stats)
        return row, self._taken()

    def batch(self, first, count):
        rows = self.eng.sdav_stream_query_batch(self.state, self.ds, first, count, self.score, 10.0, -10.0, stats=self.stats)
        return rows, self._taken()

    def staged(self, first, count):
        eng = self.eng
        need = eng.lib.dlc_sdav_stream_query_batch_workspace_bytes(self.n, self.p, count)
        ws = torch.empty(int(need), dtype=torch.uint8, device=eng.device)
        rows = torch.zeros((count, max(1, first + count - 1)), dtype=torch.float64, device=eng.device)
        eng.sdav_stream_query_batch_staged(self.state, self.ds, first, count, self.score, 1, rows, ws, 10.0, -10.0)
        eng.sdav_stream_query_batch_staged(self.state, self.ds, first, count, self.score, 2, rows, ws, 10.0, -10.0, stats=self.stats)
        return rows, self._taken()


def batches(n, sizes):
    """(first, count) covering the frames 1 .. n - 1 with the sizes in turn (the last one cut)."""
    out, f, k = [], 1, 0
    while f < n:
        c = min(sizes[k % len(sizes)], n - f)
        out.append((f, c))
        f += c
        k += 1
    return out


def check_stream(eng, ds, score, want_matrix, per_query, what):
    """per_query [n]: the model's count of every query frame; want_matrix: the matrix call's scores."""
    n = ds.shape[0]
    st = Stream(eng, ds, score)

    def rows_ok(rows, first, count):
        for q in range(count):
            f = first + q
            assert same_matrix(rows[q, :f], want_matrix[:f, f]), (what, first, count, q)

    for f in range(1, n):                                           # stream_argmin_kernel<1>
        row, direct = st.query(f)
        assert direct == per_query[f], (what, "query", f, direct, int(per_query[f]))
        rows_ok(row[None, :], f, 1)
    routes = [("pairs of frames", st.batch, batches(n, (2, 3, 7, 5, 4, 6)))]      # stream_argmin_kernel<2>, odd batches too
    if n - 1 >= 8:                                                  # the strip of gram_i8_kernel, in one call and in two stages
        routes.append(("strip", st.batch, batches(n, (8, 9, 13)) if n - 1 >= 16 else [(1, n - 1)]))
        routes.append(("strip, staged", st.staged, [(1, n - 1)] + ([(n - 9, 9), (3, 8)] if n >= 12 else [])))
    for name, call, plan in routes:
        for first, count in plan:
            if name.startswith("strip") and count < 8:              # (a cut last batch: below the strip's threshold)
                continue
            rows, direct = call(first, count)
            want = int(per_query[first:first + count].sum())
            assert direct == want, (what, name, first, count, direct, want)
            rows_ok(rows, first, count)


@pytest.mark.parametrize("shape", fo.STREAM_SHAPES, ids=str)
def test_stream_verdicts(eng, shape):
    ds, score, rng, r = device_data(eng, shape)
    want = eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, want_int64=False)[0].clone()
    check_stream(eng, ds, score, want, fo.stream_query_counts(r), "stream %s" % (shape,))
    print(fo.summary_line(r, "stream"))


def test_stream_verdicts_per_frame_pair(eng):
    """The three-frame data sets of the matrix's frame-pair check through the stream: one query, a batch of two."""
    shape = fo.PAIR_SHAPES[1]
    ds, score, rng, r = device_data(eng, shape)
    pairs = fo.boundary_pairs(r)
    for i, j in pairs:
        frames = fo.subset_frames(i, j)
        sub = ds[frames].contiguous()
        st = Stream(eng, sub, score)
        counts = [0] + [int(sum(r.pair_count[a, f] for a in frames[:k])) for k, f in enumerate(frames) if k > 0]
        for f in range(1, len(frames)):
            _, direct = st.query(f)
            assert direct == counts[f], (shape, i, j, f, direct, counts[f])
        if len(frames) == 3:
            _, direct = st.batch(1, 2)
            assert direct == counts[1] + counts[2], (shape, i, j, direct, counts)
    print(fo.summary_line(r, "stream, %d frame pairs in three-frame streams" % len(pairs)))


def test_copies_are_dropped_before_the_count(eng):
    """Twins inside every frame and a repeated frame: the counts are the model's WITH the copy rule (candidates inside the
    window first, later bit-identical copies of an earlier member dropped, undecided when two or more remain)."""
    key = ("copies",) + fo.PAIR_SHAPES[0]
    ds, score, rng, r = device_data(eng, key)
    x, m, _ = fo.shape_model(key)
    without = m.verdicts(copies=False)
    assert without.total > r.total > 0
    check_matrix(eng, ds, score, rng, r, "copies, matrix")
    want = eng.sdav_similarity_matrix(ds, score, 10.0, -10.0, want_int64=False)[0].clone()
    assert bool(torch.isinf(want[2, ds.shape[0] - 1]))               # the repeated frame
    check_stream(eng, ds, score, want, fo.stream_query_counts(r), "copies, stream")
    print(fo.summary_line(r, "copies") + "; %d without the copy rule" % without.total)
