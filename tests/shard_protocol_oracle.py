"""NumPy restatement of the sharded cosine top-k protocol (include/dlc.h, "Stage 2 split once more"; MatchPipeline):

    1. score pass + dlc_cosine_select_groups   -> group_ids [q, kg], group_max [q, kg + 1] per shard
    2. all-gather of group_max, dlc_cosine_rescore_topk (filter, fp64 re-score, bound)
    3. all-gather of the parts, dlc_topk_merge_strided (merge, certificate)
    4. dlc_cosine_exhaustive_topk for the queries with status 1, merge again.

Three things live here, none of which needs a GPU:
  * build_case(name): the operands of every case of the table (stored values as float64), the shard cuts and the CLASS of
    every query -- must_certify / must_not_certify / free -- derived from the fp64 scores of cosine_rows_oracle.chain_scores;
  * the host definitions of what each stage hands out (surviving, bound, status, part_list, merge), all taking the fp32
    group maxima the score pass produced -- the one input whose bits the contract does not fix;
  * simulate(case, score_pass): the whole protocol on the host, and check_trace(case, trace): the assertions A - F of
    tests/test_gpu_shard_protocol.py, written once and run on simulate's trace (test_shard_protocol_cpu.py, with five
    modelled defects that each of them must catch) and on the GPU's.

Tolerances.  The only ones are the library's tau -- per shard dlc_cosine_score_error_bound(q, n_shard, d, k), for the merge
tau_any(d), restated below from cosine_topk.hip and compared with the library's number on the GPU -- times the query's
tau_scale, and the factor 4 of must_certify (derived below).  Everything else is compared by bit pattern.
"""
import functools
import os
import sys

import numpy as np

import cosine_rows_oracle as cro

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.cosine import merge_topk                                         # noqa: E402

GROUP, SLACK, BLOCK = 8, 4, 4096
BIG_OFFSET = 3 * 2 ** 31 + 5
MUST, MUST_NOT, FREE = "must_certify", "must_not_certify", "free"
DEFECTS = ("filter_ge", "bound_without_other_rests", "merge_ties_by_part", "exhaustive_without_tau", "offset_int32")


def groups_per_query(k):
    return k + SLACK


def tau_any(d):
    """dlc_cosine_score_error_bound_any_plan(d): 2^-23 * 1.01 * steps + 3.7e-12 with steps the longer of the unsplit MFMA
    pass's 2 * (d / 64) + 2 and the bandwidth kernel's (d / 64) / 2 + 8 (cosine_topk.hip::score_error_bound)."""
    nk = float(d // 64)
    return 2.0 ** -23 * 1.01 * max(2.0 * nk + 2.0, nk * 0.5 + 8.0) + 3.7e-12


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def chain_scores_narrow(q, x):
    """cosine_rows_oracle.chain_scores bit for bit (pinned by test_shard_protocol_cpu.py) without the lanes that hold no
    piece of a short row: a chain that starts at +0.0 never ends at -0.0, so a lane without a piece adds +0.0, which changes
    nothing, and lane 0 of the xor butterfly holds the sum of the halving tree a[:h] + a[h:] (h = 32, 16, ..., 1; fp64
    addition commutes).  With P = the lanes in use rounded up to a power of two the tree starts at h = P / 2.  For finite
    operands only; a 64-wide row costs an eighth of the full form."""
    d = q.shape[1]
    assert x.shape[1] == d and d % cro.PIECE == 0 and np.isfinite(q).all() and np.isfinite(x).all()
    pieces = d // cro.PIECE
    steps = -(-pieces // cro.LANES)
    used = 1
    while used < min(pieces, cro.LANES):
        used *= 2
    pad = steps * cro.LANES * cro.PIECE - d

    def laid(a):                                                      # [rows, step, lane, element]
        return np.pad(a, ((0, 0), (0, pad))).reshape(a.shape[0], steps, cro.LANES, cro.PIECE)[:, :, :used]
    ql, xl = laid(q), laid(x)
    acc = np.zeros((q.shape[0], x.shape[0], used))
    for s in range(steps):
        has_piece = (s * cro.LANES + np.arange(used)) < pieces
        for e in range(cro.PIECE):
            acc = np.where(has_piece, acc + ql[:, None, s, :, e] * xl[None, :, s, :, e], acc)
    while acc.shape[2] > 1:
        h = acc.shape[2] // 2
        acc = acc[:, :, :h] + acc[:, :, h:]
    return np.ascontiguousarray(acc[:, :, 0])


def chain_scores_blocked(q, x):
    """The fp64 score of every pair, in blocks of BLOCK database rows (the [Q, N, lanes] intermediate is large)."""
    out = np.empty((q.shape[0], x.shape[0]))
    for lo in range(0, x.shape[0], BLOCK):
        out[:, lo:lo + BLOCK] = chain_scores_narrow(q, x[lo:lo + BLOCK])
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------
class Case:
    """name; q [Q, d], x [N, d]: stored values as float64; cuts: rows per shard; k; dtype 'bf16' / 'fp16'; base_offset: the
    global id of row 0; classes [Q]; scale [Q] float64: an upper bound of the tau_scale the library computes (all 1 for
    unit rows); foreign: the GPU test passes cosine_tau_scale's array to every stage; gather_order: the order in which the
    parts reach the merge (a permutation of the shards: an all-gather's rank order need not be the order of the rows);
    flip: coop the other way round; crowded / separated / empty_shard / zero_query: what the row of the table claims."""

    def __init__(self, **kw):
        self.base_offset, self.foreign, self.flip = 0, False, False
        self.crowded, self.separated, self.empty_shard, self.zero_query = [], [], None, None
        self.__dict__.update(kw)
        self.nq, self.d = self.q.shape
        self.parts = len(self.cuts)
        self.bounds = np.concatenate([[0], np.cumsum(self.cuts)]).astype(np.int64)
        self.n = int(self.bounds[-1])
        assert self.x.shape == (self.n, self.d) and self.d % 64 == 0
        self.kg = groups_per_query(self.k)
        self.tau = tau_any(self.d)
        if "gather_order" not in kw:
            self.gather_order = list(range(self.parts))
        if "scale" not in kw:
            self.scale = np.ones(self.nq)
        if "scores" not in kw:
            self.scores = chain_scores_blocked(self.q, self.x)
        self.keys = cro.f64_key(self.scores)
        kk = min(self.k + 1, self.n)                                          # k + 1 columns when there are that many rows
        self.top_i = cro.rank_by_key(self.keys, kk)
        self.top_s = np.take_along_axis(self.scores, self.top_i, 1)
        self.classes = self._classes()

    def shard(self, r):
        return int(self.bounds[r]), int(self.bounds[r + 1])

    def row_offset(self, r):
        return self.base_offset + int(self.bounds[r])

    def want(self):
        """The global top-k: (fp64 scores [Q, k], global ids [Q, k]), (-inf, -1) past the database's rows."""
        s = np.full((self.nq, self.k), -np.inf)
        i = np.full((self.nq, self.k), -1, dtype=np.int64)
        m = min(self.k, self.n)
        s[:, :m], i[:, :m] = self.top_s[:, :m], self.top_i[:, :m] + self.base_offset
        return s, i

    def _classes(self):
        """must_certify: s_k - s_{k+1} > 4 tau scale.  A row left behind by every shard is not one of the k best: were a
        top-k row's group dropped, kg groups would hold an fp32 score above its own, so k + 4 rows an fp64 score above
        s_k - 2 tau -- but beyond the k best there is none above s_k - 4 tau.  So what is left behind scores at most
        s_{k+1} + tau in fp32, the bound is at most that, and s_k > s_{k+1} + 2 tau forces status 0; the factor 4 is a
        margin of 2 on the derived 2.  (Fewer than k + 1 rows: nothing can be left behind that matters -- see below.)
        must_not_certify: the query is a stored row with exact copies in kg + 1 groups of one shard.  One copy's group is
        then unlisted, the bound is at least that copy's fp32 score >= s_copy - tau, and with s_k <= s_copy (checked here
        on the fp64 scores) s_k > bound + tau is impossible.  A zero query scores +0.0 against every row in fp32 and fp64
        alike: where a shard has more than kg groups the bound is 0.0 = s_k."""
        out = []
        for i in range(self.nq):
            if self.n > self.k:
                gap = self.top_s[i, self.k - 1] - self.top_s[i, self.k]
            else:
                # at most k rows: at most k groups, fewer than kg, so every group of every shard is listed, survives
                # (fewer than kg maxima exist) and the bound is -inf
                gap = np.inf
            cls = MUST if gap > 4.0 * self.tau * self.scale[i] else FREE
            copies = np.nonzero((self.x == self.q[i]).all(axis=1))[0]
            crowded = False
            for r in range(self.parts):
                lo, hi = self.shard(r)
                mine = copies[(copies >= lo) & (copies < hi)]
                crowded |= len(np.unique((mine - lo) // GROUP)) >= self.kg + 1
            zero = not self.q[i].any() and any(-(-c // GROUP) > self.kg for c in self.cuts)
            if crowded and self.n >= self.k and self.top_s[i, self.k - 1] <= self.scores[i, copies[0]]:
                cls = MUST_NOT
            if zero and self.n >= self.k:
                cls = MUST_NOT
            assert not (cls == MUST_NOT and gap > 4.0 * self.tau * self.scale[i])
            out.append(cls)
        return out


def _stored(x, dtype):
    import torch
    return cro.stored(x, torch.bfloat16 if dtype == "bf16" else torch.float16)


def _unit(rng, n, d):
    x = rng.standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _random_case(name, cuts, nq, k, d, dtype, seed, **kw):
    """Unit rows; the first queries are noisy copies of database rows spread over the shards, the rest are random."""
    rng = np.random.RandomState(seed)
    n = int(sum(cuts))
    x = _unit(rng, n, d)
    q = _unit(rng, nq, d)
    near = rng.permutation(n)[:(nq + 1) // 2]
    q[:len(near)] = x[near] + 0.3 * _unit(rng, len(near), d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return Case(name=name, q=_stored(q, dtype), x=_stored(x, dtype), cuts=tuple(cuts), k=k, dtype=dtype, **kw)


def _uneven16():
    return tuple(300 + ((7 * r) % 16) * 3 - 20 for r in range(16))           # 280 .. 325 rows, no two neighbours alike


def _ties(dtype="bf16"):
    """Rows 10 and 11 of shard 0 are copied into the three other shards: every copy has the query's key, the lower global
    row comes first.  Query 0 = row 10, query 1 = row 11; the parts reach the merge in reverse rank order."""
    cuts, k, d = (300, 500, 260, 400), 20, 64
    rng = np.random.RandomState(101)
    x = _unit(rng, sum(cuts), d)
    b = np.concatenate([[0], np.cumsum(cuts)])
    for r, off in ((1, 17), (2, 5), (3, 100)):
        x[b[r] + off] = x[10]
        x[b[r] + off + 64] = x[11]
    q = np.concatenate([x[[10, 11]], _unit(rng, 2, d)])
    return Case(name="ties", q=_stored(q, dtype), x=_stored(x, dtype), cuts=cuts, k=k, dtype=dtype,
                gather_order=[3, 2, 1, 0])


def _crowded(dtype):
    """Query 0 = a stored row with copies in kg + 1 = 25 groups of shard 1 and in two groups each of shards 0 and 2 (29
    copies >= k: the k-th score is the copy's).  Queries 1 .. 4: k planted neighbours at ~0.95, everything else below 0.7."""
    cuts, k, d, nq = (600, 1000, 500), 20, 64, 5
    kg = groups_per_query(k)
    rng = np.random.RandomState(202)
    n = sum(cuts)
    x = _unit(rng, n, d)
    q = _unit(rng, nq, d)
    copies = [13, 200] + [600 + GROUP * (3 * g) + (g % GROUP) for g in range(kg + 1)] + [1600 + 77, 1600 + 301]
    free = np.setdiff1d(np.arange(n), copies)
    spots = rng.permutation(free)[:(nq - 1) * k].reshape(nq - 1, k)
    for j in range(1, nq):
        x[spots[j - 1]] = q[j] + 0.3 * _unit(rng, k, d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[copies] = q[0]
    xs, qs = _stored(x, dtype), _stored(q, dtype)
    return Case(name="crowded-" + dtype, q=qs, x=xs, cuts=cuts, k=k, dtype=dtype, crowded=[0], separated=[1, 2, 3, 4])


def _zero_query():
    c = _random_case("zero-query", (400, 300), 3, 5, 64, "bf16", 303)
    q = c.q.copy()
    q[1] = 0.0
    return Case(name="zero-query", q=q, x=c.x, cuts=c.cuts, k=c.k, dtype="bf16", zero_query=1, crowded=[1])


def _filtered_shard():
    """Shard 1 holds only the direction opposite to all three queries: each of its groups has a negative maximum and kg
    larger ones elsewhere, so the filter drops all of them; what the other shards leave behind is larger."""
    cuts, k, d = (400, 64, 300), 5, 64
    rng = np.random.RandomState(404)
    x = _unit(rng, sum(cuts), d)
    q = _unit(rng, 3, d)
    anti = -q.sum(axis=0) / np.linalg.norm(q.sum(axis=0))
    x[400:464] = anti[None, :] * (1.0 - 0.004 * np.arange(64))[:, None]
    return Case(name="filtered-shard", q=_stored(q, "bf16"), x=_stored(x, "bf16"), cuts=cuts, k=k, dtype="bf16", empty_shard=1)


def _foreign(base, name):
    """The base case with every database row times 8: exact in the stored type and in every product and sum, so each fp64
    score is the base case's times 8.  scale: an upper bound of dlc_cosine_tau_scale's max(1, |q| R / 1.01) -- the library
    over-reports the norms by less than a factor 1.002 each (include/dlc.h)."""
    b = build_case(base)
    x = b.x * 8.0
    r = np.sqrt((x * x).sum(axis=1).max())
    scale = np.maximum(1.0, np.sqrt((b.q * b.q).sum(axis=1)) * r / 1.01) * 1.002 * 1.002
    return Case(name=name, q=b.q, x=x, cuts=b.cuts, k=b.k, dtype=b.dtype, scores=b.scores * 8.0, scale=scale, foreign=True)


def _with_offset(base, name):
    b = build_case(base)
    return Case(name=name, q=b.q, x=b.x, cuts=b.cuts, k=b.k, dtype=b.dtype, scores=b.scores, base_offset=BIG_OFFSET,
                gather_order=b.gather_order)


def _flipped(base, name):
    b = build_case(base)
    return Case(name=name, q=b.q, x=b.x, cuts=b.cuts, k=b.k, dtype=b.dtype, scores=b.scores, flip=True)


TINY, EDGES = (1, 7, 8, 9, 3), (127, 128, 129, 255, 256, 257)
_BUILDERS = {}
for _dt in ("bf16", "fp16"):
    for _k in (1, 3, 20, 128):
        _BUILDERS["tiny-k%d-%s" % (_k, _dt)] = functools.partial(_random_case, cuts=TINY, nq=5, k=_k, d=64, dtype=_dt, seed=1)
    _BUILDERS["edges-" + _dt] = functools.partial(_random_case, cuts=EDGES, nq=6, k=20, d=64, dtype=_dt, seed=2)
    _BUILDERS["crowded-" + _dt] = functools.partial(lambda name, dtype: _crowded(dtype), dtype=_dt)
_BUILDERS.update({
    "fewgroups-q3": functools.partial(_random_case, cuts=(1000, 1056, 1057, 2000), nq=3, k=128, d=64, dtype="bf16", seed=3),
    "fewgroups-q7": functools.partial(_random_case, cuts=(1000, 1056, 1057, 2000), nq=7, k=128, d=64, dtype="bf16", seed=4),
    "merge-limit": functools.partial(_random_case, cuts=_uneven16(), nq=5, k=128, d=64, dtype="bf16", seed=5),
    "dense-boundary": functools.partial(_random_case, cuts=(16384, 16385, 300), nq=9, k=20, d=128, dtype="bf16", seed=6),
    "onepass-boundary": functools.partial(_random_case, cuts=(65536, 70001, 5000), nq=8, k=20, d=64, dtype="bf16", seed=7),
    "splitk-q5": functools.partial(_random_case, cuts=(300, 2000, 37), nq=5, k=7, d=2048, dtype="bf16", seed=8),
    "splitk-q2": functools.partial(_random_case, cuts=(300, 2000, 37), nq=2, k=7, d=2048, dtype="bf16", seed=9),
    "gemv-lds-8192": functools.partial(_random_case, cuts=(257, 100), nq=4, k=5, d=8192, dtype="bf16", seed=10),
    "gemv-lds-8256": functools.partial(_random_case, cuts=(257, 100), nq=4, k=5, d=8256, dtype="bf16", seed=11),
    "qtail-193": functools.partial(_random_case, cuts=(700, 900), nq=193, k=4, d=64, dtype="bf16", seed=12),
    "qtail-256": functools.partial(_random_case, cuts=(700, 900), nq=256, k=4, d=64, dtype="bf16", seed=13),
    "qtail-257": functools.partial(_random_case, cuts=(700, 900), nq=257, k=4, d=64, dtype="bf16", seed=14),
    "ties": lambda name: _ties(),
    "zero-query": lambda name: _zero_query(),
    "filtered-shard": lambda name: _filtered_shard(),
    "tiny-k3-bf16-offset": functools.partial(lambda name: _with_offset("tiny-k3-bf16", name)),
    "edges-fp16-offset": functools.partial(lambda name: _with_offset("edges-fp16", name)),
    "ties-offset": functools.partial(lambda name: _with_offset("ties", name)),
    "edges-bf16-flip": functools.partial(lambda name: _flipped("edges-bf16", name)),
    "foreign-dense": functools.partial(lambda name: _foreign("dense-boundary", name)),
    "foreign-onepass": functools.partial(lambda name: _foreign("onepass-boundary", name)),
})
CASES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def build_case(name):
    return _BUILDERS[name](name=name)


# ---- host definitions -------------------------------------------------------------------------------------------------
def _lists(all_max, kg):
    """[q, parts * kg] fp32: every listed maximum of a query, shard after shard."""
    a = np.asarray(all_max, dtype=np.float32)
    return a[:, :, :kg].transpose(1, 0, 2).reshape(a.shape[1], -1)


def surviving(all_max, kg):
    """bool [parts, q, kg]: entry (p, i, e) survives unless kg or more listed maxima of query i, over all shards, are
    STRICTLY larger than it (an empty entry, -inf, never survives)."""
    a = np.asarray(all_max, dtype=np.float32)
    flat = _lists(a, kg)                                                       # [q, parts * kg]
    own = a[:, :, :kg]
    greater = (flat[None, :, None, :] > own[:, :, :, None]).sum(axis=3)
    return (greater < kg) & (own != -np.inf)


def bound(all_max, kg):
    """fp32 [q]: the largest fp32 score a row outside the surviving groups of all shards can have -- the maximum of
    every shard's rest column and of every listed maximum that does not survive; -inf when nothing is left behind."""
    a = np.asarray(all_max, dtype=np.float32)
    dropped = np.where(~surviving(a, kg) & (a[:, :, :kg] != -np.inf), a[:, :, :kg], np.float32(-np.inf))
    return np.maximum(dropped.max(axis=(0, 2)), a[:, :, kg].max(axis=0)).astype(np.float32)


def status(kth, bnd, tau, scale):
    """int32 [q]: 0 = certified: nothing was left behind (bound -inf), or the k-th fp64 score (-inf: fewer than k rows
    found) exceeds (double)bound + tau * (double)scale; 1 otherwise."""
    b = np.asarray(bnd, dtype=np.float32).astype(np.float64)
    lim = b + float(tau) * np.asarray(scale, dtype=np.float64)
    return np.where((b == -np.inf) | (np.asarray(kth, dtype=np.float64) > lim), 0, 1).astype(np.int32)


def part_list(scores, keys, groups, n_shard, row_offset, k):
    """A shard's part of one query: the k best rows by (key descending, row ascending) among the rows of `groups`
    (shard-local group indices).  scores / keys: that query's fp64 scores and keys of the shard's rows [n_shard].
    Returns (fp64 scores [k], int64 global rows [k]), (-inf, -1) past the rows found."""
    groups = np.asarray(groups, dtype=np.int64)
    rows = (groups[:, None] * GROUP + np.arange(GROUP)[None, :]).reshape(-1)
    rows = np.unique(rows[rows < n_shard])
    order = rows[np.lexsort((rows, -keys[rows]))][:k]
    s = np.full(k, -np.inf)
    i = np.full(k, -1, dtype=np.int64)
    s[:len(order)], i[:len(order)] = scores[order], order + row_offset
    return s, i


def merge(part_s, part_i, k):
    """[parts, q, k] -> the merged (fp64 scores [q, k], rows [q, k]): oracle/cosine.py::merge_topk, whose order (score
    quantised to 2^-40 descending, lower global row first) is the order of cosine_rows_oracle.f64_key on these values --
    asserted here -- with empty slots (row < 0) last, as (-inf, -1)."""
    ps = np.asarray(part_s, dtype=np.float64).transpose(1, 0, 2).reshape(part_s.shape[1], -1).copy()
    pi = np.asarray(part_i, dtype=np.int64).transpose(1, 0, 2).reshape(part_s.shape[1], -1).copy()
    ps[pi < 0] = -np.inf
    sort_i = np.where(pi < 0, np.iinfo(np.int64).max, pi)                      # empty slots after every row of their key
    s, i = merge_topk(ps, sort_i, k)
    key = cro.f64_key(ps)
    for r in range(ps.shape[0]):
        assert np.array_equal(i[r], sort_i[r][np.lexsort((sort_i[r], -key[r]))][:k])
    i = np.where(i == np.iinfo(np.int64).max, -1, i)
    if s.shape[1] < k:                                                         # (parts * k < k cannot happen; k > columns neither)
        raise AssertionError("merge: fewer candidates than k")
    return s, i


# ---- the protocol on the host -------------------------------------------------------------------------------------------
class Trace:
    """What the stages handed out, as NumPy arrays.  Per shard r (lists): ids [q, kg] int32, gmax [q, kg + 1] fp32,
    un_s / un_i [q, k]: the unfiltered re-score, part_s / part_i [q, k]: the filtered one, bnd [q] fp32, tau_shard (float);
    all_max [parts, q, kg + 1]; merged m_s32 / m_s64 / m_i [q, k] and status [q]; after the exhaustive round the parts
    ex_s / ex_i per shard, the final f_s32 / f_s64 / f_i and status2 [q]; scale [q]: the tau_scale every stage was given."""


def default_score_pass(case):
    return case.scores.astype(np.float32)


def _select(s32, n_shard, kg):
    """One shard's select_groups from its fp32 scores [q, n_shard]: group maxima, the kg largest by (maximum descending,
    group ascending), the largest maximum not listed."""
    nq = s32.shape[0]
    ng = -(-n_shard // GROUP)
    pad = np.full((nq, ng * GROUP), -np.inf, dtype=np.float32)
    pad[:, :n_shard] = s32
    gm = pad.reshape(nq, ng, GROUP).max(axis=2)
    ids = np.full((nq, kg), -1, dtype=np.int32)
    out = np.full((nq, kg + 1), -np.inf, dtype=np.float32)
    for i in range(nq):
        order = np.lexsort((np.arange(ng), -gm[i].astype(np.float64)))
        m = min(kg, ng)
        ids[i, :m], out[i, :m] = order[:m], gm[i, order[:m]]
        if ng > kg:
            out[i, kg] = gm[i, order[kg]]
    return ids, out, gm


def simulate(case, score_pass=None, defect=None):
    """The protocol in NumPy.  score_pass(case) -> fp32 [Q, N]: what the score pass makes of every pair (default: the
    fp64 score rounded to fp32).  defect: one of DEFECTS, a modelled mistake of an implementation."""
    assert defect is None or defect in DEFECTS
    c, k, kg = case, case.k, case.kg
    s32 = (score_pass or default_score_pass)(c)
    assert s32.dtype == np.float32 and s32.shape == c.scores.shape
    t = Trace()
    t.scale = c.scale.astype(np.float32).astype(np.float64)
    t.ids, t.gmax, t.un_s, t.un_i, t.part_s, t.part_i, t.bnd, t.tau_shard, gms = [], [], [], [], [], [], [], [], []
    for r in range(c.parts):
        lo, hi = c.shard(r)
        ids, gmax, gm = _select(s32[:, lo:hi], hi - lo, kg)
        t.ids.append(ids), t.gmax.append(gmax), gms.append(gm), t.tau_shard.append(c.tau)
    t.all_max = np.stack(t.gmax)

    def offset(r):
        o = c.row_offset(r)
        low = o & 0xffffffff
        return (low - (1 << 32) if low >= (1 << 31) else low) if defect == "offset_int32" else o

    alive = surviving(t.all_max, kg)
    if defect == "filter_ge":
        flat = _lists(t.all_max, kg)
        own = t.all_max[:, :, :kg]
        alive = ((flat[None, :, None, :] >= own[:, :, :, None]).sum(axis=3) < kg) & (own != -np.inf)
    for r in range(c.parts):
        lo, hi = c.shard(r)
        us, ui, ps, pi = (np.empty((c.nq, k)), np.empty((c.nq, k), dtype=np.int64), np.empty((c.nq, k)),
                          np.empty((c.nq, k), dtype=np.int64))
        for i in range(c.nq):
            listed = t.ids[r][i][t.ids[r][i] >= 0]
            us[i], ui[i] = part_list(c.scores[i, lo:hi], c.keys[i, lo:hi], listed, hi - lo, offset(r), k)
            kept = t.ids[r][i][alive[r, i] & (t.ids[r][i] >= 0)]
            ps[i], pi[i] = part_list(c.scores[i, lo:hi], c.keys[i, lo:hi], kept, hi - lo, offset(r), k)
        b = bound(t.all_max, kg)
        if defect == "bound_without_other_rests":
            others = t.all_max.copy()
            others[np.arange(c.parts) != r, :, kg] = -np.inf
            b = bound(others, kg)
        t.un_s.append(us), t.un_i.append(ui), t.part_s.append(ps), t.part_i.append(pi), t.bnd.append(b)

    def merged(parts_s, parts_i):
        ps = np.stack([parts_s[r] for r in c.gather_order])
        pi = np.stack([parts_i[r] for r in c.gather_order])
        if defect == "merge_ties_by_part":                                   # (key, position in the gathered buffer)
            pos = np.broadcast_to(np.arange(c.parts * k).reshape(c.parts, 1, k), pi.shape)
            _, at = merge(ps, np.where(pi < 0, -1, pos), k)
            fs, fi = ps.transpose(1, 0, 2).reshape(c.nq, -1), pi.transpose(1, 0, 2).reshape(c.nq, -1)
            safe = np.maximum(at, 0)
            return (np.where(at < 0, -np.inf, np.take_along_axis(fs, safe, 1)),
                    np.where(at < 0, -1, np.take_along_axis(fi, safe, 1)))
        return merge(ps, pi, k)
    t.m_s64, t.m_i = merged(t.part_s, t.part_i)
    t.m_s32 = t.m_s64.astype(np.float32)
    t.status = status(t.m_s64[:, k - 1], t.bnd[0], c.tau, t.scale)

    # the exhaustive round: every group whose fp32 maximum is >= lower - tau * scale, re-scored; the shard's exact list
    t.ex_s, t.ex_i = [p.copy() for p in t.part_s], [p.copy() for p in t.part_i]
    for r in range(c.parts):
        lo, hi = c.shard(r)
        for i in np.nonzero(t.status == 1)[0]:
            theta = t.m_s64[i, k - 1] - (0.0 if defect == "exhaustive_without_tau" else c.tau * t.scale[i])
            groups = np.nonzero(gms[r][i].astype(np.float64) >= theta)[0]
            t.ex_s[r][i], t.ex_i[r][i] = part_list(c.scores[i, lo:hi], c.keys[i, lo:hi], groups, hi - lo, offset(r), k)
    t.status2 = np.where(t.status == 1, 2, t.status).astype(np.int32)
    t.f_s64, t.f_i = merged(t.ex_s, t.ex_i)
    t.f_s32 = t.f_s64.astype(np.float32)
    return t


# ---- the assertions (A - F of the issue; B's and G's comparisons with the one-shot call are the GPU file's) ------------
def check_select(case, r, ids, gmax, tau_shard, scale):
    """A.  ids distinct, inside the shard's groups, -1 only at the end, min(kg, groups) of them; maxima non-increasing,
    equal ones by ascending group (include/dlc.h);
    listed maxima within tau of the fp64 maximum of the group's rows; every unlisted row at most rest + tau; rest -inf
    exactly when every group is listed."""
    lo, hi = case.shard(r)
    kg, ng = case.kg, -(-(hi - lo) // GROUP)
    assert ids.shape == (case.nq, kg) and ids.dtype == np.int32 and gmax.shape == (case.nq, kg + 1) and gmax.dtype == np.float32
    m = min(kg, ng)
    for i in range(case.nq):
        tau = tau_shard * scale[i]
        assert (ids[i, :m] >= 0).all() and (ids[i, :m] < ng).all() and (ids[i, m:] == -1).all(), (r, i, ids[i])
        assert len(np.unique(ids[i, :m])) == m, (r, i, "group listed twice")
        assert (gmax[i, m:kg] == -np.inf).all() and not np.isnan(gmax[i]).any()
        step = np.diff(gmax[i, :m].astype(np.float64))
        assert (step <= 0).all(), (r, i, "maxima not in rank order")
        assert (np.diff(ids[i, :m])[step == 0] > 0).all(), (r, i, "equal maxima: the lower group comes first")
        if not case.q[i].any():                                       # every maximum is +0.0: the list ends inside a tie
            assert np.array_equal(ids[i, :m], np.arange(m)), (r, i, "a tie at the end of the list keeps the lower groups")
        s = np.full(ng * GROUP, -np.inf)
        s[:hi - lo] = case.scores[i, lo:hi]
        g64 = s.reshape(ng, GROUP).max(axis=1)
        err = np.abs(gmax[i, :m].astype(np.float64) - g64[ids[i, :m]])
        assert (err <= tau).all(), (r, i, "listed maximum off by %g > tau %g" % (err.max(), tau))
        rest = float(gmax[i, kg])
        assert (rest == -np.inf) == (ng <= kg), (r, i, rest)
        unlisted = np.setdiff1d(np.arange(ng), ids[i, :m])
        if len(unlisted):
            assert g64[unlisted].max() <= rest + tau, (r, i, "an unlisted row scores %g above rest + tau" %
                                                       (g64[unlisted].max() - rest - tau))
            assert rest <= float(gmax[i, m - 1]), (r, i, "rest above a listed maximum")


def check_unfiltered(case, r, ids, un_s, un_i):
    """B.  parts = 0: the top-k by (key, row) over the rows of the listed groups, scores bit-equal to chain_scores."""
    lo, hi = case.shard(r)
    for i in range(case.nq):
        s, g = part_list(case.scores[i, lo:hi], case.keys[i, lo:hi], ids[i][ids[i] >= 0], hi - lo, case.row_offset(r), case.k)
        assert np.array_equal(un_i[i], g), (r, i, un_i[i], g)
        assert same_bits(un_s[i], s), (r, i)


def check_filtered(case, t):
    """C.  Every shard's list = part_list over surviving(all_max); its bound = bound(all_max) bit for bit (so equal on
    every shard); no row outside the surviving groups of all shards scores above bound + tau_any * scale."""
    alive = surviving(t.all_max, case.kg)
    want_b = bound(t.all_max, case.kg)
    outside = np.ones((case.nq, case.n), dtype=bool)
    for r in range(case.parts):
        lo, hi = case.shard(r)
        assert t.bnd[r].dtype == np.float32 and same_bits(t.bnd[r], want_b), (r, t.bnd[r], want_b)
        for i in range(case.nq):
            kept = t.ids[r][i][alive[r, i] & (t.ids[r][i] >= 0)]
            s, g = part_list(case.scores[i, lo:hi], case.keys[i, lo:hi], kept, hi - lo, case.row_offset(r), case.k)
            assert np.array_equal(t.part_i[r][i], g), (r, i, t.part_i[r][i], g)
            assert same_bits(t.part_s[r][i], s), (r, i)
            rows = (kept.astype(np.int64)[:, None] * GROUP + np.arange(GROUP)[None, :]).reshape(-1)
            outside[i, lo + rows[rows < hi - lo]] = False
    for i in range(case.nq):
        if outside[i].any():
            top = case.scores[i][outside[i]].max()
            assert top <= float(want_b[i]) + case.tau * t.scale[i], (i, "a row left behind scores %g above the bound" %
                                                                      (top - float(want_b[i])))


def check_merge(case, t):
    """D.  idx, fp64 and fp32 scores = merge(parts); status = the host definition; the classes hold."""
    ps = np.stack([t.part_s[r] for r in case.gather_order])
    pi = np.stack([t.part_i[r] for r in case.gather_order])
    s, i = merge(ps, pi, case.k)
    assert np.array_equal(t.m_i, i), (t.m_i, i)
    assert same_bits(t.m_s64, s) and t.m_s32.dtype == np.float32 and same_bits(t.m_s32, s.astype(np.float32))
    want = status(s[:, case.k - 1], t.bnd[0], case.tau, t.scale)
    assert t.status.dtype == np.int32 and np.array_equal(t.status, want), (t.status, want)
    for j, cls in enumerate(case.classes):
        assert not (cls == MUST and t.status[j] != 0), (j, "must certify", t.status[j])
        assert not (cls == MUST_NOT and t.status[j] != 1), (j, "must not certify", t.status[j])


def check_certified(case, t):
    """E.  A certified query already has the global top-k: ids equal, fp64 scores bit-equal to chain_scores."""
    ws, wi = case.want()
    for j in np.nonzero(t.status == 0)[0]:
        assert np.array_equal(t.m_i[j], wi[j]), (j, t.m_i[j], wi[j])
        assert same_bits(t.m_s64[j], ws[j]), j


def check_final(case, t):
    """F.  After the exhaustive round and the second merge every query has the global top-k; status 1 became 2, the
    others stayed; the certified queries' parts are what they were."""
    ws, wi = case.want()
    assert np.array_equal(t.f_i, wi), (np.nonzero((t.f_i != wi).any(axis=1))[0], t.f_i, wi)
    assert same_bits(t.f_s64, ws) and same_bits(t.f_s32, ws.astype(np.float32))
    assert np.array_equal(t.status2, np.where(t.status == 1, 2, t.status)), (t.status, t.status2)
    keep = t.status != 1
    for r in range(case.parts):
        assert same_bits(t.ex_s[r][keep], t.part_s[r][keep]) and np.array_equal(t.ex_i[r][keep], t.part_i[r][keep]), r


def check_trace(case, t):
    for r in range(case.parts):
        check_select(case, r, t.ids[r], t.gmax[r], t.tau_shard[r], t.scale)
        check_unfiltered(case, r, t.ids[r], t.un_s[r], t.un_i[r])
    check_filtered(case, t)
    check_merge(case, t)
    check_certified(case, t)
    check_final(case, t)


def status_counts(t):
    """(status 0, status 1 after the first merge, status 2 after the round)."""
    return int((t.status == 0).sum()), int((t.status == 1).sum()), int((t.status2 == 2).sum())
