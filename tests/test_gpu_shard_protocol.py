"""The sharded cosine top-k protocol (include/dlc.h, "Stage 2 split once more") stage by stage on one GPU, against the host
definitions and the fp64 scores of tests/shard_protocol_oracle.py (pinned without a GPU by test_shard_protocol_cpu.py).

run_protocol emulates the ranks through the Engine methods MatchPipeline calls -- score_groups, select_groups,
rescore_topk, topk_merge_packed, exhaustive_topk -- with a workspace per shard, every output buffer pre-filled with a
sentinel, the all-gathers as copies, and the exhaustive round run with the merge's own statuses.  The assertions A - F are
shard_protocol_oracle.check_trace (the ones the CPU file shows to catch five modelled defects); B's and G's comparisons
with the one-shot match_topk, the sentinels and the refusals of the raw C ABI are here.

Tolerances: tau only -- dlc_cosine_score_error_bound(q, n_shard, d, k) per shard, dlc_cosine_score_error_bound_any_plan(d)
for the merge (the oracle restates it: compared below), each times the query's tau_scale -- and the factor 4 behind
must_certify.  Everything else is compared by bit pattern.

Measured on one MI355X: the 35 tests of this file take 4.8 s on their own (33 cases + the two refusal tests, the slowest
case 0.5 s), beside 205 s for the rest of the GPU suite (840 tests in 210 s with this file).  Queries with status 0 / 1 after the first merge / 2 after
the round, per case: crowded-bf16 and crowded-fp16 4 / 1 / 1 (query 0, the one with copies in kg + 1 groups of shard 1);
zero-query 2 / 1 / 1 (the zero row); every other case certifies every query at once -- tiny-k* 5 / 0 / 0, edges-* 6 / 0 / 0,
fewgroups-q3 3 / 0 / 0, fewgroups-q7 7 / 0 / 0, merge-limit 5 / 0 / 0, dense-boundary and foreign-dense 9 / 0 / 0,
onepass-boundary and foreign-onepass 8 / 0 / 0, splitk-q5 5 / 0 / 0, splitk-q2 2 / 0 / 0, gemv-lds-8192 and -8256
4 / 0 / 0, qtail-193 / -256 / -257 all of their queries, ties and ties-offset 4 / 0 / 0, filtered-shard 3 / 0 / 0.  Every
must_not_certify query came out 1 then 2, every must_certify query 0; no stage failed a check, so cosine_topk.hip is
unchanged.  Nothing of the table was left out or could not be run.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import shard_protocol_oracle as spo

pytestmark = pytest.mark.gpu

S32 = 0x5A5A5A5A
S64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def eng(dlc):
    return dlc.default_engine()


def upload(eng, a, dtype):
    """Stored values (float64, exact in the stored type) -> a device tensor of that type."""
    dt = torch.bfloat16 if dtype == "bf16" else torch.float16
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    assert torch.equal(t.double(), torch.from_numpy(np.ascontiguousarray(a)))
    return t.to(eng.device)


def filled(eng, shape, dtype):
    """A device buffer holding the sentinel word everywhere."""
    if dtype in (torch.int64, torch.float64):
        return torch.full(shape, S64, dtype=torch.int64, device=eng.device).view(dtype)
    return torch.full(shape, S32, dtype=torch.int32, device=eng.device).view(dtype)


def untouched(t):
    w = t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)
    return bool((w == (S64 if t.element_size() == 8 else S32)).all())


def written(t):
    """No element still holds the sentinel."""
    w = t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)
    return not bool((w == (S64 if t.element_size() == 8 else S32)).any())


def np_(t):
    return t.detach().cpu().numpy()


def tau_scale_of(eng, case, q, db):
    """Foreign norms: cosine_tau_scale(q, the largest max_row_norm of the shards), the array every stage is given; it must
    lie between the exact max(1, |q| R / 1.01) and the upper bound the oracle derived the classes with."""
    if not case.foreign:
        return None
    r = torch.zeros((1,), dtype=torch.float32, device=eng.device)
    for s in range(case.parts):
        lo, hi = case.shard(s)
        eng.max_row_norm(db[lo:hi], out=r)
    ts = eng.cosine_tau_scale(q, r)
    exact = np.maximum(1.0, np.sqrt((case.q ** 2).sum(axis=1)) * np.sqrt((case.x ** 2).sum(axis=1).max()) / 1.01)
    got = np_(ts).astype(np.float64)
    assert (got >= exact).all() and (got <= case.scale).all(), (got, exact, case.scale)
    return ts


def run_protocol(eng, case, coop):
    """The ranks of the protocol one after the other on one GPU.  coop: the small-footprint kernels on the odd shards in
    select_groups and on the even ones in rescore_topk (False: the other way round).  Returns (trace, device operands)."""
    c, k, kg, nq, d = case, case.k, case.kg, case.nq, case.d
    q, db = upload(eng, c.q, c.dtype), upload(eng, c.x, c.dtype)
    ts = tau_scale_of(eng, c, q, db)
    t = spo.Trace()
    t.scale = np.ones(nq) if ts is None else np_(ts).astype(np.float64)
    t.ids, t.gmax, t.un_s, t.un_i, t.part_s, t.part_i, t.bnd, t.tau_shard, t.ex_s, t.ex_i = ([] for _ in range(10))
    tau_any = eng.score_error_bound_any_plan(d)
    assert tau_any == spo.tau_any(d) == c.tau, (tau_any, spo.tau_any(d))             # the restated formula is the library's
    wss, ids, gms = [], [], []
    for r in range(c.parts):
        lo, hi = c.shard(r)
        ws = torch.empty(eng.topk_workspace_bytes(nq, hi - lo, d, k), dtype=torch.uint8, device=eng.device)
        gi, gm = filled(eng, (nq, kg), torch.int32), filled(eng, (nq, kg + 1), torch.float32)
        eng.score_groups(q, db[lo:hi], k, ws)
        eng.select_groups(q, db[lo:hi], k, ws, gi, gm, coop=(r % 2 == 1) == coop)
        tau_r = eng.score_error_bound(nq, hi - lo, d, k)
        assert 0.0 < tau_r <= tau_any, (r, tau_r, tau_any)
        assert written(gm), "select_groups left a maximum unwritten"
        wss.append(ws), ids.append(gi), gms.append(gm)
        t.ids.append(np_(gi)), t.gmax.append(np_(gm)), t.tau_shard.append(tau_r)
    all_max = torch.stack(gms)                                                       # the first all-gather
    t.all_max = np_(all_max)
    slot = {r: j for j, r in enumerate(c.gather_order)}                              # where shard r's part lands
    gathered = torch.full((c.parts, nq * k * 16), 0x5A, dtype=torch.uint8, device=eng.device)

    def part(r):
        row = gathered[slot[r]]
        return row[nq * k * 8:].view(torch.float64).view(nq, k), row[:nq * k * 8].view(torch.int64).view(nq, k)
    bounds = []
    for r in range(c.parts):
        lo, hi = c.shard(r)
        s2, i2 = filled(eng, (nq, k), torch.float64), filled(eng, (nq, k), torch.int64)
        eng.rescore_topk(q, db[lo:hi], k, ids[r], gms[r], s2, i2, all_max=None, row_offset=c.row_offset(r),
                         coop=(r % 2 == 0) == coop, tau_scale=ts)
        sc, ix = part(r)
        b = filled(eng, (nq,), torch.float32)
        eng.rescore_topk(q, db[lo:hi], k, ids[r], gms[r], sc, ix, bound=b, all_max=all_max, row_offset=c.row_offset(r),
                         coop=(r % 2 == 0) == coop, tau_scale=ts)
        assert written(s2) and written(i2) and written(sc) and written(ix) and written(b), r
        assert torch.equal(ids[r], torch.from_numpy(t.ids[r]).to(eng.device)), "rescore_topk wrote to its group list"
        t.un_s.append(np_(s2)), t.un_i.append(np_(i2)), t.part_s.append(np_(sc)), t.part_i.append(np_(ix))
        t.bnd.append(np_(b)), bounds.append(b)
        # B: where the shard's one-shot call certified at once, the unfiltered re-score is its result, bit for bit
        one = eng.match_topk(q, db[lo:hi], k, row_offset=c.row_offset(r), details=True, tau_scale=ts)
        ok = one.status == 0
        assert torch.equal(one.idx[ok], i2[ok]) and torch.equal(one.scores_f64[ok].view(torch.int64), s2[ok].view(torch.int64)), r
    m_s32, m_s64, m_i = (filled(eng, (nq, k), torch.float32), filled(eng, (nq, k), torch.float64),
                         filled(eng, (nq, k), torch.int64))
    status = filled(eng, (nq,), torch.int32)
    eng.topk_merge_packed(gathered, nq, k, out=(m_s32, m_i), bound=bounds[0], tau=tau_any, scores_f64=m_s64, status=status,
                          tau_scale=ts)
    assert written(m_s32) and written(m_s64) and written(m_i) and written(status)
    t.m_s32, t.m_s64, t.m_i, t.status = np_(m_s32), np_(m_s64), np_(m_i), np_(status)
    # the exhaustive round with the merge's own statuses: each rank holds its own copy of them
    lower = m_s64[:, k - 1].contiguous()
    for r in range(c.parts):
        lo, hi = c.shard(r)
        sc, ix = part(r)
        st = status.clone()
        eng.exhaustive_topk(q, db[lo:hi], k, wss[r], lower, tau_any, st, sc, ix, row_offset=c.row_offset(r), tau_scale=ts)
        assert torch.equal(st, torch.where(status == 1, torch.full_like(status, 2), status)), (r, st, status)
        t.ex_s.append(np_(sc)), t.ex_i.append(np_(ix))
    f_s32, f_s64, f_i = (filled(eng, (nq, k), torch.float32), filled(eng, (nq, k), torch.float64),
                         filled(eng, (nq, k), torch.int64))
    eng.topk_merge_packed(gathered, nq, k, out=(f_s32, f_i), scores_f64=f_s64)
    assert written(f_s32) and written(f_s64) and written(f_i)
    t.f_s32, t.f_s64, t.f_i = np_(f_s32), np_(f_s64), np_(f_i)
    t.status2 = np.where(t.status == 1, 2, t.status).astype(np.int32)                # (asserted per rank above)
    return t, (q, db, ts)


@pytest.mark.parametrize("name", spo.CASES)
def test_protocol_stage_by_stage(eng, name):
    c = spo.build_case(name)
    t, (q, db, ts) = run_protocol(eng, c, coop=not c.flip)
    print("shard-protocol case %s: status 0 / 1 / 2 = %d / %d / %d" % ((name,) + spo.status_counts(t)))
    spo.check_trace(c, t)                                                            # A - F
    # G: the one-shot call on the whole database
    one = eng.match_topk(q, db, c.k, row_offset=c.base_offset, details=True, tau_scale=ts)
    assert np.array_equal(np_(one.idx), t.f_i)
    assert spo.same_bits(np_(one.scores_f64), t.f_s64) and spo.same_bits(np_(one.scores), t.f_s32)
    for j, cls in enumerate(c.classes):                                              # (D and F state it; said once more)
        assert cls != spo.MUST or (t.status[j], t.status2[j]) == (0, 0), (name, j)
        assert cls != spo.MUST_NOT or (t.status[j], t.status2[j]) == (1, 2), (name, j)
    if c.empty_shard is not None:                                                    # a fully filtered shard
        r = c.empty_shard
        assert (t.part_i[r] == -1).all() and (t.part_s[r] == -np.inf).all()
        assert spo.same_bits(spo.bound(np.delete(t.all_max, r, axis=0), c.kg), t.bnd[0])
    if c.zero_query is not None:
        j = c.zero_query
        assert t.f_i[j].tolist() == list(range(c.k)) and spo.same_bits(t.f_s64[j], np.zeros(c.k))
    if name.startswith("ties"):                                                      # the copies, lower global row first
        lo = c.bounds[:4] + c.base_offset
        assert t.f_i[0, :4].tolist() == [lo[0] + 10, lo[1] + 17, lo[2] + 5, lo[3] + 100]
        assert t.f_i[1, :4].tolist() == [lo[0] + 11, lo[1] + 81, lo[2] + 69, lo[3] + 164]
    if c.base_offset:
        assert (t.f_i[t.f_i >= 0] > 2 ** 32).all()


# ---- bad arguments, through the raw C ABI: a status, and nothing written ---------------------------------------------------
def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


REFUSED = (-1, -2)                                                                   # DLC_ERR_BAD_ARG, DLC_ERR_BAD_SHAPE


def test_merge_refuses_bad_arguments(eng, dlc):
    from deeploopcloser_amd import _lib as L
    nq = 2

    def call(parts, k, s_stride=None, i_stride=None, tau=1e-6, bound=True):
        ps = torch.zeros((max(parts, 1), nq, k), dtype=torch.float64, device=eng.device)
        pi = torch.arange(max(parts, 1) * nq * k, dtype=torch.int64, device=eng.device).view(max(parts, 1), nq, k)
        outs = [filled(eng, (nq, k), torch.float32), filled(eng, (nq, k), torch.float64), filled(eng, (nq, k), torch.int64),
                filled(eng, (nq,), torch.int32)]
        b = torch.zeros((nq,), dtype=torch.float32, device=eng.device) if bound else None
        rc = eng.lib.dlc_topk_merge_strided(eng.ctx, _vp(ps), nq * k if s_stride is None else s_stride, _vp(pi),
                                            nq * k if i_stride is None else i_stride, parts, nq, k, _vp(b), tau, None,
                                            _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(outs[3]), None)
        torch.cuda.synchronize()
        return rc, all(untouched(o) for o in outs)
    assert call(16, 128) == (0, False)                                               # parts * k = 2048: the limit itself
    assert call(2049, 1) == (L.DLC_ERR_BAD_SHAPE, True)
    assert call(683, 3) == (L.DLC_ERR_BAD_SHAPE, True)
    for kw in (dict(parts=0, k=4), dict(parts=-1, k=4), dict(parts=3, k=4, tau=-1e-9), dict(parts=3, k=4, tau=float("nan")),
               dict(parts=3, k=4, s_stride=nq * 4 - 1), dict(parts=3, k=4, i_stride=nq * 4 - 1), dict(parts=3, k=0),
               dict(parts=3, k=129)):
        rc, clean = call(**kw)
        assert rc in REFUSED and clean, (kw, rc)
    assert call(3, 4, tau=0.0) == (0, False)


def test_rescore_and_exhaustive_refuse_bad_arguments(eng, dlc):
    from deeploopcloser_amd import _lib as L
    c = spo.build_case("tiny-k3-bf16")
    nq, k, kg, d = c.nq, c.k, c.kg, c.d
    q, db = upload(eng, c.q, c.dtype), upload(eng, c.x, c.dtype)
    n = db.shape[0]
    ws = torch.empty(eng.topk_workspace_bytes(nq, n, d, k), dtype=torch.uint8, device=eng.device)
    gi, gm = filled(eng, (nq, kg), torch.int32), filled(eng, (nq, kg + 1), torch.float32)
    eng.score_groups(q, db, k, ws)
    eng.select_groups(q, db, k, ws, gi, gm)
    all_max = gm.unsqueeze(0).contiguous()

    def rescore(parts, am):
        outs = [filled(eng, (nq, k), torch.float64), filled(eng, (nq, k), torch.int64), filled(eng, (nq,), torch.float32)]
        rc = eng.lib.dlc_cosine_rescore_topk(eng.ctx, L.DLC_BF16, _vp(q), nq, q.stride(0), _vp(db), n, db.stride(0), d, k, 0,
                                             _vp(gi), _vp(gm), _vp(am), parts, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), None,
                                             0, None)
        torch.cuda.synchronize()
        return rc, all(untouched(o) for o in outs)
    assert rescore(1, all_max) == (0, False) and rescore(0, None) == (0, False)
    for parts, am in ((-1, all_max), (1, None), (3, None)):
        rc, clean = rescore(parts, am)
        assert rc in REFUSED and clean, (parts, rc)

    def exhaustive(tau, stride):
        lower = torch.zeros((nq,), dtype=torch.float64, device=eng.device)
        st = torch.ones((nq,), dtype=torch.int32, device=eng.device)
        outs = [filled(eng, (nq, k), torch.float32), filled(eng, (nq, k), torch.float64), filled(eng, (nq, k), torch.int64)]
        rc = eng.lib.dlc_cosine_exhaustive_topk(eng.ctx, L.DLC_BF16, _vp(q), nq, q.stride(0), _vp(db), n, db.stride(0), d, k, 0,
                                                _vp(lower), stride, tau, None, _vp(st), _vp(outs[0]), _vp(outs[1]),
                                                _vp(outs[2]), _vp(ws), ws.numel(), None)
        torch.cuda.synchronize()
        return rc, all(untouched(o) for o in outs) and bool((st == 1).all())
    for tau, stride in ((-1e-9, 1), (float("nan"), 1), (1e-6, -1)):
        rc, clean = exhaustive(tau, stride)
        assert rc in REFUSED and clean, (tau, stride, rc)
    assert exhaustive(1e-6, 1) == (0, False)
    assert exhaustive(1e-6, 0) == (0, False)                                         # stride 0: one lower for every query
