"""tests/shard_protocol_oracle.py pinned without a GPU: every case of the table builds and holds the query classes its row
claims; the protocol simulated on the host returns the oracle's global top-k (for every certified query at once, for all
queries after its exhaustive round); and the assertions the GPU test runs on the library's stages (check_trace, A - F) catch
each of five modelled defects of an implementation."""
import numpy as np
import pytest
import torch

import cosine_rows_oracle as cro
import shard_protocol_oracle as spo


# ---- 0. the oracle's own restatements ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 64, 128, 520, 2048, 4160, 8256])
def test_narrow_chain_is_chain_scores(d):
    rng = np.random.RandomState(d)
    q = cro.stored(rng.standard_normal((4, d)), torch.bfloat16)
    x = cro.stored(0.1 * rng.standard_normal((37, d)), torch.float16)
    q[1], x[3], x[5, ::2] = 0.0, 0.0, -0.0
    assert spo.same_bits(spo.chain_scores_narrow(q, x), cro.chain_scores(q, x))


def test_merge_orders_by_key_then_global_row():
    s = np.array([[[0.5, 0.25, -np.inf]], [[0.5, 0.5 + 2.0 ** -42, 0.125]]])              # [parts 2, q 1, k 3]
    i = np.array([[[7, 9, -1]], [[3, 4, 5]]], dtype=np.int64)
    ms, mi = spo.merge(s, i, 3)
    assert mi.tolist() == [[3, 4, 7]] and spo.same_bits(ms, np.array([[0.5, 0.5 + 2.0 ** -42, 0.5]]))   # one key: lower row first
    ms, mi = spo.merge(s[:1], i[:1], 3)
    assert mi.tolist() == [[7, 9, -1]] and ms[0, 2] == -np.inf


def test_host_definitions_on_a_built_list():
    kg = 2                                                                              # [parts 2, q 1, kg + 1]
    a = np.array([[[0.9, 0.5, 0.1]], [[0.9, 0.7, -np.inf]]], dtype=np.float32)
    assert spo.surviving(a, kg).tolist() == [[[True, False]], [[True, False]]]            # 0.7 has two larger ones, 0.5 three
    assert spo.bound(a, kg).tolist() == [float(np.float32(0.7))]
    # equal maxima are not "strictly larger": both 0.9 survive although each sees the other
    b = np.array([[[0.9, 0.9, 0.9]], [[0.9, 0.9, -np.inf]]], dtype=np.float32)
    assert spo.surviving(b, kg).all() and spo.bound(b, kg).tolist() == [float(np.float32(0.9))]
    assert spo.status([0.5, 0.5, -np.inf, -np.inf], np.float32([0.25, 0.5, -np.inf, 0.0]), 1e-6, [1, 1, 1, 1]).tolist() == \
        [0, 1, 0, 1]
    assert spo.status([0.5], np.float32([0.25]), 1e-6, [np.inf]).tolist() == [1]         # a scale of +inf certifies nothing


# ---- 1. the table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", spo.CASES)
def test_case_builds_and_holds_its_classes(name):
    c = spo.build_case(name)
    assert len(c.classes) == c.nq and set(c.classes) <= {spo.MUST, spo.MUST_NOT, spo.FREE}
    assert sum(c.cuts) == c.n and c.q.shape == (c.nq, c.d) and c.d % 64 == 0
    dt = torch.bfloat16 if c.dtype == "bf16" else torch.float16
    assert spo.same_bits(cro.stored(c.q, dt), c.q) and spo.same_bits(cro.stored(c.x, dt), c.x)      # values of the stored type
    assert spo.same_bits(spo.build_case(name).x, c.x)                                                # seeded
    lo = c.n // 2                                                                                    # scores: chain_scores'
    assert spo.same_bits(c.scores[:3, lo:lo + 9], cro.chain_scores(c.q[:3], c.x[lo:lo + 9]))
    for i in c.crowded:
        assert c.classes[i] == spo.MUST_NOT, (name, i)
    for i in c.separated:
        assert c.classes[i] == spo.MUST, (name, i)


def test_table_has_what_the_issue_lists():
    by = {n: spo.build_case(n) for n in ("tiny-k128-bf16", "fewgroups-q3", "merge-limit", "crowded-bf16", "crowded-fp16",
                                          "zero-query", "ties-offset", "foreign-dense", "gemv-lds-8192", "gemv-lds-8256")}
    assert by["tiny-k128-bf16"].k > by["tiny-k128-bf16"].n
    f = by["fewgroups-q3"]
    assert sorted(-(-c // spo.GROUP) - f.kg for c in f.cuts) == [-7, 0, 1, 118]            # fewer than, exactly, one more than kg
    assert by["merge-limit"].parts * by["merge-limit"].k == 2048 and len(set(by["merge-limit"].cuts)) > 8
    for n in ("crowded-bf16", "crowded-fp16"):
        assert by[n].classes == [spo.MUST_NOT] + [spo.MUST] * 4
    assert by["zero-query"].classes[1] == spo.MUST_NOT and not by["zero-query"].scores[1].any()
    assert by["ties-offset"].base_offset == 3 * 2 ** 31 + 5 and by["ties-offset"].gather_order == [3, 2, 1, 0]
    assert by["foreign-dense"].scale.min() > 7.9 and spo.same_bits(by["foreign-dense"].scores,
                                                                  8.0 * spo.build_case("dense-boundary").scores)
    assert 4 * (8192 // 64) * 128 <= 64 * 1024 < 4 * (8256 // 64) * 128                     # either side of the LDS limit


# ---- 2. the simulated protocol is sound ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", spo.CASES)
def test_simulated_protocol_returns_the_global_topk(name):
    c = spo.build_case(name)
    t = spo.simulate(c)
    ws, wi = c.want()
    done = t.status == 0
    assert np.array_equal(t.m_i[done], wi[done]) and spo.same_bits(t.m_s64[done], ws[done])
    assert np.array_equal(t.f_i, wi) and spo.same_bits(t.f_s64, ws)
    spo.check_trace(c, t)
    if c.empty_shard is not None:
        r = c.empty_shard
        assert (t.part_i[r] == -1).all() and (t.part_s[r] == -np.inf).all()
        others = np.delete(t.all_max, r, axis=0)
        assert spo.same_bits(spo.bound(others, c.kg), t.bnd[0])
    if c.zero_query is not None:
        assert t.status[c.zero_query] == 1 and t.f_i[c.zero_query].tolist() == list(range(c.k))


# ---- 3. five modelled defects --------------------------------------------------------------------------------------------
def score_pass_with_error(c):
    """The crowded case's score pass erring DOWN by tau / 2 -- inside its bound -- on the rows of the groups that hold query
    0's first ten copies in shard 1: those groups' fp32 maxima lie below the k-th merged score, and their rows (the lowest
    global rows of the tie) belong in the exact list."""
    s = c.scores.copy()
    copies = np.nonzero((c.x == c.q[0]).all(axis=1))[0]
    lo, hi = c.shard(1)
    mine = copies[(copies >= lo) & (copies < hi)][:10]
    for row in mine:
        g0 = lo + (row - lo) // spo.GROUP * spo.GROUP
        s[0, g0:g0 + spo.GROUP] -= 0.5 * c.tau
    out = s.astype(np.float32)
    assert (np.abs(out.astype(np.float64) - c.scores) <= c.tau).all()
    return out


DEFECT_CASES = [("filter_ge", "ties", None, "check_filtered"),
                ("bound_without_other_rests", "crowded-bf16", None, "check_filtered"),
                ("merge_ties_by_part", "ties", None, "check_merge"),
                ("exhaustive_without_tau", "crowded-bf16", score_pass_with_error, "check_final"),
                ("offset_int32", "ties-offset", None, "check_unfiltered")]


@pytest.mark.parametrize("defect, name, score_pass, caught_by", DEFECT_CASES, ids=[d[0] for d in DEFECT_CASES])
def test_modelled_defect_is_caught(defect, name, score_pass, caught_by):
    c = spo.build_case(name)
    spo.check_trace(c, spo.simulate(c, score_pass))                      # the sound protocol passes on the same inputs
    t = spo.simulate(c, score_pass, defect=defect)
    with pytest.raises(AssertionError):
        spo.check_trace(c, t)
    # ... by the assertion that states the broken rule, not by an accident elsewhere
    with pytest.raises(AssertionError):
        if caught_by == "check_unfiltered":
            spo.check_unfiltered(c, 1, t.ids[1], t.un_s[1], t.un_i[1])
        else:
            getattr(spo, caught_by)(c, t)


def test_defect_list_is_the_table_above():
    assert sorted(d[0] for d in DEFECT_CASES) == sorted(spo.DEFECTS)


# ---- 4. fewer rows than k ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_fewer_rows_than_k(dt):
    c = spo.build_case("tiny-k128-" + dt)
    t = spo.simulate(c)
    assert c.n == 28 < c.k
    assert (t.m_i[:, c.n:] == -1).all() and (t.m_s64[:, c.n:] == -np.inf).all() and (t.m_i[:, :c.n] >= 0).all()
    assert (t.m_s32[:, c.n:] == -np.inf).all()
    assert (t.status == 0).all() and (np.stack(t.bnd) == -np.inf).all()
    assert all(sorted(row[:c.n].tolist()) == list(range(c.n)) for row in t.m_i)
