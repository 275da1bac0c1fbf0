"""NumPy restatement of place tracking as include/dlc.h defines it (dlc_track_rows, dlc_track_backtrace): state in, state
out, fp64 / int64, one maximum and one addition per cell in the same place, so that every comparison against the GPU is
exact.  For the call's row r, lim(r) = clamp(limit0 + r * limit_step, 0, n):

    V_r(c) = P + M[r][c]      P = the best present of: V_{r-1}(c - d), d = d_min .. d_max (lowest d first); G_{r-1} worsened
                              by jump; U_{r-1} worsened by gate; the origin 0 (first row ever only) -- the earlier among equals
    U_r    = Q + null_score   Q = the best present of: U_{r-1}; G_{r-1} worsened by gate; the origin 0
    G_r, g_r = the best present V_r(c) and the lowest column attaining it;  place_r = g_r if G_r beats U_r (or U_r is absent)

Absent is NaN (INT64_MIN for int64 rows) in V, U and G.  "Best" and the limits are sequence_oracle's."""
import numpy as np

from sequence_oracle import limits, merit_keys, same_bits   # noqa: F401  (same_bits: for the tests that import this module)

JUMP, FROM_NULL, ORIGIN, ABSENT = -1, -2, -3, -128
END_FILTERED, NO_PATH = -2, -2
I64_MIN = np.iinfo(np.int64).min


class State:
    """V [n], the rows seen, U, G (one-element arrays of V's type) and g."""

    def __init__(self, n, is_int):
        self.is_int = is_int
        self.dtype = np.int64 if is_int else np.float64
        self.mark = I64_MIN if is_int else np.nan
        self.V = np.full(n, self.mark, self.dtype)
        self.seen, self.g = 0, -1
        self.U = np.full(1, self.mark, self.dtype)
        self.G = np.full(1, self.mark, self.dtype)

    def grow(self, n):
        if n > self.V.size:
            self.V = np.concatenate([self.V, np.full(n - self.V.size, self.mark, self.dtype)])

    def present(self, a):
        return a != I64_MIN if self.is_int else ~np.isnan(a)

    def head(self):
        """The four words of the C ABI's head, as int64 bits."""
        return np.array([self.seen, self.U.view(np.int64)[0], self.G.view(np.int64)[0], self.g], dtype=np.int64)


def _worsen(v, p, lower):
    with np.errstate(over="ignore", invalid="ignore"):
        return v + p if lower else v - p


def track_rows(matrix, state, steps=(0, 2), jump=0, gate=0, null_score=np.nan, n=None, limit0=None, limit_step=0,
               lower_is_better=False):
    """The rows of matrix through the recursion, `state` updated in place.  Returns a dict: place, g [rows] int64; G, U
    [rows] (fp64 / int64, absent marked); backU [rows] int8; back [rows, n] int8; dense [rows, n]."""
    m = np.asarray(matrix)
    is_int = m.dtype == np.int64
    assert is_int == state.is_int
    if not is_int:
        m = m.astype(np.float64)                                   # fp32 -> fp64 is exact
    rows = m.shape[0]
    n = m.shape[1] if n is None else n
    m = m[:, :n]
    state.grow(n)
    assert state.V.size == n
    dt, mark, lower = state.dtype, state.mark, bool(lower_is_better)
    d_min, d_max = steps
    null_on = not np.isnan(null_score)
    jump_a, gate_a = np.full(1, jump, dt), np.full(1, gate, dt)
    null_a = np.full(1, null_score if null_on else 0, dt)
    zero = np.zeros(1, dt)
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    out = dict(place=np.full(rows, -1, np.int64), g=np.full(rows, -1, np.int64), G=np.full(rows, mark, dt), U=np.full(rows, mark, dt),
               backU=np.full(rows, ABSENT, np.int8), back=np.full((rows, n), ABSENT, np.int8), dense=np.full((rows, n), mark, dt))
    cols = np.arange(n)
    for r in range(rows):
        first = state.seen == 0
        prev = state.V if not first else np.full(n, mark, dt)
        U = state.U if not first else np.full(1, mark, dt)
        G = state.G if not first else np.full(1, mark, dt)
        hg, hu = bool(state.present(G)[0]), null_on and bool(state.present(U)[0])
        present = state.present(prev)
        rank = merit_keys(prev, lower)
        have = np.zeros(n, bool)
        b_rank = np.zeros(n, np.uint64)
        b_val = np.zeros(n, dt)
        code = np.full(n, ABSENT, np.int8)
        for d in range(d_min, d_max + 1):                          # ascending d, strict compare: the lowest d among equals
            if d >= n:
                break
            take = present[:n - d] & (~have[d:] | (rank[:n - d] > b_rank[d:]))
            np.copyto(b_rank[d:], rank[:n - d], where=take)
            np.copyto(b_val[d:], prev[:n - d], where=take)
            np.copyto(code[d:], np.int8(d), where=take)
            have[d:] |= take
        row_wide = [(hg, _worsen(G, jump_a, lower), JUMP), (hu, _worsen(U, gate_a, lower), FROM_NULL), (first, zero, ORIGIN)]
        for there, value, what in row_wide:
            if there:
                take = ~have | (merit_keys(value, lower)[0] > b_rank)
                b_rank[take], b_val[take], code[take] = merit_keys(value, lower)[0], value[0], what
                have |= take
        with np.errstate(over="ignore", invalid="ignore"):
            val = b_val + m[r]
        ok = have & (cols < lim[r]) & state.present(val)
        if not is_int:
            ok &= ~np.isnan(m[r])
        V = np.where(ok, val, mark).astype(dt)
        code = np.where(ok, code, ABSENT).astype(np.int8)
        # the no-loop state
        q_have, q_val, q_code = False, zero, ABSENT
        for there, value, what in [(hu, U, 0), (hg, _worsen(G, gate_a, lower), JUMP), (first, zero, ORIGIN)]:
            if there and (not q_have or merit_keys(value, lower)[0] > merit_keys(q_val, lower)[0]):
                q_have, q_val, q_code = True, value, what
        newU, codeU = np.full(1, mark, dt), ABSENT
        if null_on and q_have:
            with np.errstate(over="ignore", invalid="ignore"):
                u = q_val + null_a
            if state.present(u)[0]:
                newU, codeU = u, q_code
        # the row's best
        newG, g = np.full(1, mark, dt), -1
        if ok.any():
            keys = np.where(ok, merit_keys(V, lower), np.uint64(0))
            best = keys[ok].max()
            g = int(np.nonzero(ok & (keys == best))[0][0])
            newG = V[g:g + 1].copy()
        place = g if g >= 0 and (not state.present(newU)[0] or merit_keys(newG, lower)[0] > merit_keys(newU, lower)[0]) else -1
        out["place"][r], out["g"][r], out["G"][r], out["U"][r], out["backU"][r] = place, g, newG[0], newU[0], codeU
        out["back"][r], out["dense"][r] = code, V
        state.V, state.U, state.G, state.g, state.seen = V, newU, newG, g, state.seen + 1
    return out


def backtrace(back, backU, g, end, place_last=None):
    """path [rows] int64 from the state `end` of the last row (a column, -1 or END_FILTERED = place_last) back to row 0;
    NO_PATH from a row whose state is absent on."""
    rows, n = back.shape
    path = np.full(rows, NO_PATH, np.int64)
    s = int(place_last) if end == END_FILTERED else int(end)
    if s < -1 or s >= n:
        return path
    for r in range(rows - 1, -1, -1):
        code = int(back[r, s]) if s >= 0 else int(backU[r])
        if code == ABSENT:
            break
        path[r] = s
        if code == ORIGIN:
            if r > 0:
                break
        elif code == JUMP:
            s = int(g[r - 1]) if r > 0 else -1
        elif code == FROM_NULL:
            s = -1 if s >= 0 else -2
        elif code >= 0:
            s = s - code if s >= 0 else (-1 if code == 0 else -2)
        else:
            s = -2
        if r > 0 and (s < -1 or s >= n):
            break
    return path


def track_places(matrix, steps=(0, 2), jump=0, gate=0, null_score=np.nan, lower_is_better=False, n=None, limit0=None, limit_step=0):
    """(place, path, G, U) of the whole matrix from a fresh state: the filtered place per frame and the labelling traced
    back from the last row's filtered place."""
    m = np.asarray(matrix)
    o = track_rows(m, State(m.shape[1] if n is None else n, m.dtype == np.int64), steps, jump, gate, null_score, n, limit0, limit_step,
                   lower_is_better)
    return o["place"], backtrace(o["back"], o["backU"], o["g"], END_FILTERED, o["place"][-1]), o["G"], o["U"]


def planted_traversal(seed):
    """(matrix [120, 100], truth [120]): N(0, 1) rounded to multiples of 2^-6; frames 40-79 and 100-119 revisit key-frames,
    stepping 0-2 key-frames per frame, +4.0 on the true cell; truth is -1 elsewhere."""
    rng = np.random.RandomState(seed)
    m = np.round(rng.standard_normal((120, 100)) * 64) / 64
    truth = np.full(120, -1, np.int64)
    for lo, hi, start in ((40, 80, 5), (100, 120, 30)):
        c = start
        for f in range(lo, hi):
            if f > lo:
                c += int(rng.randint(0, 3))
            truth[f] = c
            m[f, c] += 4.0
    return m, truth
