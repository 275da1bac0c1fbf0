"""The kernel text of csrc/verify.hip on the host (no GPU): compiled as C++ against the stand-in of tests/host_sanitize/
-- one host thread per GPU thread, barriers emulated -- and run as a stand-alone program under AddressSanitizer + UBSan:
the signed-overflow and out-of-bounds check of the integer geometry and the LDS indexing.  The program prints what
dlc_verify_pairs wrote; the same inputs are formed here from the same generator and every printed number is compared
with tests/verify_oracle.py -- integers with ==, the distance tables by their bits."""
import numpy as np

import host_kernel
import verify_oracle as vfo

# (Q, k, N, P, H, model, tol, S, mutual, R, corners): tests/host_sanitize/verify/driver.cpp's table
CASES = [
    (1, 1, 1, 1, 1, 0, 0, 0, 1, 6, 0), (2, 3, 5, 3, 7, 0, 1, 32, 1, 6, 0), (2, 2, 4, 30, 33, 0, 3, 32, 1, 12, 0),
    (1, 2, 3, 33, 31, 1, 2, 0, 0, 8, 0), (1, 1, 2, 64, 5, 0, 255, 0, 0, 0, 1), (3, 2, 4, 9, 2, 1, 0, 0, 1, 4, 0),
    (12, 5, 6, 33, 66, 0, 1, 0, 0, 5, 0), (26, 20, 7, 17, 34, 0, 2, 32, 1, 5, 0), (1, 3, 2, 30, 65, 0, 0, 16, 0, 3, 0),
    (2, 1, 3, 8, 32, 1, 255, 0, 1, 0, 1), (1, 2, 3, 5, 130, 0, 1, 32, 1, 6, 0),
]


class Lcg:
    def __init__(self, seed):
        self.s = seed

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self.s >> 33


def inputs(ci, case):
    """The driver's inputs of case ci: (q_desc [Q, P, H], q_pts, db_desc [N, P, H], db_pts, cand [Q, k])."""
    Q, k, N, P, H, _, _, _, _, R, corners = case
    g = Lcg(ci + 1)
    qd = np.array([(g.next() % 9 - 4) / 4.0 for _ in range(Q * P * H)]).reshape(Q * P, H)
    dd = np.empty((N * P, H))
    for f in range(N):
        for j in range(P):
            copy = g.next() % 2
            src = (f % Q) * P + (j * 7 + 3) % P
            v = [(g.next() % 9 - 4) / 4.0 for _ in range(H)]
            dd[f * P + j] = qd[src] if copy else v
    if P >= 3:
        qd[1, 0] = np.nan
    if N * P >= 4:
        dd[2, H - 1] = np.inf

    def coord():
        if corners:
            return (g.next() % 2) * 8191
        v = g.next() % (R + 2)
        return -1 if v == R else 8192 if v == R + 1 else v
    qp = np.array([coord() for _ in range(Q * P * 2)], dtype=np.int64).reshape(Q, P, 2)
    dp = np.array([coord() for _ in range(N * P * 2)], dtype=np.int64).reshape(N, P, 2)
    cand = np.array([g.next() % (N + 2) - 1 for _ in range(Q * k)], dtype=np.int64).reshape(Q, k)
    cand[0, 0] = ci % N
    return qd.reshape(Q, P, H), qp, dd.reshape(N, P, H), dp, cand


def test_verify_kernel_text_on_the_host_under_sanitizers(tmp_path):
    res = host_kernel.run(tmp_path, "verify", "verify")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "%d cases, 0 bad" % len(CASES) in res.stdout
    got = {"R": {}, "D": {}, "S": {}}
    for line in res.stdout.splitlines():
        f = line.split(" ")
        if f[0] in got:
            got[f[0]][(int(f[1]), int(f[2]))] = f[3:]
    peak = vfo.Peak()
    for ci, case in enumerate(CASES):
        Q, k, N, P, H, model, tol, S, mutual = case[:9]
        qd, qp, dd, dp, cand = inputs(ci, case)
        want = vfo.verify_pairs(qd, qp, dd, dp, cand, model=model, tol=tol, S=S, mutual=mutual, peak=peak)
        for r in range(Q):
            for s in range(k):
                w, key = want[r][s], (ci, r * k + s)
                line = [str(w["inliers"]), str(w["n_matches"]), str(w["hyp"][0]), str(w["hyp"][1]), "%x" % w["mask"],
                        ",".join(str(int(v)) for v in w["match"])]
                assert got["R"][key] == line, (key, got["R"][key], line)
                assert got["S"][key] == line[:2], key
                if w["dist"] is None:
                    assert got["D"][key] == ["untouched"], key
                else:
                    bits = np.ascontiguousarray(w["dist"]).view(np.uint64).reshape(-1)
                    have = np.array([int(v, 16) for v in got["D"][key][0].split(",")], dtype=np.uint64)
                    nan = np.isnan(w["dist"]).reshape(-1)                  # (a NaN's payload is not part of the definition)
                    assert np.array_equal(have[~nan], bits[~nan]) and np.isnan(have.view(np.float64)[nan]).all(), key
    assert sum(len(v) for v in got.values()) == 3 * sum(c[0] * c[1] for c in CASES)
    # the corner cases with tol = 255 drove the integers as far as the definition lets them go: well inside int64
    assert 1 << 50 < peak.value < 1 << 57
