// The kernel text of verify.hip on the host: dlc_verify_pairs at shapes either side of the register tiles (one, two and
// four cells a side per thread), their LDS chunks of 128, 64 and 32 columns and the 256 hypotheses of a pass -- dyadic
// descriptors (ties, copied patches, a NaN row, an infinite distance), points in a small range (coincident points, real
// inliers), at the
// corners of [0, 8191]^2 (the int64 bound under UBSan) and absent ones, candidate ids of -1 and N, NaN-filled padding
// columns, outputs in sentinel-filled buffers.  Every case runs twice: with every optional output and with none.  The
// results are PRINTED; tests/test_verify_host_cpu.py forms the same inputs from the same generator and compares them
// with tests/verify_oracle.py.  Built with -fsanitize=address,undefined.
#include "dlc_internal.h"
#include "verify.cpp"
typedef std::vector<double> vec;
typedef std::vector<int> ivec;
static const double QNAN = __longlong_as_double(0x7ff8000000000000ll);
static const int SENT = 0x5A5A5A5A;
static const double SENTD = __longlong_as_double(0x5A5A5A5A5A5A5A5All);

struct Lcg {                                               // the generator test_verify_host_cpu.py restates
    unsigned long long s;
    unsigned long long next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }
};

struct Case { int Q, k, N, P, H, model, tol, S, mutual, R, corners; };

int main() {
    const Case cases[] = {
        {1, 1, 1, 1, 1, 0, 0, 0, 1, 6, 0},      {2, 3, 5, 3, 7, 0, 1, 32, 1, 6, 0},    {2, 2, 4, 30, 33, 0, 3, 32, 1, 12, 0},
        {1, 2, 3, 33, 31, 1, 2, 0, 0, 8, 0},    {1, 1, 2, 64, 5, 0, 255, 0, 0, 0, 1}, {3, 2, 4, 9, 2, 1, 0, 0, 1, 4, 0},
        {12, 5, 6, 33, 66, 0, 1, 0, 0, 5, 0},    {26, 20, 7, 17, 34, 0, 2, 32, 1, 5, 0}, {1, 3, 2, 30, 65, 0, 0, 16, 0, 3, 0},
        {2, 1, 3, 8, 32, 1, 255, 0, 1, 0, 1},   {1, 2, 3, 5, 130, 0, 1, 32, 1, 6, 0},
    };
    dlc_ctx ctx{0};
    int bad = 0, ci = 0;
    for (const Case& c : cases) {
        Lcg g{(unsigned long long)(ci + 1)};
        const long long ldq = c.H + 3, ldd = c.H + 1, ldc = c.k + 2, pairs = (long long)c.Q * c.k;
        vec qd(c.Q * c.P * ldq, QNAN), dd(c.N * c.P * ldd, QNAN);
        for (int r = 0; r < c.Q * c.P; ++r) for (int h = 0; h < c.H; ++h) qd[r * ldq + h] = (double)((long long)(g.next() % 9) - 4) / 4.0;
        for (int f = 0; f < c.N; ++f) for (int j = 0; j < c.P; ++j) {
            const bool copy = g.next() % 2;
            const int src = (f % c.Q) * c.P + (j * 7 + 3) % c.P;
            for (int h = 0; h < c.H; ++h) {
                const double v = (double)((long long)(g.next() % 9) - 4) / 4.0;
                dd[(f * c.P + j) * ldd + h] = copy ? qd[src * ldq + h] : v;
            }
        }
        if (c.P >= 3) qd[1 * ldq] = QNAN;
        if (c.N * c.P >= 4) dd[2 * ldd + c.H - 1] = INFINITY;
        auto coord = [&]() -> int {
            if (c.corners) return (int)(g.next() % 2) * 8191;
            const int v = (int)(g.next() % (c.R + 2));
            return v == c.R ? -1 : v == c.R + 1 ? 8192 : v;
        };
        ivec qp(c.Q * c.P * 2), dp(c.N * c.P * 2);
        for (int& v : qp) v = coord();
        for (int& v : dp) v = coord();
        std::vector<int64_t> cand(c.Q * ldc, 99);
        for (int r = 0; r < c.Q; ++r) for (int s = 0; s < c.k; ++s) cand[r * ldc + s] = (int64_t)(g.next() % (c.N + 2)) - 1;
        cand[0] = ci % c.N;                                  // (every case has a pair that is one)
        const size_t need = dlc_verify_pairs_workspace_bytes(c.Q, c.k, c.P);
        std::vector<double> ws(need / 8 + 2);
        for (int full = 1; full >= 0; --full) {
            ivec inl(pairs + 2, SENT), nm(pairs + 2, SENT), hyp(2 * pairs + 2, SENT), match(pairs * c.P + 2, SENT);
            std::vector<uint64_t> mask(pairs + 2, 0x5A5A5A5A5A5A5A5Aull);
            vec dist(pairs * c.P * c.P + 2, SENTD);
            const int rc = dlc_verify_pairs(&ctx, qd.data(), ldq, qp.data(), c.Q, dd.data(), ldd, dp.data(), c.N, c.P, c.H, cand.data(),
                                            ldc, c.k, c.model, c.tol, c.S, c.mutual, inl.data() + 1, nm.data() + 1,
                                            full ? hyp.data() + 2 : nullptr, full ? mask.data() + 1 : nullptr,
                                            full ? match.data() + 1 : nullptr, full ? dist.data() + 1 : nullptr, ws.data(), need, nullptr);
            if (rc || !need) { ++bad; printf("BAD case %d rc=%d need=%zu %s\n", ci, rc, need, ctx.err); continue; }
            if (inl[0] != SENT || inl[pairs + 1] != SENT || nm[0] != SENT || nm[pairs + 1] != SENT) { ++bad; printf("BAD case %d frame\n", ci); }
            if (!full) {
                for (long long p = 0; p < pairs; ++p) printf("S %d %lld %d %d\n", ci, p, inl[p + 1], nm[p + 1]);
                continue;
            }
            if (hyp[0] != SENT || hyp[1] != SENT || match[0] != SENT || match[pairs * c.P + 1] != SENT ||
                mask[0] != 0x5A5A5A5A5A5A5A5Aull || mask[pairs + 1] != 0x5A5A5A5A5A5A5A5Aull ||
                memcmp(&dist[0], &SENTD, 8) || memcmp(&dist[pairs * c.P * c.P + 1], &SENTD, 8)) { ++bad; printf("BAD case %d frame\n", ci); }
            for (long long p = 0; p < pairs; ++p) {
                printf("R %d %lld %d %d %d %d %llx", ci, p, inl[p + 1], nm[p + 1], hyp[2 + 2 * p], hyp[3 + 2 * p], (unsigned long long)mask[p + 1]);
                for (int j = 0; j < c.P; ++j) printf("%c%d", j ? ',' : ' ', match[1 + p * c.P + j]);
                printf("\nD %d %lld", ci, p);
                const long long cd = cand[(p / c.k) * ldc + p % c.k];
                if (cd < 0 || cd >= c.N) {
                    bool kept = true;
                    for (int e = 0; e < c.P * c.P; ++e) kept = kept && !memcmp(&dist[1 + p * c.P * c.P + e], &SENTD, 8);
                    printf(kept ? " untouched" : " TOUCHED");
                } else {
                    for (int e = 0; e < c.P * c.P; ++e) printf("%c%llx", e ? ',' : ' ', (unsigned long long)__double_as_longlong(dist[1 + p * c.P * c.P + e]));
                }
                printf("\n");
            }
        }
        ++ci;
    }
    printf("%d cases, %d bad\n", ci, bad);
    return bad != 0;
}
