// The kernel text of vlad.hip on the host: dlc_vlad_assign, dlc_vlad_encode (both norms) and dlc_kmeans_step at shapes
// either side of the register tiles, the LDS chunk of 32 columns, the accumulator tile widths, the tree block of 2048
// leaves and the k-means block of 1024 rows -- on a dyadic grid (ties, duplicated centres, an all-NaN row) and on
// Gaussian operands, NaN-filled padding columns, outputs in sentinel-filled buffers -- against per-element loops over the
// definition of include/dlc.h and a recursive TREE, bit for bit.  Built with -fsanitize=address,undefined
// (tests/test_vlad_host_cpu.py).
#include "dlc_internal.h"
#include "vlad.cpp"
#include <random>
#pragma clang fp contract(off)
typedef std::vector<double> vec;
static double tree(const vec& v, size_t lo, size_t len) {
    if (len == 1) return lo < v.size() ? v[lo] : -0.0;
    return tree(v, lo, len / 2) + tree(v, lo + len / 2, len / 2);
}
static double TREE(const vec& v) { size_t P = 1; while (P < v.size()) P <<= 1; return tree(v, 0, P); }
static const double QNAN = __longlong_as_double(0x7ff8000000000000ll);

struct Problem {
    long long rows, H, ldx, ldc; int K;
    vec x, c;                                            // with NaN padding columns
    double X(long long n, long long h) const { return x[n * ldx + h]; }
    double C(int k, long long h) const { return c[k * ldc + h]; }
};
static Problem make(long long rows, long long H, int K, bool dyadic, std::mt19937_64& rng) {
    Problem p{rows, H, H + 3, H + 1, K, {}, {}};
    p.x.assign(rows * p.ldx, QNAN); p.c.assign(K * p.ldc, QNAN);
    std::normal_distribution<double> g(0, 1);
    auto val = [&] { return dyadic ? (double)((long long)(rng() % 9) - 4) / 8.0 : g(rng); };
    for (long long n = 0; n < rows; ++n) for (long long h = 0; h < H; ++h) p.x[n * p.ldx + h] = val();
    for (int k = 0; k < K; ++k) for (long long h = 0; h < H; ++h) p.c[k * p.ldc + h] = val();
    if (K >= 3) for (long long h = 0; h < H; ++h) p.c[(K - 1) * p.ldc + h] = p.c[h];      // a copy of word 0 at the top
    if (rows >= 4) p.x[2 * p.ldx] = QNAN;                                                  // an all-NaN row
    if (rows >= 6 && K >= 2) p.c[1 * p.ldc + H - 1] = INFINITY;                            // a word at infinite distance
    return p;
}
static void ref_assign(const Problem& p, std::vector<int>& a, vec& dist) {
    a.assign(p.rows, -1); dist.assign(p.rows, QNAN);
    for (long long n = 0; n < p.rows; ++n)
        for (int k = 0; k < p.K; ++k) {
            double d = 0.0;
            for (long long h = 0; h < p.H; ++h) { double t = p.X(n, h) - p.C(k, h); double q = t * t; d = d + q; }
            if (d != d) continue;
            if (a[n] < 0 || d < dist[n]) { a[n] = k; dist[n] = d; }
        }
}
static bool same(const void* a, const void* b, size_t bytes, const char* what, int& bad) {
    if (!memcmp(a, b, bytes)) return true;
    size_t at = 0; while (((const char*)a)[at] == ((const char*)b)[at]) ++at;
    printf("MISMATCH %s at byte %zu\n", what, at); ++bad; return false;
}

int main() {
    std::mt19937_64 rng(11);
    int bad = 0, cases = 0;
    dlc_ctx ctx{0};
    // ---- assign + encode: {frames, P, H, K, dyadic grid?, norms (bit 0: NONE, bit 1: INTRA)}; a workgroup costs the host
    // 256 threads, INTRA takes one per (frame, word): the many-word shapes run one norm
    const long long enc[][6] = {{1, 1, 1, 1, 0, 3}, {1, 1, 1, 1, 1, 3}, {3, 5, 7, 2, 0, 3}, {3, 5, 7, 2, 1, 3}, {2, 30, 33, 16, 1, 3},
                                {2, 30, 32, 17, 0, 3}, {1, 5, 65, 33, 1, 3}, {1, 30, 40, 64, 0, 2}, {1, 7, 9, 256, 1, 1},
                                {1, 2, 2049, 1, 0, 3}, {9, 9, 1, 3, 1, 3}, {1, 30, 300, 130, 0, 1}};
    for (auto& e : enc) {
        const int dyadic = (int)e[4];
        const long long frames = e[0], H = e[2]; const int P = (int)e[1], K = (int)e[3];
        const Problem p = make(frames * P, H, K, dyadic, rng);
        std::vector<int> a; vec dist; ref_assign(p, a, dist);
        {   // dlc_vlad_assign
            std::vector<int> oa(p.rows + 2, -77); vec od(p.rows + 2, -7.0);
            const int rc = dlc_vlad_assign(&ctx, p.x.data(), p.rows, H, p.ldx, p.c.data(), K, p.ldc, oa.data() + 1, od.data() + 1, nullptr);
            std::vector<int> ea(p.rows + 2, -77); vec ed(p.rows + 2, -7.0);
            memcpy(ea.data() + 1, a.data(), p.rows * 4); memcpy(ed.data() + 1, dist.data(), p.rows * 8);
            ++cases; if (rc) { ++bad; printf("assign rc=%d\n", rc); }
            same(oa.data(), ea.data(), oa.size() * 4, "assign", bad); same(od.data(), ed.data(), od.size() * 8, "assign dist", bad);
        }
        for (int norm = 0; norm < 2; ++norm) {
            if (!(e[5] >> norm & 1)) continue;
            const long long KH = (long long)K * H, ldo = KH + 2;
            vec ref(frames * ldo, -7.0);
            for (long long f = 0; f < frames; ++f) for (int k = 0; k < K; ++k) {
                vec R(H, 0.0); bool seen = false;
                for (int q = 0; q < P; ++q) {
                    const long long n = f * P + q;
                    if (a[n] != k) continue;
                    for (long long h = 0; h < H; ++h) { double r = p.X(n, h) - p.C(k, h); R[h] = seen ? R[h] + r : r; }
                    seen = true;
                }
                if (norm == DLC_VLAD_NORM_INTRA) {
                    vec sq(H); for (long long h = 0; h < H; ++h) sq[h] = R[h] * R[h];
                    const double nk = sqrt(TREE(sq));
                    for (long long h = 0; h < H; ++h) R[h] = nk == 0.0 ? 0.0 : R[h] / nk;
                }
                for (long long h = 0; h < H; ++h) ref[f * ldo + k * H + h] = R[h];
            }
            const size_t need = dlc_vlad_encode_workspace_bytes(frames, P, H, K);
            std::vector<double> ws(need / 8 + 2); vec out(frames * ldo, -7.0); std::vector<int> oa(p.rows, -77);
            const int rc = dlc_vlad_encode(&ctx, p.x.data(), frames, P, H, p.ldx, p.c.data(), K, p.ldc, norm, out.data(), ldo,
                                           norm ? oa.data() : nullptr, ws.data(), need, nullptr);
            ++cases; if (rc || !need) { ++bad; printf("encode rc=%d need=%zu\n", rc, need); }
            char what[96]; snprintf(what, sizeof(what), "encode frames=%lld P=%d H=%lld K=%d norm=%d dyadic=%d", frames, P, H, K, norm, dyadic);
            same(out.data(), ref.data(), out.size() * 8, what, bad);
            if (norm) same(oa.data(), a.data(), oa.size() * 4, "encode out_assign", bad);
        }
    }
    // ---- k-means step: {rows, H, K, dyadic grid?, prev_assign given?}
    const long long km[][5] = {{1, 3, 2, 0, 0}, {1023, 5, 3, 1, 1}, {1024, 2, 2, 0, 1}, {1025, 5, 3, 0, 0}, {2100, 3, 17, 1, 1},
                               {300, 40, 256, 0, 1}};
    for (auto& e : km) {
        const int dyadic = (int)e[3], with_prev = (int)e[4];
        const long long rows = e[0], H = e[1]; const int K = (int)e[2];
        const Problem p = make(rows, H, K, dyadic, rng);
        std::vector<int> a; vec dist; ref_assign(p, a, dist);
        std::vector<int> prev(rows); for (long long n = 0; n < rows; ++n) prev[n] = n % 3 ? a[n] : (int)(rng() % K);
        const long long nb = (rows + DLC_KMEANS_BLOCK - 1) / DLC_KMEANS_BLOCK, ldo = H + 2;
        vec cref(K * ldo, -7.0), inert(nb, 0.0); std::vector<long long> cnt(K, 0);
        long long changed = 0;
        for (long long n = 0; n < rows; ++n) {
            changed += with_prev ? prev[n] != a[n] : 1;
            if (a[n] >= 0) { inert[n / DLC_KMEANS_BLOCK] = inert[n / DLC_KMEANS_BLOCK] + dist[n]; ++cnt[a[n]]; }
        }
        for (int k = 0; k < K; ++k) for (long long h = 0; h < H; ++h) {
            vec S(nb, -0.0);
            for (long long n = 0; n < rows; ++n) if (a[n] == k) S[n / DLC_KMEANS_BLOCK] = S[n / DLC_KMEANS_BLOCK] + p.X(n, h);
            cref[k * ldo + h] = cnt[k] > 0 ? TREE(S) / (double)cnt[k] : p.C(k, h);
        }
        const double iref = TREE(inert);
        const size_t need = dlc_kmeans_step_workspace_bytes(rows, H, K);
        std::vector<double> ws(need / 8 + 2); vec cout_(K * ldo, -7.0); std::vector<int> oa(rows, -77);
        std::vector<int64_t> ocnt(K, -5); double oin = -7.0; int64_t och = -5;
        const int rc = dlc_kmeans_step(&ctx, p.x.data(), rows, H, p.ldx, p.c.data(), K, p.ldc, cout_.data(), ldo,
                                       with_prev ? prev.data() : nullptr, oa.data(), ocnt.data(), &oin, &och, ws.data(), need, nullptr);
        ++cases; if (rc || !need) { ++bad; printf("kmeans rc=%d need=%zu\n", rc, need); }
        char what[96]; snprintf(what, sizeof(what), "kmeans rows=%lld H=%lld K=%d dyadic=%d", rows, H, K, dyadic);
        same(cout_.data(), cref.data(), cout_.size() * 8, what, bad);
        same(oa.data(), a.data(), rows * 4, "kmeans assign", bad);
        same(ocnt.data(), cnt.data(), K * 8, "kmeans counts", bad);
        same(&oin, &iref, 8, "kmeans inertia", bad);
        if (och != changed) { ++bad; printf("MISMATCH changed %lld vs %lld\n", (long long)och, changed); }
    }
    printf("%d cases, %d bad\n", cases, bad);
    return bad != 0;
}
