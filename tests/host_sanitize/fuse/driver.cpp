// dlc_fuse_rows' kernel text on the host: every plan and norm at shapes either side of the lane, chunk and slab
// boundaries, mixed dtypes, sources one element off their 16-byte alignment, row limits that end inside a lane's four
// cells -- against a recursive TREE and per-cell loops over the definition of include/dlc.h, bit for bit, untouched words
// against a sentinel.  Built with -fsanitize=address,undefined (tests/test_fuse_host_cpu.py).
#include "dlc_internal.h"
#include "fuse_rows.cpp"
#include <algorithm>
#include <random>
static double tree(const std::vector<double>& v, size_t lo, size_t len) {
    if (len == 1) return lo < v.size() ? v[lo] : -0.0;
    return tree(v, lo, len / 2) + tree(v, lo + len / 2, len / 2);
}
static double TREE(const std::vector<double>& v) { size_t P = 1; while (P < v.size()) P <<= 1; return tree(v, 0, P); }
#pragma clang fp contract(off)
int main() {
    std::mt19937_64 rng(7);
    std::normal_distribution<double> g(0, 1);
    int bad = 0, cases = 0;
    const long long shapes[][2] = {{1,1},{3,2},{3,65},{2,257},{2,4097},{1,8193}};
    for (auto& sh : shapes) for (int m : {1, 3}) for (int norm = 0; norm < 3; ++norm) {
        const long long rows = sh[0], n = sh[1];
        std::vector<std::vector<double>> f64(m); std::vector<std::vector<float>> f32(m); std::vector<std::vector<long long>> i64(m);
        int dt[8], lib[8]; const void* src[8]; long long ld[8]; double w[8];
        for (int i = 0; i < m; ++i) {
            dt[i] = i % 3 == 0 ? DLC_F64 : (i % 3 == 1 ? DLC_F32 : DLC_I64); lib[i] = i & 1; ld[i] = n + 3 + i; w[i] = i == 1 ? -0.75 : 1.0 + i;
            f64[i].assign(rows * ld[i] + 1, 1e300); f32[i].assign(rows * ld[i] + 1, 1e30f); i64[i].assign(rows * ld[i] + 1, 1ll << 62);
            for (auto& x : f64[i]) x = g(rng) * 3 + 1; for (auto& x : f32[i]) x = (float)g(rng); for (auto& x : i64[i]) x = (long long)(g(rng) * 1e17);
            // odd alignment: start one element in
            src[i] = dt[i] == DLC_F64 ? (const void*)(f64[i].data() + (i & 1)) : dt[i] == DLC_F32 ? (const void*)(f32[i].data() + 1) : (const void*)(i64[i].data() + 1);
        }
        const long long limit0 = n - 2, step = 1, ldo = n + 1;
        std::vector<double> ref(rows * ldo, -7.0);
        for (long long r = 0; r < rows; ++r) {
            long long c = std::clamp(limit0 + r * step, 0ll, n);        // include/dlc.h's words, not the library's dlc::row_limit
            if (!c) continue;
            for (int i = 0; i < m; ++i) {
                std::vector<double> x(c);
                for (long long j = 0; j < c; ++j) {
                    if (dt[i] == DLC_F64) x[j] = ((const double*)src[i])[r * ld[i] + j];
                    else if (dt[i] == DLC_F32) x[j] = ((const float*)src[i])[r * ld[i] + j];
                    else x[j] = (double)((const long long*)src[i])[r * ld[i] + j];
                }
                std::vector<double> u(c);
                if (norm == 0) for (long long j = 0; j < c; ++j) u[j] = lib[i] ? -x[j] : x[j];
                else if (norm == 1) {
                    double mean = TREE(x) / (double)c; std::vector<double> d2(c);
                    for (long long j = 0; j < c; ++j) { double d = x[j] - mean; d2[j] = d * d; }
                    double sd = sqrt(TREE(d2) / (double)(c - 1));
                    for (long long j = 0; j < c; ++j) u[j] = (c < 2 || sd == 0.0) ? 0.0 : (lib[i] ? (mean - x[j]) / sd : (x[j] - mean) / sd);
                } else {
                    double lo = x[0], hi = x[0];
                    for (double v : x) { if (v < lo) lo = v; if (v > hi) hi = v; }
                    double range = hi - lo;
                    for (long long j = 0; j < c; ++j) u[j] = range == 0.0 ? 0.0 : (lib[i] ? (hi - x[j]) / range : (x[j] - lo) / range);
                }
                for (long long j = 0; j < c; ++j) { double t = w[i] * u[j]; ref[r * ldo + j] = i == 0 ? t : ref[r * ldo + j] + t; }
            }
        }
        dlc_ctx ctx{0};
        size_t need = dlc_fuse_rows_workspace_bytes(rows, n, m);
        std::vector<double> ws(need / 8 + 2);
        for (int plan = 1; plan <= 2; ++plan) {
            std::vector<double> out(rows * ldo, -7.0);
            int64_t ld64[8]; for (int i = 0; i < m; ++i) ld64[i] = ld[i];
            int rc = dlc_fuse_rows(&ctx, m, dt, src, ld64, w, lib, rows, n, limit0, step, norm, plan, out.data(), ldo, ws.data(), need, nullptr);
            ++cases;
            if (rc != 0 || memcmp(out.data(), ref.data(), out.size() * 8)) {
                ++bad; long long first = -1; for (size_t q = 0; q < out.size(); ++q) if (memcmp(&out[q], &ref[q], 8)) { first = q; break; }
                printf("MISMATCH rows=%lld n=%lld m=%d norm=%d plan=%d rc=%d first=%lld (%a vs %a)\n", rows, n, m, norm, plan, rc, first, first >= 0 ? out[first] : 0, first >= 0 ? ref[first] : 0);
            }
        }
    }
    printf("%d cases, %d bad\n", cases, bad);
    return bad != 0;
}
