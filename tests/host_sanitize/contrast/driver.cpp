// contrast_rows.hip on the host: the kernel's own text (copied beside this file as contrast_rows.cpp, with the stand-in
// ../dlc_internal.h in front of it) run with one host thread per GPU thread, its barriers real ones, against the
// definition of include/dlc.h written as plain loops per cell, under AddressSanitizer + UBSan: every load, every store and
// every LDS index of the kernel is a checked access to a host array of exactly the caller's size.
// tests/test_contrast_host_cpu.py builds and runs it.
#include "contrast_rows.cpp"
#include <vector>
#include <algorithm>
#include <random>
#pragma clang fp contract(off)
static double ref_cell(const std::vector<double>& x, long long j, long long lim, int R) {
    long long a = j - R < 0 ? 0 : j - R, b = j + R + 1 > lim ? lim : j + R + 1, cnt = b - a;
    volatile double s = x[a];
    for (long long c = a + 1; c < b; ++c) s = s + x[c];
    volatile double mean = s / (double)cnt;
    volatile double d = x[a] - mean; volatile double q = d * d;
    for (long long c = a + 1; c < b; ++c) { volatile double e = x[c] - mean; volatile double e2 = e * e; q = q + e2; }
    volatile double sd = sqrt(q / (double)(cnt - 1));
    if (cnt < 2 || sd == 0.0) return 0.0;
    volatile double z = (x[j] - mean) / sd;
    return z;
}
template <typename T> static long long run(int dt, long long rows, long long n, long long limit0, long long step, int R, std::mt19937_64& g, int flavour) {
    const long long ld = n + 5, ldo = n + 3;
    std::vector<T> m(rows * ld + 1);
    for (auto& v : m) {
        if (dt == DLC_I64) v = (T)(flavour ? (long long)(g() % (1ull << 42)) - (1ll << 41) : (long long)(g() % 4097));
        else v = (T)(((double)(g() % 2000001) - 1e6) / 977.0);
    }
    if (flavour && dt != DLC_I64 && n > 3) { m[1 + 2] = (T)-0.0; m[1 + n / 2] = (T)INFINITY; if (rows > 1) m[1 + ld + n / 3] = (T)NAN; }
    if (n > 12) for (int i = 0; i < 2 * R + 3 && 5 + i < n; ++i) m[1 + (rows - 1) * ld + 5 + i] = (T)7;
    const unsigned long long SENT = 0x5A5A5A5A5A5A5A5Aull;
    std::vector<double> out(rows * ldo);
    for (auto& v : out) memcpy(&v, &SENT, 8);
    dlc_ctx ctx{0};
    int rc = dlc_contrast_rows(&ctx, dt, m.data() + 1, rows, n, ld, limit0, step, R, out.data(), ldo, nullptr);
    if (rc != 0) { printf("rc %d\n", rc); return 1; }
    long long bad = 0;
    for (long long r = 0; r < rows; ++r) {
        long long lim = std::clamp(limit0 + r * step, 0ll, n);          // include/dlc.h's words, not the library's dlc::row_limit
        std::vector<double> x(n);
        for (long long c = 0; c < n; ++c) x[c] = (double)m[1 + r * ld + c];
        for (long long j = 0; j < ldo; ++j) {
            unsigned long long got; memcpy(&got, &out[r * ldo + j], 8);
            if (j < lim) {
                double w = ref_cell(x, j, lim, R); unsigned long long wb; memcpy(&wb, &w, 8);
                if (!(w != w && out[r * ldo + j] != out[r * ldo + j]) && wb != got) { if (bad < 5) printf("  r=%lld j=%lld got %a want %a\n", r, j, out[r * ldo + j], w); ++bad; }
            } else if (got != SENT) { if (bad < 5) printf("  r=%lld j=%lld touched\n", r, j); ++bad; }
        }
    }
    return bad;
}
int main() {
    std::mt19937_64 g(1);
    long long shapes[][2] = {{1, 1}, {1, 2}, {5, 3}, {33, 130}, {2, 256}, {3, 513}, {2, 1100}};
    long long lims[][2] = {{1 << 30, 0}, {-4, 1}, {120, 1}, {7, 0}, {136, -2}, {0, 0}, {250, 3}};
    long long total = 0, cases = 0;
    for (auto& sh : shapes) for (auto& lm : lims) for (int R : {1, 5, 7, 16, 32}) for (int dt : {DLC_F64, DLC_F32, DLC_I64}) {
        const int fl = (int)(cases & 1);
        long long bad = dt == DLC_F64 ? run<double>(dt, sh[0], sh[1], lm[0], lm[1], R, g, fl) : dt == DLC_F32 ? run<float>(dt, sh[0], sh[1], lm[0], lm[1], R, g, fl) : run<long long>(dt, sh[0], sh[1], lm[0], lm[1], R, g, fl);
        if (bad) printf("shape %lldx%lld lim (%lld,%lld) R=%d dt=%d fl=%d: %lld bad\n", sh[0], sh[1], lm[0], lm[1], R, dt, fl, bad);
        total += bad; ++cases;
    }
    printf("contrast_rows on the host: %lld cases, %lld bad cells\n", cases, total);
    return total != 0;
}
