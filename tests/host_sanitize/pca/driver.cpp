// The kernel text of pca.hip on the host: dlc_pca_project under both plans (and AUTO), both basis dtypes and every
// combination of NULL / given mean and scale, at shapes either side of the row tiles (2, 8), the column tiles (256, 512),
// the LDS slab of 128 columns, the 8 basis rows in flight and the chunk of 1024 -- NaN-filled padding columns on x and
// the basis, outputs in sentinel-filled buffers wider than M -- against per-element loops over the definition of
// include/dlc.h, bit for bit; and the refusals, which write nothing.  Built with -fsanitize=address,undefined
// (tests/test_pca_host_cpu.py).
#include "dlc_internal.h"
#include "pca.cpp"
#include <random>
#pragma clang fp contract(off)
typedef std::vector<double> vec;
static const double QNAN = __longlong_as_double(0x7ff8000000000000ll);

static bool same(const void* a, const void* b, size_t bytes, const char* what, int& bad) {
    if (!memcmp(a, b, bytes)) return true;
    size_t at = 0; while (((const char*)a)[at] == ((const char*)b)[at]) ++at;
    printf("MISMATCH %s at byte %zu\n", what, at); ++bad; return false;
}

int main() {
    std::mt19937_64 rng(31);
    std::normal_distribution<double> g(0, 1);
    int bad = 0, cases = 0;
    dlc_ctx ctx{0};
    // {rows, D, M}
    const long long shapes[][3] = {{1, 1, 1}, {3, 7, 2}, {2, 1025, 65}, {9, 1030, 257}, {17, 135, 300}, {5, 2049, 3}, {1, 1024, 513}};
    for (auto& e : shapes) {
        const long long rows = e[0], D = e[1], ldx = D + 3, ldo = e[2] + 2;
        const int M = (int)e[2];
        const long long ldb = M + 1, chunks = (D + DLC_PCA_CHUNK - 1) / DLC_PCA_CHUNK;
        vec x(rows * ldx, QNAN), mean(D), scale(M), b64(D * ldb, QNAN);
        std::vector<float> b32(D * ldb, NAN);
        for (long long r = 0; r < rows; ++r) for (long long d = 0; d < D; ++d) x[r * ldx + d] = g(rng);
        for (long long d = 0; d < D; ++d) mean[d] = g(rng);
        for (int c = 0; c < M; ++c) scale[c] = 0.5 + (double)(rng() % 100) / 64.0;
        for (long long d = 0; d < D; ++d) for (int c = 0; c < M; ++c) { b64[d * ldb + c] = g(rng); b32[d * ldb + c] = (float)g(rng); }
        if (D >= 7) { x[3] = INFINITY; mean[3] = 1.0; x[5] = -0.0; mean[5] = 0.0; }
        if (rows >= 3 && D >= 7) x[2 * ldx + 6] = QNAN;
        for (int dt = 0; dt < 2; ++dt) for (int ms = 0; ms < 4; ++ms) {
            const double* mp = ms & 1 ? mean.data() : nullptr;
            const double* sp = ms & 2 ? scale.data() : nullptr;
            vec ref(rows * ldo, -7.0);
            for (long long r = 0; r < rows; ++r) for (int c = 0; c < M; ++c) {
                double y = 0.0;
                for (long long j = 0; j < chunks; ++j) {
                    double s = 0.0;
                    for (long long d = j * DLC_PCA_CHUNK; d < D && d < (j + 1) * DLC_PCA_CHUNK; ++d) {
                        const double bd = dt ? (double)b32[d * ldb + c] : b64[d * ldb + c];
                        const double t = mp ? x[r * ldx + d] - mp[d] : x[r * ldx + d];
                        const double q = t * bd;
                        s = s + q;
                    }
                    y = j == 0 ? s : y + s;
                }
                ref[r * ldo + c] = sp ? y * sp[c] : y;
            }
            for (int plan = 0; plan < 3; ++plan) {
                const size_t need = dlc_pca_project_workspace_bytes(rows, D, M, plan);
                std::vector<double> ws(need / 8 + 2);
                vec out(rows * ldo, -7.0);
                const int rc = dlc_pca_project(&ctx, x.data(), rows, D, ldx, mp, dt ? DLC_F32 : DLC_F64, dt ? (const void*)b32.data() : (const void*)b64.data(),
                                               M, ldb, sp, out.data(), ldo, plan, need ? ws.data() : nullptr, need, nullptr);
                ++cases;
                if (rc || (plan == DLC_PCA_PLAN_SPLIT && need < (size_t)(rows * chunks * M * 8))) { ++bad; printf("project rc=%d need=%zu\n", rc, need); }
                char what[112];
                snprintf(what, sizeof(what), "rows=%lld D=%lld M=%d f32=%d mean=%d scale=%d plan=%d", rows, D, M, dt, ms & 1, ms >> 1, plan);
                // NaN results: the payload is the machine's; compare them as NaN, everything else by its bits
                for (size_t i = 0; i < out.size(); ++i) if (out[i] != out[i] && ref[i] != ref[i]) out[i] = ref[i];
                same(out.data(), ref.data(), out.size() * 8, what, bad);
            }
        }
    }
    {   // refusals write nothing: SPLIT above its row limit, a short pitch, out on top of x, a workspace that is too small
        const long long rows = 65, D = 9; const int M = 2;
        vec x(rows * D, 1.0), b(D * M, 1.0), out(rows * M, -7.0), keep(rows * M, -7.0), ws(rows * M + 2);
        const int r1 = dlc_pca_project(&ctx, x.data(), rows, D, D, nullptr, DLC_F64, b.data(), M, M, nullptr, out.data(), M, DLC_PCA_PLAN_SPLIT, ws.data(), ws.size() * 8, nullptr);
        const int r2 = dlc_pca_project(&ctx, x.data(), rows, D, D - 1, nullptr, DLC_F64, b.data(), M, M, nullptr, out.data(), M, DLC_PCA_PLAN_ONE_PASS, nullptr, 0, nullptr);
        const int r3 = dlc_pca_project(&ctx, x.data(), 2, D, D, nullptr, DLC_F64, b.data(), M, M, nullptr, x.data() + 1, M, DLC_PCA_PLAN_ONE_PASS, nullptr, 0, nullptr);
        const int r4 = dlc_pca_project(&ctx, x.data(), 2, D, D, nullptr, DLC_F64, b.data(), M, M, nullptr, out.data(), M, DLC_PCA_PLAN_SPLIT, ws.data(), 8, nullptr);
        cases += 4;
        if (r1 != DLC_ERR_BAD_SHAPE || r2 != DLC_ERR_BAD_ARG || r3 != DLC_ERR_BAD_ARG || r4 != DLC_ERR_WORKSPACE) { ++bad; printf("refusals %d %d %d %d\n", r1, r2, r3, r4); }
        if (dlc_pca_project_workspace_bytes(rows, D, M, DLC_PCA_PLAN_SPLIT) != 0) { ++bad; printf("workspace of a refused shape\n"); }
        same(out.data(), keep.data(), out.size() * 8, "refused calls wrote", bad);
    }
    printf("%d cases, %d bad\n", cases, bad);
    return bad != 0;
}
