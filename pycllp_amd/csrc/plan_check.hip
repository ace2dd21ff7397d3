// plan_check.hip -- a program of its own (make plan_check; not part of the library): every plan kind of wreg_plan.h, big_plan.h and
// block_plan.h built over a seeded set of matrices, and the invariants of the LDS layout checked on each.  It makes no HIP call
// and needs no GPU; it is meant for a host sanitizer:
//     make plan_check EXTRA="-Xarch_host -fsanitize=address,undefined" && ./plan_check
#include "wreg_plan.h"
#include "big_plan.h"
#include "block_plan.h"
#include <random>

namespace {

struct Csr { int m, n; std::vector<double> val; std::vector<int> ptr, col; };

// m x n with `density` of the columns in front of an identity tail (tail: the last m columns) filled
Csr random_csr(int m, int n, double density, bool tail, unsigned seed) {
    std::mt19937 g(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    Csr A{m, n, {}, {0}, {}};
    const int nd = tail && n > m ? n - m : n;
    for (int i = 0; i < m; i++) {
        for (int j = 0; j < nd; j++)
            if (u(g) < density) { A.col.push_back(j); A.val.push_back((0.05 + 0.95 * u(g)) * (u(g) < 0.5 ? -1.0 : 1.0)); }
        if (nd < n) { A.col.push_back(nd + i); A.val.push_back(1.0); }
        A.ptr.push_back((int)A.col.size());
    }
    return A;
}

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Span { long lo, hi; const char* name; };

void check_wave(const WregHostPlan& P, int max_lds, const char* what) {
    const WregTab& T = P.tab;
    const long nnz = T.nnz, ell = 64L * std::max(T.ctot, 1), terms = std::max(T.n_term, 1), mpl = 64 * ((16 * P.mb + 63) / 64);
    std::vector<Span> s = { {T.o_wave, T.o_wave + 8L * T.wpb * T.wave_doubles, "wave"} };
    if (P.da && !P.pa) s.push_back({T.o_img, T.o_img + 8L * T.img_rows * T.as, "img"});
    if (!P.da) {
        s.insert(s.end(), { {T.o_lev, T.o_lev + 4L * (T.n_lev + 1), "lev"}, {T.o_t_cd, T.o_t_cd + 4 * terms, "t_cd"},
                            {T.o_colmap, T.o_colmap + 4L * 64 * P.nq, "colmap"}, {T.o_meta, T.o_meta + 4L * META_N, "meta"},
                            {T.o_csr_col, T.o_csr_col + 2 * nnz, "csr_col"}, {T.o_csr_ptr, T.o_csr_ptr + 2 * mpl, "csr_ptr"},
                            {T.o_csr_len, T.o_csr_len + 2 * mpl, "csr_len"}, {T.o_ec_row, T.o_ec_row + 2 * ell, "ec_row"} });
        if (P.pa) s.insert(s.end(), { {T.o_t_ab, T.o_t_ab + 4 * terms, "t_ab"}, {T.o_ec_src, T.o_ec_src + 2 * ell, "ec_src"} });
        else s.insert(s.end(), { {T.o_csr_val, T.o_csr_val + 8 * nnz, "csr_val"}, {T.o_ec_val, T.o_ec_val + 8 * ell, "ec_val"},
                                 {T.o_t_w, T.o_t_w + 8 * terms, "t_w"} });
    }
    std::sort(s.begin(), s.end(), [](const Span& a, const Span& b) { return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi; });
    for (size_t i = 0; i < s.size(); i++) {
        CHECK(s[i].lo % 16 == 0 && s[i].lo >= 0 && s[i].hi <= T.lds_bytes, "%s: %s [%ld, %ld) of %d", what, s[i].name, s[i].lo, s[i].hi, T.lds_bytes);
        if (i && s[i].hi > s[i].lo) CHECK(s[i - 1].hi <= s[i].lo, "%s: %s overlaps %s", what, s[i - 1].name, s[i].name);
    }
    CHECK(T.wpb >= 1 && T.wpb <= 4 && T.lds_bytes <= max_lds, "%s: wpb %d, lds %d", what, T.wpb, T.lds_bytes);
    CHECK(16 * P.mb >= T.m && 64 * P.nq >= T.n, "%s: (%d, %d) does not cover", what, P.mb, P.nq);
    if (!P.da) {
        // 16-bit packed indices: columns' positions, destinations inside the stage and the W area, CSR sources
        const char* b = P.blob.bytes.data();
        const unsigned* t_cd = (const unsigned*)(b + P.a_t_cd);
        const unsigned* t_ab = (const unsigned*)(b + P.a_t_ab);
        for (long t = 0; t < T.n_term; t++) {
            CHECK((int)(t_cd[t] & 0xffff) < 64 * P.nq && (int)(t_cd[t] >> 16) < stage_d(P.nq) + P.mb * WL, "%s: t_cd[%ld]", what, t);
            CHECK((long)(t_ab[t] & 0xffff) <= nnz && (long)(t_ab[t] >> 16) <= nnz, "%s: t_ab[%ld]", what, t);
        }
        const unsigned* colmap = (const unsigned*)(b + P.a_colmap);
        for (int p = 0; p < 64 * P.nq; p++) CHECK(p < T.n ? colmap[p] < 8u * T.n : colmap[p] == PAD_OFF, "%s: colmap[%d]", what, p);
    }
}

void check_blob(const PlanBlob& b, const char* what) {
    size_t end = 0;
    for (const PlanBlob::Section& s : b.sec) {
        CHECK(s.off % 16 == 0 && s.off >= end && s.off + s.count * s.elem <= b.bytes.size(), "%s: blob section at %zu", what, s.off);
        end = s.off + s.count * s.elem;
    }
}

int plans = 0;

void every_kind(const Csr& A, const char* name) {
    const int max_lds = 160 * 1024;
    char what[128];
    long long s[PLAN_NSCALARS];
    for (int kind = WPLAN_SHARED; kind <= WPLAN_BOUNDED_DENSE_PA; kind++) {
        WregHostPlan P;
        snprintf(what, sizeof(what), "%s wave kind %d", name, kind);
        if (wreg_host_plan((WregPlanKind)kind, wreg_listed_shapes, A.m, A.n, (int)A.val.size(), A.val.data(), A.ptr.data(), A.col.data(),
                           max_lds, P) != 0) continue;
        plans++;
        check_wave(P, max_lds, what); check_blob(P.blob, what); (void)wreg_plan_report(P, s);
    }
    {
        BigHostPlan P;
        snprintf(what, sizeof(what), "%s big", name);
        if (big_host_plan(A.m, A.n, (int)A.val.size(), A.val.data(), A.ptr.data(), A.col.data(), max_lds, P) == 0) {
            plans++;
            CHECK(2L * P.tab.lds_bytes <= max_lds && P.tab.lds_bytes % 8 == 0, "%s: lds %d", what, P.tab.lds_bytes);
            CHECK((size_t)P.tab.lds_bytes == 8 * big_lds_doubles(P.tab.MB, A.n, P.tab.m_in_lds != 0), "%s: lds", what);
            check_blob(P.blob, what); (void)big_plan_report(P, s);
        }
    }
    if (A.m <= BLK_MAX_M && A.n <= BLK_MAX_N) {
        BlockHostPlan P;
        snprintf(what, sizeof(what), "%s block", name);
        if (block_host_plan(A.m, A.n, (int)A.val.size(), A.val.data(), A.ptr.data(), A.col.data(), max_lds, P) == 0) {
            plans++;
            CHECK(P.lds <= max_lds && P.lds_with_a <= max_lds && P.lds % 4 == 0, "%s: lds %d", what, P.lds);
            check_blob(P.blob, what); (void)block_plan_report(P, s);
        }
    }
}

}  // namespace

int main() {
    char name[64];
    unsigned seed = 1;
    const int sizes[][2] = { {1, 5}, {3, 1}, {1, 1}, {5, 9}, {16, 64}, {17, 65}, {33, 129}, {64, 256}, {100, 300}, {113, 385}, {128, 512},
                             {129, 200}, {200, 900}, {256, 1280} };
    for (const auto& sz : sizes)
        for (double density : {0.0, 0.02, 0.1, 0.3, 1.0})
            for (int tail = 0; tail < 2; tail++) {
                if (sz[0] * (double)sz[1] * density > 40000.0 && density > 0.3) continue;      // (dense and large: the three below)
                snprintf(name, sizeof(name), "%dx%d at %g%s", sz[0], sz[1], density, tail ? " with tail" : "");
                every_kind(random_csr(sz[0], sz[1], density, tail != 0, seed++), name);
            }
    // the largest compiled shapes
    every_kind(random_csr(128, 512, 0.025, true, 101), "128x512 at 0.025 with tail");
    every_kind(random_csr(256, 1280, 0.02, true, 102), "256x1280 at 0.02 with tail");
    every_kind(random_csr(112, 384, 1.0, true, 103), "112x384 dense with tail");
    every_kind(random_csr(48, 384, 1.0, false, 104), "48x384 dense");
    // an A with an empty row and an empty column
    Csr hollow{3, 4, {1.0, 2.0, 3.0, 4.0}, {0, 2, 2, 4}, {0, 2, 0, 3}};
    every_kind(hollow, "hollow");
    printf("plan_check: %d plans built, %d checks failed\n", plans, failures);
    return failures ? 1 : 0;
}
