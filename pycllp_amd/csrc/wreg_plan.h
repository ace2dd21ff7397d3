// wreg_plan.h -- the plans of the wavefront-per-LP kernels, built on the host without a HIP call: the variant, the term tables
// or the dense image, the LDS layout and the waves per workgroup of one constraint matrix given as CSR arrays.  ipm_wreg.hip
// uploads the blob and sets the device pointers (wreg_plan_create*); pycllp_hip_debug_plan and plan_check.hip read the result
// as it stands.  Host code only.
#ifndef PYCLLP_WREG_PLAN_H
#define PYCLLP_WREG_PLAN_H
#include "wreg.h"
#include "plan_host.h"

struct WShape { int mb, nq; };
#define WSHAPE_ENTRY(MB, NQ) {MB, NQ},
static const std::vector<WShape> kWTabShapes = { WREG_TAB_SHAPES(WSHAPE_ENTRY) };
static const std::vector<WShape> kWDaShapes = { WREG_DA_SHAPES(WSHAPE_ENTRY) };
static const std::vector<WShape> kWDapaShapes = { WREG_DAPA_SHAPES(WSHAPE_ENTRY) };
static const std::vector<WShape> kWBddapaShapes = { WREG_BDDAPA_SHAPES(WSHAPE_ENTRY) };
#undef WSHAPE_ENTRY
// the shape list of a plan's kind as wreg.h has it (the library asks its launcher tables instead: ipm_wreg.hip)
inline const std::vector<WShape>& wreg_listed_shapes(bool da, bool pa, bool bd) {
    return da ? (pa ? (bd ? kWBddapaShapes : kWDapaShapes) : kWDaShapes) : kWTabShapes;
}

// the first shape of a list (ordered by cost) that covers (m, n), or null
inline const WShape* first_covering(const std::vector<WShape>& s, int m, int n) {
    for (const WShape& v : s)
        if (m <= 16 * v.mb && n <= 64 * v.nq) return &v;
    return nullptr;
}

// A plan as the host builds it: the device view with every field but the device pointers, the tables, their offsets in the blob
struct WregHostPlan {
    WregTab tab;
    int mb = 0, nq = 0;
    bool da = false, pa = false, bd = false;
    PlanBlob blob;
    size_t a_csr_val = 0, a_ec_val = 0, a_t_w = 0, a_lev = 0, a_csr_col = 0, a_csr_ptr = 0, a_csr_len = 0, a_ec_row = 0, a_colmap = 0,
           a_t_cd = 0, a_ec_src = 0, a_t_ab = 0, a_img = 0;
    WregHostPlan() { memset(&tab, 0, sizeof(tab)); }
};

// the kinds of plan: one per creator of wreg.h
enum WregPlanKind { WPLAN_SHARED, WPLAN_PA, WPLAN_BOUNDED, WPLAN_BOUNDED_PA, WPLAN_DENSE_PA, WPLAN_DENSE_PA_KEEP,
                    WPLAN_BOUNDED_DENSE_PA };

namespace wreg_plan_detail {

// what the dense-image plans share: the first covering variant and the image's geometry -- nd columns in front of an identity
// tail (all n without one, or with keep_tail), rows of AS doubles, R rows
inline const WShape* image_geometry(const std::vector<WShape>& shapes, int m, int n, int nnz, const double* val, const int* ptr,
                                    const int* col, bool keep_tail, WregHostPlan& P) {
    const WShape* v = first_covering(shapes, m, n);
    if (!v) return nullptr;
    const bool sl = !keep_tail && identity_tail(m, n, ptr, col, val);
    const int nd = sl ? n - m : n, ndp = ((std::max(nd, 1) + 15) / 16) * 16;   // (16: gram_dense takes four k-steps per trip)
    WregTab& T = P.tab;
    T.m = m; T.n = n; T.nnz = nnz; T.nd = nd; T.as = ndp + 1; T.img_rows = ((m + 7) / 8) * 8;
    P.mb = v->mb; P.nq = v->nq; P.da = true;
    return v;
}

// the most waves per workgroup, 4 down to 1, whose areas fit max_lds beside `front` bytes; 0 when not even one does
inline int most_waves(size_t front, int wave_doubles, int max_lds) {
    for (int w = 4; w >= 1; w--)
        if (front + sizeof(double) * (size_t)w * wave_doubles <= (size_t)max_lds) return w;
    return 0;
}

}  // namespace wreg_plan_detail

// Plan with A as a dense image in LDS (no tables): for matrices whose Gram term list does not fit -- dense A's, e.g. the LPs
// hip_dense_primal_normal hands over beyond m = 32.  The last m columns are kept out of the image when they are the
// identity (equality form of a StandardLP).  Fewer than four waves per workgroup when that is what lets the image fit.
// bd: the plan of the bounded kernel (t and s behind every wave area).  Returns 0, or 1 when no shape or LDS plan covers A.
inline int wreg_image_plan(const std::vector<WShape>& shapes, int m, int n, int nnz, const double* val, const int* ptr, const int* col,
                           int max_lds, bool bd, WregHostPlan& P) {
    using namespace wreg_plan_detail;
    if (!image_geometry(shapes, m, n, nnz, val, ptr, col, false, P)) return 1;
    WregTab& T = P.tab;
    T.wave_doubles = wave_doubles(P.mb, P.nq) + (bd ? 2 * 64 * P.nq : 0);
    const size_t img_bytes = sizeof(double) * (size_t)T.img_rows * T.as;
    T.wpb = most_waves(img_bytes + 16, T.wave_doubles, max_lds);
    if (!T.wpb) return 1;
    T.o_img = 0; T.o_wave = (int)((img_bytes + 15) & ~(size_t)15);
    T.lds_bytes = T.o_wave + (int)(sizeof(double) * (size_t)T.wpb * T.wave_doubles);
    std::vector<double> img((size_t)T.img_rows * T.as, 0.0);
    for (int i = 0; i < m; i++)
        for (int e = ptr[i]; e < ptr[i + 1]; e++)
            if (col[e] < T.nd) img[(size_t)i * T.as + col[e]] = val[e];
    P.a_img = P.blob.put(img);
    P.blob.pack();
    P.bd = bd;
    return 0;
}

// The plan of the kernel on per-problem dense matrices: the geometry of the image plan, an image behind every wave area and
// nothing in front of the waves, no table.  keep_tail: an identity tail stays in the image.  bd: the plan of the bounded kernel
// (t and s behind every wave's image: [wave area | image | t NP | s NP]).
inline int wreg_image_pa_plan(const std::vector<WShape>& shapes, int m, int n, int nnz, const double* val, const int* ptr,
                              const int* col, int max_lds, bool keep_tail, WregHostPlan& P, bool bd = false) {
    using namespace wreg_plan_detail;
    if (!image_geometry(shapes, m, n, nnz, val, ptr, col, keep_tail, P)) return 1;
    WregTab& T = P.tab;
    T.pa = 1;
    T.wave_doubles = wave_doubles(P.mb, P.nq) + T.img_rows * T.as + (bd ? 2 * 64 * P.nq : 0);
    T.wpb = most_waves(0, T.wave_doubles, max_lds);
    if (!T.wpb) return 1;
    T.o_img = 0; T.o_wave = 0;
    T.lds_bytes = (int)(sizeof(double) * (size_t)T.wpb * T.wave_doubles);
    P.pa = true; P.bd = bd;
    return 0;
}

// Plan on term tables.  pa: the structure-only tables of the per-problem-A variants (the values `val` only stand in where a
// table still wants one; no kernel of those variants reads them).  bd: the plan of the bounded kernel (t and s behind every wave
// area, fewer waves per workgroup where that is what lets the tables fit).  Returns 0, or 1 when no shape covers A or its
// tables do not fit.
inline int wreg_tables_plan(const std::vector<WShape>& shapes, int m, int n, int nnz, const double* val, const int* ptr, const int* col,
                            int max_lds, bool pa, bool bd, WregHostPlan& P) {
    const WShape* v = first_covering(shapes, m, n);
    if (!v || nnz >= 65535) return 1;
    const int MB = v->mb, NQ = v->nq;
    const int MP = 16 * MB, MPL = 64 * ((MP + 63) / 64), NP = 64 * NQ;
    WregTab& T = P.tab;
    T.m = m; T.n = n; T.nnz = nnz;
    // ---- column positions: the columns sorted by length (longest first) are dealt to positions 0, 1, ...; position p
    //      is element p % 64 of N-vector register p / 64, so every register holds 64 columns of similar length ----
    const PlanCsc csc = csc_from_csr(m, n, nnz, ptr, col, val);
    const std::vector<int>& cptr = csc.ptr;
    std::vector<int> order(n), posof(n);
    for (int j = 0; j < n; j++) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cptr[a + 1] - cptr[a] > cptr[b + 1] - cptr[b]; });
    std::vector<unsigned> colmap(NP, PAD_OFF);
    for (int p = 0; p < n; p++) { colmap[p] = 8u * (unsigned)order[p]; posof[order[p]] = p; }
    // ---- A by rows (column indices = positions), compact ----
    std::vector<double> csr_val(val, val + nnz);
    std::vector<unsigned short> csr_col(nnz), csr_ptr(MPL, 0), csr_len(MPL, 0);
    int rmax = 0;
    for (int i = 0; i < m; i++) {
        csr_ptr[i] = (unsigned short)ptr[i]; csr_len[i] = (unsigned short)(ptr[i + 1] - ptr[i]);
        rmax = std::max(rmax, ptr[i + 1] - ptr[i]);
    }
    for (int e = 0; e < nnz; e++) csr_col[e] = (unsigned short)posof[col[e]];
    T.rmax = rmax;
    // ---- A by columns, ELL over positions ----
    int ctot = 0;
    for (int q = 0; q < NQ; q++) {
        int cm = 0;
        for (int p = 64 * q; p < std::min(n, 64 * q + 64); p++) cm = std::max(cm, cptr[order[p] + 1] - cptr[order[p]]);
        T.meta[q] = cm; T.meta[META_COFF + q] = ctot; ctot += cm;
    }
    T.ctot = ctot;
    std::vector<double> ec_val((size_t)std::max(ctot, 1) * 64, 0.0);
    std::vector<unsigned short> ec_row((size_t)std::max(ctot, 1) * 64, 0);
    std::vector<unsigned short> ec_src((size_t)std::max(ctot, 1) * 64, (unsigned short)nnz);      // padded slots: the zero entry
    for (int p = 0; p < n; p++) {
        const int j = order[p], q = p / 64, l = p % 64;
        for (int e = cptr[j], t = 0; e < cptr[j + 1]; e++, t++) {
            ec_val[(size_t)(T.meta[META_COFF + q] + t) * 64 + l] = csc.val[e];
            ec_row[(size_t)(T.meta[META_COFF + q] + t) * 64 + l] = (unsigned short)csc.row[e];
            ec_src[(size_t)(T.meta[META_COFF + q] + t) * 64 + l] = (unsigned short)csc.src[e];
        }
    }
    // ---- Gram entries (strictly lower triangle of M): off-diagonal blocks grouped by staging chunk (HB blocks of the
    //      linear block order each); the entries inside the diagonal blocks go to their slots in the W area, as part of
    //      the last chunk's group when that chunk ends in front of the W area, else as a group of their own.  All
    //      destinations are offsets from the start of the stage. ----
    struct Term { int group, dst, colj; double w; int ia, ib; };
    std::vector<Term> terms;
    const int nblk = MB * (MB - 1) / 2, nchunk = (nblk + HB - 1) / HB;
    const bool merge = merge_diag(MB, NQ);
    const int diag_group = merge ? nchunk - 1 : nchunk, ngroup = merge ? nchunk : nchunk + 1;
    if (ngroup + 1 > META_N - META_SEG || stage_d(NQ) + MB * WL > 65535) return 1;
    const bool few = gram_terms<false>(n, csc, (size_t)1 << 22, [&](int i, int k, int j, double w, int ia, int ib) {
        const int K = k / 16, I = i / 16, il = i % 16, kl = k % 16;      // rows ascend inside a column: i > k
        if (I == K) {          // diagonal block K: element [il][kl] of the packed lower triangle in slot K
            terms.push_back({diag_group, stage_d(NQ) + K * WL + il * (il + 1) / 2 + kl, posof[j], w, ia, ib});
        } else {               // block (K, I) of U: element [kl][il] of block bix % HB of chunk bix / HB
            const int bx = K * MB - K * (K + 1) / 2 + (I - K - 1);
            terms.push_back({bx / HB, (bx % HB) * 256 + kl * 16 + il, posof[j], w, ia, ib});
        }
    });
    if (!few) return 1;
    // Records of a group: first the FIRST term of every entry (one flat pass), then rounds of triples -- terms 2..4 of the
    // entries that have them, then terms 5..7, ... -- in column order (the order a per-entry loop would add them in), short
    // triples padded with weight 0.  lev[] holds the record boundaries, meta[META_SEG + g] the first boundary of group g.
    std::stable_sort(terms.begin(), terms.end(), [](const Term& a, const Term& b) {
        return a.group != b.group ? a.group < b.group : a.dst < b.dst; });
    std::vector<double> t_w;
    std::vector<unsigned> t_cd, t_ab;
    const unsigned ab_zero = (unsigned)nnz | ((unsigned)nnz << 16);       // padded records: 0 x 0
    std::vector<int> lev(1, 0), gl(ngroup + 1, 0);
    {
        size_t t0 = 0;
        for (int g = 0; g < ngroup; g++) {
            size_t t1 = t0;
            while (t1 < terms.size() && terms[t1].group == g) t1++;
            gl[g] = (int)lev.size() - 1;
            // entries of the group: [e0, e1) term ranges
            std::vector<std::pair<size_t, size_t>> ent;
            for (size_t t = t0; t < t1;) {
                size_t u = t + 1;
                while (u < t1 && terms[u].dst == terms[t].dst) u++;
                ent.push_back({t, u}); t = u;
            }
            if (!ent.empty()) {
                for (auto& e : ent) {
                    t_w.push_back(terms[e.first].w); t_cd.push_back((unsigned)terms[e.first].colj | ((unsigned)terms[e.first].dst << 16));
                    t_ab.push_back((unsigned)terms[e.first].ia | ((unsigned)terms[e.first].ib << 16));
                }
                lev.push_back((int)t_w.size());
                for (size_t r = 0;; r++) {
                    bool any = false;
                    for (auto& e : ent) {
                        const size_t f = e.first + 1 + 3 * r;
                        if (f >= e.second) continue;
                        any = true;
                        for (size_t k = 0; k < 3; k++) {
                            const bool have = f + k < e.second;
                            t_w.push_back(have ? terms[f + k].w : 0.0);
                            t_cd.push_back((have ? (unsigned)terms[f + k].colj : 0u) | ((unsigned)terms[e.first].dst << 16));
                            t_ab.push_back(have ? ((unsigned)terms[f + k].ia | ((unsigned)terms[f + k].ib << 16)) : ab_zero);
                        }
                    }
                    if (!any) break;
                    lev.push_back((int)t_w.size());
                }
            }
            t0 = t1;
        }
        gl[ngroup] = (int)lev.size() - 1;
    }
    for (int g = 0; g <= ngroup; g++) T.meta[META_SEG + g] = gl[g];
    T.n_lev = (int)lev.size() - 1; T.n_term = (int)t_w.size();
    if (t_w.empty()) { t_w.push_back(0.0); t_cd.push_back(0); t_ab.push_back(ab_zero); }
    // ---- LDS plan ----
    // PA: no value tables; every wave carries nnzp doubles of its LP's values behind its area, and as many waves share a
    // workgroup as the LDS takes (three at config 5's structure: 3 x 37.6 KB + 22 KB of structure tables)
    T.pa = pa ? 1 : 0;
    T.nnzp = pa ? ((nnz + 1 + 1) & ~1) : 0;
    T.wave_doubles = wave_doubles(MB, NQ) + T.nnzp + (bd ? 2 * NP : 0);
    int wpb = 4;
    for (;;) {
        size_t off = 0;
        auto take = [&](size_t bytes) { off = (off + 15) & ~(size_t)15; const size_t o_ = off; off += bytes; return (int)o_; };
        if (!pa) {
            T.o_csr_val = take(sizeof(double) * csr_val.size());
            T.o_ec_val = take(sizeof(double) * ec_val.size());
            T.o_t_w = take(sizeof(double) * t_w.size());
        }
        T.o_wave = take(sizeof(double) * (size_t)wpb * (size_t)T.wave_doubles);
        T.o_lev = take(sizeof(int) * lev.size());
        T.o_t_cd = take(sizeof(unsigned) * t_cd.size());
        if (pa) T.o_t_ab = take(sizeof(unsigned) * t_ab.size());
        T.o_colmap = take(sizeof(unsigned) * colmap.size());
        T.o_meta = take(sizeof(int) * META_N);
        T.o_csr_col = take(sizeof(unsigned short) * csr_col.size());
        T.o_csr_ptr = take(sizeof(unsigned short) * csr_ptr.size());
        T.o_csr_len = take(sizeof(unsigned short) * csr_len.size());
        T.o_ec_row = take(sizeof(unsigned short) * ec_row.size());
        if (pa) T.o_ec_src = take(sizeof(unsigned short) * ec_src.size());
        T.lds_bytes = (int)((off + 15) & ~(size_t)15);
        if (T.lds_bytes <= max_lds) break;
        if (!(pa || bd) || wpb == 1) return 1;
        wpb--;
    }
    T.wpb = wpb;
    // ---- the tables, as uploaded ----
    PlanBlob& b = P.blob;
    P.a_csr_val = b.put(csr_val); P.a_ec_val = b.put(ec_val); P.a_t_w = b.put(t_w); P.a_lev = b.put(lev);
    P.a_csr_col = b.put(csr_col); P.a_csr_ptr = b.put(csr_ptr); P.a_csr_len = b.put(csr_len); P.a_ec_row = b.put(ec_row);
    P.a_colmap = b.put(colmap); P.a_t_cd = b.put(t_cd); P.a_ec_src = b.put(ec_src); P.a_t_ab = b.put(t_ab);
    b.pack();
    P.mb = MB; P.nq = NQ; P.pa = pa; P.bd = bd;
    return 0;
}

// The plan of a creator of wreg.h.  shapes_of(da, pa, bd): the shape list of a plan's kind.  A plan on a shared A takes the
// term tables where they fit and the dense image where they do not.
template <typename ShapesOf>
inline int wreg_host_plan(WregPlanKind kind, ShapesOf&& shapes_of, int m, int n, int nnz, const double* val, const int* ptr,
                          const int* col, int max_lds, WregHostPlan& P) {
    const bool bd = kind == WPLAN_BOUNDED || kind == WPLAN_BOUNDED_PA;
    if (kind == WPLAN_DENSE_PA || kind == WPLAN_DENSE_PA_KEEP)
        return wreg_image_pa_plan(shapes_of(true, true, false), m, n, nnz, val, ptr, col, max_lds, kind == WPLAN_DENSE_PA_KEEP, P);
    if (kind == WPLAN_BOUNDED_DENSE_PA)
        return wreg_image_pa_plan(shapes_of(true, true, true), m, n, nnz, val, ptr, col, max_lds, false, P, true);
    const bool pa = kind == WPLAN_PA || kind == WPLAN_BOUNDED_PA;
    const int rc = wreg_tables_plan(shapes_of(false, pa, bd), m, n, nnz, val, ptr, col, max_lds, pa, bd, P);
    if (rc != 1 || pa) return rc;
    P = WregHostPlan();
    return wreg_image_plan(shapes_of(true, false, bd), m, n, nnz, val, ptr, col, max_lds, bd, P);
}

// The scalar fields of a plan (plan_host.h): mb, nq, waves per workgroup, lds_bytes, wave_doubles, nd, as, img_rows, rmax, ctot,
// n_lev, n_term, nnzp, variant (1 term tables, 2 dense image), pa, bd, then the LDS offsets o_csr_val, o_ec_val, o_t_w, o_wave,
// o_lev, o_meta, o_csr_col, o_csr_ptr, o_csr_len, o_ec_row, o_colmap, o_t_cd, o_ec_src, o_t_ab, o_img.  The digest: the tables
// (csr_val, ec_val, t_w, lev, csr_col, csr_ptr, csr_len, ec_row, colmap, t_cd, ec_src, t_ab -- or the image), meta, the scalars.
inline uint64_t wreg_plan_report(const WregHostPlan& P, long long* s) {
    const WregTab& T = P.tab;
    const long long v[PLAN_NSCALARS] = {
        P.mb, P.nq, T.wpb, T.lds_bytes, T.wave_doubles, T.nd, T.as, T.img_rows, T.rmax, T.ctot, T.n_lev, T.n_term, T.nnzp,
        P.da ? 2 : 1, P.pa, P.bd, T.o_csr_val, T.o_ec_val, T.o_t_w, T.o_wave, T.o_lev, T.o_meta, T.o_csr_col, T.o_csr_ptr,
        T.o_csr_len, T.o_ec_row, T.o_colmap, T.o_t_cd, T.o_ec_src, T.o_t_ab, T.o_img, 0 };
    memcpy(s, v, sizeof(v));
    PlanDigest d;
    plan_digest_tables(d, P.blob);
    d.word(META_N); d.bytes(T.meta, sizeof(T.meta));
    return plan_digest_scalars(d, s);
}

// ... on the shapes the library's launcher tables hold (ipm_wreg.hip): what wreg_plan_create* upload
int wreg_plan_host(WregPlanKind kind, int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                   WregHostPlan* out);
#endif
