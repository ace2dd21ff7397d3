// big_plan.h -- the plan of the large-LP kernel (ipm_big.hip), built on the host without a HIP call: CSR / CSC copies of A, the
// Gram term list or the dense images, and where the factor blocks sit.  ipm_big.hip uploads the blob and sets the device
// pointers (big_plan_create); pycllp_hip_debug_plan and plan_check.hip read the result as it stands.  Host code only.
#ifndef PYCLLP_BIG_PLAN_H
#define PYCLLP_BIG_PLAN_H
#include "big.h"
#include "plan_host.h"

// A plan as the host builds it: the device view with every field but the device pointers, the tables, their offsets in the blob
struct BigHostPlan {
    BigTab tab;
    size_t ws_doubles_per_block = 0;     // the L2 workspace a workgroup needs for the factor blocks (0: they sit in LDS)
    PlanBlob blob;
    size_t a_csr_val = 0, a_csr_ptr = 0, a_csr_col = 0, a_csc_val = 0, a_csc_ptr = 0, a_csc_row = 0, a_img = 0, a_ent_dst = 0,
           a_ent_dst2 = 0, a_ent_ptr = 0, a_term_w = 0, a_term_col = 0, a_img_rm = 0, a_img_cm = 0;
    BigHostPlan() { memset(&tab, 0, sizeof(tab)); }
};

// Returns 0, or 1 when the problem is outside the kernel's limits
inline int big_host_plan(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds, BigHostPlan& P) {
    if (m > BIG_MAX_M || n > BIG_MAX_N || m < 1 || n < 1) return 1;
    const int MB = (m + 15) / 16, MP = 16 * MB;
    BigTab& T = P.tab;
    T.m = m; T.n = n; T.nnz = nnz; T.MB = MB;
    const PlanCsc csc = csc_from_csr(m, n, nnz, ptr, col, val);
    const int nd = identity_tail(m, n, ptr, col, val) ? n - m : n;      // (equality form of a StandardLP: the tail is implied)
    // ---- Gram by term list or on the matrix cores?  terms = sum over columns of len (len + 1) / 2 products per Newton step,
    //      against MP^2 / 2 * nd for the dense product at the 8x higher rate of the matrix pipe over a gather-bound loop ----
    double n_terms = 0.0;
    for (int j = 0; j < n; j++) { const double l = csc.ptr[j + 1] - csc.ptr[j]; n_terms += l * (l + 1) / 2; }
    T.dense = n_terms > 0.125 * (double)MP * MP * nd ? 1 : 0;
    std::vector<double> img, img_rm, img_cm;
    std::vector<int> ent_dst, ent_dst2, ent_ptr, term_col;
    std::vector<double> term_w;
    if (T.dense) {
        T.nd = nd; T.n_sl = n - nd; T.ks = (nd + 3) / 4; T.imgR = MP;
        img.assign((size_t)T.ks * MP * 4, 0.0);
        img_rm.assign((size_t)m * nd, 0.0);
        img_cm.assign((size_t)nd * MP, 0.0);
        for (int i = 0; i < m; i++)
            for (int e = ptr[i]; e < ptr[i + 1]; e++)
                if (col[e] < nd) {
                    img[((size_t)(col[e] >> 2) * MP + i) * 4 + (col[e] & 3)] = val[e];
                    img_rm[(size_t)i * nd + col[e]] = val[e];
                    img_cm[(size_t)col[e] * MP + i] = val[e];
                }
    } else {
        struct Term { int key, colj; double w; };
        std::vector<Term> terms;
        const size_t max_terms = (size_t)1 << 24;      // one more refuses the plan
        if (!gram_terms<true>(n, csc, max_terms, [&](int i, int k, int j, double w, int, int) { terms.push_back({i * m + k, j, w}); }))
            return 1;
        std::stable_sort(terms.begin(), terms.end(), [](const Term& x, const Term& y) { return x.key < y.key; });
        term_col.resize(terms.size()); term_w.resize(terms.size());
        for (size_t t = 0; t < terms.size(); t++) {
            if (t == 0 || terms[t].key != terms[t - 1].key) {
                const int i = terms[t].key / m, k = terms[t].key % m;
                const int K = k >> 4, I = i >> 4, kl = k & 15, il = i & 15;
                ent_dst.push_back(bidx(K, I) * 256 + boff(kl, il));
                ent_dst2.push_back((K == I && kl != il) ? bidx(K, K) * 256 + boff(il, kl) : -1);
                ent_ptr.push_back((int)t);
            }
            term_col[t] = terms[t].colj; term_w[t] = terms[t].w;
        }
        ent_ptr.push_back((int)terms.size());
        T.n_ent = (int)ent_dst.size();
    }
    // ---- LDS plan: the blocks in LDS only when two workgroups still fit a CU with them -- measured (round 3,
    //      profiles/r03/large_lp_kernel.txt): a second resident workgroup is worth more than LDS-resident blocks (m = 144 with
    //      the blocks in LDS and one workgroup per CU: 22 k LPs/s; with the blocks in the L2 workspace and two: 35 k, three: 44 k) ----
    T.m_in_lds = big_lds_doubles(MB, n, true) * sizeof(double) * 2 <= (size_t)max_lds ? 1 : 0;
    const size_t lds = big_lds_doubles(MB, n, T.m_in_lds != 0) * sizeof(double);
    if (lds > (size_t)max_lds) return 1;
    T.lds_bytes = (int)lds;
    P.ws_doubles_per_block = T.m_in_lds ? 0 : (size_t)MB * (MB + 1) / 2 * 256;
    // ---- the tables, as uploaded ----
    PlanBlob& b = P.blob;
    const std::vector<double> csr_val(val, val + nnz);
    const std::vector<int> csr_ptr(ptr, ptr + m + 1), csr_col(col, col + nnz);
    P.a_csr_val = b.put(csr_val); P.a_csr_ptr = b.put(csr_ptr); P.a_csr_col = b.put(csr_col);
    P.a_csc_val = b.put(csc.val); P.a_csc_ptr = b.put(csc.ptr); P.a_csc_row = b.put(csc.row);
    P.a_img = b.put(img); P.a_ent_dst = b.put(ent_dst); P.a_ent_dst2 = b.put(ent_dst2); P.a_ent_ptr = b.put(ent_ptr);
    P.a_term_w = b.put(term_w); P.a_term_col = b.put(term_col); P.a_img_rm = b.put(img_rm); P.a_img_cm = b.put(img_cm);
    b.pack();
    return 0;
}

// The scalar fields of a plan (plan_host.h): MB, dense, m_in_lds, lds_bytes, n_ent, ks, workspace doubles per workgroup, nd,
// imgR, n_sl.  The digest: the tables (csr_val, csr_ptr, csr_col, csc_val, csc_ptr, csc_row, img, ent_dst, ent_dst2, ent_ptr,
// term_w, term_col, img_rm, img_cm), the scalars.
inline uint64_t big_plan_report(const BigHostPlan& P, long long* s) {
    const BigTab& T = P.tab;
    const long long v[PLAN_NSCALARS] = { T.MB, T.dense, T.m_in_lds, T.lds_bytes, T.n_ent, T.ks, (long long)P.ws_doubles_per_block,
                                         T.nd, T.imgR, T.n_sl };
    memcpy(s, v, sizeof(v));
    PlanDigest d;
    plan_digest_tables(d, P.blob);
    return plan_digest_scalars(d, s);
}
#endif
