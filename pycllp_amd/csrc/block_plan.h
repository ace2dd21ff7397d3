// block_plan.h -- the plan of the block kernel (ipm_block.inc), built on the host without a HIP call: CSR / CSC copies of A, the
// Gram term list, and whether A's arrays go into LDS.  sparse_init_host (abi_sparse.hip) uploads the blob and sets the device
// pointers; pycllp_hip_debug_plan and plan_check.hip read the result as it stands.  Host code only.
#ifndef PYCLLP_BLOCK_PLAN_H
#define PYCLLP_BLOCK_PLAN_H
#include "block.h"
#include "plan_host.h"

// A plan as the host builds it: the device view with every field but the device pointers, the tables, their offsets in the blob
struct BlockHostPlan {
    BlockA desc;
    int lds = 0;            // LDS bytes of a workgroup
    int lds_with_a = 0;     // ... with A's arrays in LDS (what per-problem values need), 0 when that does not fit
    PlanBlob blob;
    size_t a_csr_val = 0, a_csr_ptr = 0, a_csr_col = 0, a_csc_val = 0, a_csc_ptr = 0, a_csc_row = 0, a_ent_tri = 0, a_ent_ptr = 0,
           a_term_w = 0, a_term_col = 0, a_csc_src = 0, a_term_ia = 0, a_term_ib = 0;
    BlockHostPlan() { memset(&desc, 0, sizeof(desc)); }
};

enum { BLOCK_PLAN_OK = 0, BLOCK_PLAN_TOO_DENSE = 1, BLOCK_PLAN_NO_LDS = 2 };

inline int block_host_plan(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds, BlockHostPlan& P) {
    const PlanCsc csc = csc_from_csr(m, n, nnz, ptr, col, val);
    // Gram term list: entry (i,k), i >= k, gets a term a_ij a_kj for every column j holding both rows
    struct Term { int key, colj; double w; int ia, ib; };
    std::vector<Term> terms;
    if (!gram_terms<true>(n, csc, (size_t)8 << 20, [&](int i, int k, int j, double w, int ia, int ib) {
            terms.push_back({i * (i + 1) / 2 + k, j, w, ia, ib}); }))
        return BLOCK_PLAN_TOO_DENSE;
    std::stable_sort(terms.begin(), terms.end(), [](const Term& x, const Term& y) { return x.key < y.key; });
    std::vector<int> ent_tri, ent_ptr, term_col(terms.size()), term_ia(terms.size()), term_ib(terms.size());
    std::vector<double> term_w(terms.size());
    for (size_t t = 0; t < terms.size(); t++) {
        if (t == 0 || terms[t].key != terms[t - 1].key) { ent_tri.push_back(terms[t].key); ent_ptr.push_back((int)t); }
        term_col[t] = terms[t].colj; term_w[t] = terms[t].w; term_ia[t] = terms[t].ia; term_ib[t] = terms[t].ib;
    }
    ent_ptr.push_back((int)terms.size());
    BlockA& d = P.desc;
    d.m = m; d.n = n; d.nnz = nnz;
    d.n_entries = (int)ent_tri.size(); d.n_terms = (int)terms.size();
    // LDS plan: two workgroups per CU hide each other's LDS latency, so the CSR/CSC copy goes into LDS only when the
    // workgroup still fits in half a CU (or when it cannot be paired anyway)
    const size_t base = block_lds_bytes(m, n, nnz, false), with_a = block_lds_bytes(m, n, nnz, true);
    const size_t half = (size_t)max_lds / 2;
    if (with_a <= half) d.a_in_lds = 1;
    else if (base <= half) d.a_in_lds = 0;
    else d.a_in_lds = with_a <= (size_t)max_lds ? 1 : 0;
    P.lds = (int)(d.a_in_lds ? with_a : base);
    P.lds_with_a = with_a <= (size_t)max_lds ? (int)with_a : 0;
    if ((size_t)P.lds > (size_t)max_lds) return BLOCK_PLAN_NO_LDS;
    // ---- the tables, as uploaded ----
    PlanBlob& b = P.blob;
    const std::vector<double> csr_val(val, val + nnz);
    const std::vector<int> csr_ptr(ptr, ptr + m + 1), csr_col(col, col + nnz);
    P.a_csr_val = b.put(csr_val); P.a_csr_ptr = b.put(csr_ptr); P.a_csr_col = b.put(csr_col);
    P.a_csc_val = b.put(csc.val); P.a_csc_ptr = b.put(csc.ptr); P.a_csc_row = b.put(csc.row);
    P.a_ent_tri = b.put(ent_tri); P.a_ent_ptr = b.put(ent_ptr); P.a_term_w = b.put(term_w); P.a_term_col = b.put(term_col);
    P.a_csc_src = b.put(csc.src); P.a_term_ia = b.put(term_ia); P.a_term_ib = b.put(term_ib);
    b.pack();
    return BLOCK_PLAN_OK;
}

// The scalar fields of a plan (plan_host.h): a_in_lds, lds, lds_with_a, n_entries, n_terms.  The digest: the tables (csr_val,
// csr_ptr, csr_col, csc_val, csc_ptr, csc_row, ent_tri, ent_ptr, term_w, term_col, csc_src, term_ia, term_ib), the scalars.
inline uint64_t block_plan_report(const BlockHostPlan& P, long long* s) {
    const long long v[PLAN_NSCALARS] = { P.desc.a_in_lds, P.lds, P.lds_with_a, P.desc.n_entries, P.desc.n_terms };
    memcpy(s, v, sizeof(v));
    PlanDigest d;
    plan_digest_tables(d, P.blob);
    return plan_digest_scalars(d, s);
}
#endif
