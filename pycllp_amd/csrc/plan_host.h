// plan_host.h -- the passes every plan builder of the sparse handle runs over A's CSR arrays (wreg_plan.h: the wavefront-per-LP
// kernels, big_plan.h: the large-LP kernel, block_plan.h: the block kernel), each written once: CSR -> CSC, the identity-tail
// test, the enumeration of the Gram terms, the blob the tables are packed into, and the digest of a plan that
// pycllp_hip_debug_plan reports.  Host only, standard C++ only (no HIP header): a plain C++ program can include it.
#ifndef PYCLLP_PLAN_HOST_H
#define PYCLLP_PLAN_HOST_H
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// A by columns, rows ascending inside a column; src: the CSR index of each entry
struct PlanCsc { std::vector<int> ptr, row, src; std::vector<double> val; };

// CSR -> CSC by counting sort
inline PlanCsc csc_from_csr(int m, int n, int nnz, const int* ptr, const int* col, const double* val) {
    PlanCsc c;
    c.ptr.assign((size_t)n + 1, 0); c.row.resize(nnz); c.src.resize(nnz); c.val.resize(nnz);
    for (int e = 0; e < nnz; e++) c.ptr[col[e] + 1]++;
    for (int j = 0; j < n; j++) c.ptr[j + 1] += c.ptr[j];
    std::vector<int> fill(c.ptr.begin(), c.ptr.end() - 1);
    for (int i = 0; i < m; i++)
        for (int e = ptr[i]; e < ptr[i + 1]; e++) { const int p = fill[col[e]]++; c.row[p] = i; c.val[p] = val[e]; c.src[p] = e; }
    return c;
}

// the last m columns are exactly the identity (equality form of a StandardLP): column n - m + i holds one entry, a 1.0 in row i
inline bool identity_tail(int m, int n, const int* ptr, const int* col, const double* val) {
    bool sl = n > m;
    std::vector<int> tail_cnt(sl ? m : 0, 0);
    for (int i = 0; i < m && sl; i++)
        for (int e = ptr[i]; e < ptr[i + 1]; e++)
            if (col[e] >= n - m) { if (col[e] != n - m + i || val[e] != 1.0) sl = false; else tail_cnt[i]++; }
    for (int i = 0; i < m && sl; i++) if (tail_cnt[i] != 1) sl = false;
    return sl;
}

// The Gram terms a_ij a_kj of M = A D A', in the order (column j, entry a of the column, entry b2 <= a -- b2 < a without DIAG):
// term(i, k, j, weight, ia, ib) with rows i >= k and the CSR indices of both entries.  False, and no further term, once more
// than `cap` terms were visited.
template <bool DIAG, typename Term>
inline bool gram_terms(int n, const PlanCsc& c, size_t cap, Term&& term) {
    size_t count = 0;
    for (int j = 0; j < n; j++)
        for (int a = c.ptr[j]; a < c.ptr[j + 1]; a++)
            for (int b2 = c.ptr[j]; DIAG ? b2 <= a : b2 < a; b2++) {
                term(c.row[a], c.row[b2], j, c.val[a] * c.val[b2], c.src[a], c.src[b2]);
                if (++count > cap) return false;
            }
    return true;
}

// The tables of a plan packed for one upload: sections aligned to 16 bytes, an empty vector takes none (its offset is that of
// whatever follows).  put() hands out the offsets, pack() copies every table once into storage of the final size: the vectors
// put must live until then.  sec: what was put, in order.
struct PlanBlob {
    struct Section { size_t off, count, elem; const void* src; };
    std::vector<char> bytes;
    std::vector<Section> sec;
    size_t size = 0;
    template <typename T>
    size_t put(const std::vector<T>& v) {
        const size_t off = (size + 15) & ~(size_t)15;
        size = off + v.size() * sizeof(T);
        sec.push_back({off, v.size(), sizeof(T), v.data()});
        return off;
    }
    template <typename T> size_t put(std::vector<T>&&) = delete;
    void pack() {
        bytes.resize(size);
        for (Section& s : sec) { if (s.count) memcpy(bytes.data() + s.off, s.src, s.count * s.elem); s.src = nullptr; }
    }
};

// FNV-1a, 64 bits
struct PlanDigest {
    uint64_t h = 14695981039346656037ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    }
    void word(long long v) { bytes(&v, sizeof(v)); }
};
// What pycllp_hip_debug_plan reports of a plan: PLAN_NSCALARS scalar fields (each plan header lists its own; the rest 0) and
// a digest -- every table in the order it was put, its element count (64 bits) and then its bytes, then the scalars (64 bits
// each).  Over contents, not over the blob's layout.
constexpr int PLAN_NSCALARS = 32;
inline void plan_digest_tables(PlanDigest& d, const PlanBlob& b) {
    for (const PlanBlob::Section& s : b.sec) { d.word((long long)s.count); d.bytes(b.bytes.data() + s.off, s.count * s.elem); }
}
inline uint64_t plan_digest_scalars(PlanDigest& d, const long long* scalars) {
    for (int i = 0; i < PLAN_NSCALARS; i++) d.word(scalars[i]);
    return d.h;
}
#endif
