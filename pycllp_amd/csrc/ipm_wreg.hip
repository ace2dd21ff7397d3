// ipm_wreg.hip -- host side of the register-resident one-LP-per-wavefront kernels (wreg_wave.h): the plan of one constraint
// matrix (term tables or dense image, LDS layout), the choice of a launcher from the tables of the kernel units
// (ipm_wreg_{tab,da,pa,dapa,pc,pcda,pcpa,bd,bdpa}.hip), grid sizing and the wreg_launch_* entry points of wreg.h.  The only kernels
// compiled here are the two that have no table: the stand-alone LDL' solve and the selftest of the cross-lane primitives.
#include "wreg_wave.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// stand-alone LDL' solve of explicit dense symmetric matrices: the register factor + block substitution on their own
// (pycllp/ldl.py:202-239 solve_ldl; also the bring-up check of factor()/solve())
// ------------------------------------------------------------------------------------------------------------------
template <int MB>
__global__ void __launch_bounds__(256, 1)
ldl_solve_wreg_kernel(int n, long B, const double* __restrict__ Ag, const double* __restrict__ rhs, double* __restrict__ out,
                      double floor_, int* __restrict__ queue) {
    using G = WGeo<MB>;
    constexpr int MP = G::MP;
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, 1> w;
    USE_AGPR_FORM();
    const int tid = threadIdx.x;
    wreg_carve(w, (double*)lraw + (size_t)(tid >> 6) * G::WAVE_D(1), tid);
    const int &lane = w.lane, &q = w.q, &c16 = w.c16;
    long mat = next_item(queue, lane);
    while (mat < B) {
        const double* A = Ag + mat * (long)n * n;
        // off-diagonal blocks: U[K][I] register r = M[i = 16I + c16][k = 16K + 4r + q] (i > k); padded rows are zero
        static_for<0, MB>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
            static_for<K + 1, MB>([&](auto Ic) {
                constexpr int I = decltype(Ic)::value;
                double4_t blk;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = 16 * I + c16, k = 16 * K + 4 * r + q;
                    blk[r] = (i < n) ? A[(long)i * n + k] : 0.0;
                }
                park(w.P[G::bix(K, I)], blk);
            });
        });
        for (int i = lane; i < MP; i += 64) w.um_()[i] = (i < n) ? rhs[mat * n + i] : 0.0;
        // diagonal blocks into their slots: element [row][col], col <= row, of block K at K WL + row (row + 1) / 2 + col
        static_for<0, MB>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int il = 4 * r + q, row = 16 * K + il, col = 16 * K + c16;
                if (c16 <= il) w.wl_()[K * WL + il * (il + 1) / 2 + c16] = (row < n) ? A[(long)row * n + col] : ((row == col) ? 1.0 : 0.0);
            }
        });
        wave_lds_sync();
        STAMP_DECL
        (void)w.template factor<false>(1e300, floor_ STAMP_PASS);
        w.solve();
        for (int i = lane; i < n; i += 64) out[mat * n + i] = w.um_()[i];
        wave_lds_sync();
        mat = next_item(queue, lane);
    }
}

// ---- selftest of the cross-lane primitives (bring-up aid) --------------------------------------------------------
__global__ void wreg_selftest_kernel(double* out) {
    const int lane = threadIdx.x & 63;
    const double v = 1.0 + lane;
    out[lane] = quad_sum(v);                 // expect sum over l' = l mod 16 + 16 k
    out[64 + lane] = row_sum(v);             // expect sum over the 16-lane row
    out[128 + lane] = wsum(v);               // expect 2080
    out[192 + lane] = row_bcast<5>(v);       // expect 1 + (lane & ~15) + 5
    // MFMA layout: A[m][k] = 100 m + k (k = 0..3), B[k][n] = (k == 1) ? n + 1 : 0  ->  C[m][n] = (100 m + 1)(n + 1)
    const int c16 = lane & 15, qd = lane >> 4;
    const double a = 100.0 * c16 + qd, b = (qd == 1) ? c16 + 1.0 : 0.0;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    for (int r = 0; r < 4; r++) out[256 + 64 * r + lane] = acc[r];   // expect (100 (4r + q) + 1)(c16 + 1)
    out[512 + lane] = wmax(v);               // expect 64
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
struct WregPlan {
    WregTab tab;
    int mb, nq;
    bool da = false, pa = false;
    bool bd = false;      // the plan of the bounded kernel (wreg_plan_create_bounded): 2 NP more doubles per wave
    void* dev_blob;
};

namespace {

template <typename T>
size_t put(std::vector<char>& host, const std::vector<T>& v) {
    size_t off = (host.size() + 15) & ~(size_t)15;
    host.resize(off + v.size() * sizeof(T));
    if (!v.empty()) memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

}  // namespace

// the launcher table of a plan's kind; pc: its predictor-corrector kernels (plans of the bounded kernel have none)
static const WVariants& table_of(bool da, bool pa, bool bd, bool pc = false) {
    static const WVariants none = { nullptr, 0 };
    if (da && pa) return (bd || pc) ? none : kWDAPA;      // per-problem dense matrices: the plain kernel only
    if (bd) return pa ? kWBDPA : (da ? kWBDDA : kWBD);
    if (pc) return pa ? kWPCPA : (da ? kWPCDA : kWPC);
    return pa ? kWPA : (da ? kWDA : kWTab);
}

// the first variant of a table (ordered by cost) that covers (m, n), or null
static const WVariant* first_covering(const WVariants& t, int m, int n) {
    for (int i = 0; i < t.n; i++)
        if (m <= 16 * t.v[i].mb && n <= 64 * t.v[i].nq) return &t.v[i];
    return nullptr;
}

// Plan with A as a dense image in LDS (no tables): for matrices whose Gram term list does not fit -- dense A's, e.g. the LPs
// hip_dense_primal_normal hands over beyond m = 32.  The last m columns are kept out of the image when they are the
// identity (equality form of a StandardLP).  Fewer than four waves per workgroup when that is what lets the image fit.
// bd: the plan of the bounded kernel (its variants; t and s behind every wave area)
// dpa: the plan of the kernel on per-problem dense matrices (wreg_plan_create_dense_pa: an image per wave, no device copy);
// keep_tail (dpa only): an identity tail stays in the image
static int wreg_plan_create_dense(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                  bool bd, hipStream_t st, WregPlan** out, bool dpa = false, bool keep_tail = false) {
    const WVariant* v = first_covering(table_of(true, dpa, bd), m, n);
    if (!v) return 1;
    const int MB = v->mb, NQ = v->nq;
    const int MP = 16 * MB;
    // identity tail?
    bool sl = n > m && !keep_tail;
    std::vector<int> tail_cnt(sl ? m : 0, 0);
    for (int i = 0; i < m && sl; i++)
        for (int e = ptr[i]; e < ptr[i + 1]; e++)
            if (col[e] >= n - m) { if (col[e] != n - m + i || val[e] != 1.0) sl = false; else tail_cnt[i]++; }
    for (int i = 0; i < m && sl; i++) if (tail_cnt[i] != 1) sl = false;
    const int nd = sl ? n - m : n, ndp = ((std::max(nd, 1) + 15) / 16) * 16, AS = ndp + 1, R = ((m + 7) / 8) * 8;   // (16: gram_dense takes four k-steps per trip)
    WregPlan* P = new WregPlan();
    WregTab& T = P->tab;
    memset(&T, 0, sizeof(T));
    T.m = m; T.n = n; T.nnz = nnz; T.nd = nd; T.as = AS; T.img_rows = R;
    T.wave_doubles = stage_d(NQ) + 64 * NQ + 5 * MP + MB * WL + (bd ? 2 * 64 * NQ : 0);
    if (dpa) {
        // the image behind every wave area; nothing in front of the waves
        T.pa = 1;
        T.wave_doubles += R * AS;
        int wp = 0;
        for (int w = 4; w >= 1; w--)
            if (sizeof(double) * (size_t)w * T.wave_doubles <= (size_t)max_lds) { wp = w; break; }
        if (!wp) { delete P; return 1; }
        T.wpb = wp; T.o_img = 0; T.o_wave = 0;
        T.lds_bytes = (int)(sizeof(double) * (size_t)wp * T.wave_doubles);
        P->dev_blob = nullptr;
        P->mb = MB; P->nq = NQ; P->da = true; P->pa = true;
        *out = P;
        return 0;
    }
    const size_t img_bytes = sizeof(double) * (size_t)R * AS;
    int wpb = 0;
    for (int w = 4; w >= 1; w--)
        if (img_bytes + 16 + sizeof(double) * (size_t)w * T.wave_doubles <= (size_t)max_lds) { wpb = w; break; }
    if (!wpb) { delete P; return 1; }
    T.wpb = wpb; T.o_img = 0; T.o_wave = (int)((img_bytes + 15) & ~(size_t)15);
    T.lds_bytes = T.o_wave + (int)(sizeof(double) * (size_t)wpb * T.wave_doubles);
    std::vector<double> img((size_t)R * AS, 0.0);
    for (int i = 0; i < m; i++)
        for (int e = ptr[i]; e < ptr[i + 1]; e++)
            if (col[e] < nd) img[(size_t)i * AS + col[e]] = val[e];
    hipError_t e = hipMalloc(&P->dev_blob, img.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(P->dev_blob, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { if (P->dev_blob) (void)hipFree(P->dev_blob); delete P; return 1000 + (int)e; }
    T.img = (const double*)P->dev_blob;
    P->mb = MB; P->nq = NQ; P->da = true; P->bd = bd;
    *out = P;
    return 0;
}

static int wreg_plan_create_tables(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                   bool pa, bool bd, hipStream_t st, WregPlan** out);

int wreg_plan_create(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds, int pa,
                     hipStream_t st, WregPlan** out) {
    if (pa) return wreg_plan_create_tables(m, n, nnz, val, ptr, col, max_lds, true, false, st, out);
    const int rc = wreg_plan_create_tables(m, n, nnz, val, ptr, col, max_lds, false, false, st, out);
    if (rc != 1) return rc;
    return wreg_plan_create_dense(m, n, nnz, val, ptr, col, max_lds, false, st, out);
}

int wreg_plan_create_bounded(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                             hipStream_t st, WregPlan** out) {
    const int rc = wreg_plan_create_tables(m, n, nnz, val, ptr, col, max_lds, false, true, st, out);
    if (rc != 1) return rc;
    return wreg_plan_create_dense(m, n, nnz, val, ptr, col, max_lds, true, st, out);
}

int wreg_plan_create_dense_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                              int keep_tail, hipStream_t st, WregPlan** out) {
    return wreg_plan_create_dense(m, n, nnz, val, ptr, col, max_lds, false, st, out, true, keep_tail != 0);
}

int wreg_plan_create_bounded_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                hipStream_t st, WregPlan** out) {
    return wreg_plan_create_tables(m, n, nnz, val, ptr, col, max_lds, true, true, st, out);
}

// pa: the structure-only tables of the per-problem-A variants (the values `val` only stand in where a table still wants
// one; no kernel of those variants reads them).  bd: the plan of the bounded kernel (its variants; t and s behind every wave
// area, fewer waves per workgroup where that is what lets the tables fit)
static int wreg_plan_create_tables(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                   bool pa, bool bd, hipStream_t st, WregPlan** out) {
    const WVariant* v = first_covering(table_of(false, pa, bd), m, n);
    if (!v || nnz >= 65535) return 1;
    const int MB = v->mb, NQ = v->nq;
    const int MP = 16 * MB, MPL = 64 * ((MP + 63) / 64), NP = 64 * NQ;
    WregPlan* P = new WregPlan();
    WregTab& T = P->tab;
    memset(&T, 0, sizeof(T));
    T.m = m; T.n = n; T.nnz = nnz;
    // ---- column positions: the columns sorted by length (longest first) are dealt to positions 0, 1, ...; position p
    //      is element p % 64 of N-vector register p / 64, so every register holds 64 columns of similar length ----
    std::vector<int> cptr(n + 1, 0), crow(nnz), csc_src(nnz);
    std::vector<double> csc_val(nnz);
    for (int e = 0; e < nnz; e++) cptr[col[e] + 1]++;
    for (int j = 0; j < n; j++) cptr[j + 1] += cptr[j];
    {
        std::vector<int> fill(cptr.begin(), cptr.end() - 1);
        for (int i = 0; i < m; i++)
            for (int e = ptr[i]; e < ptr[i + 1]; e++) { const int p = fill[col[e]]++; crow[p] = i; csc_val[p] = val[e]; csc_src[p] = e; }
    }
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
            ec_val[(size_t)(T.meta[META_COFF + q] + t) * 64 + l] = csc_val[e];
            ec_row[(size_t)(T.meta[META_COFF + q] + t) * 64 + l] = (unsigned short)crow[e];
            ec_src[(size_t)(T.meta[META_COFF + q] + t) * 64 + l] = (unsigned short)csc_src[e];
        }
    }
    // ---- Gram entries (strictly lower triangle of M): off-diagonal blocks grouped by staging chunk (HB blocks of the
    //      linear block order each); the entries inside the diagonal blocks go to their slots in the W area, as part of
    //      the last chunk's group when that chunk ends in front of the W area, else as a group of their own.  All
    //      destinations are offsets from the start of the stage. ----
    struct Term { int group, dst, colj; double w; int ia, ib; };
    std::vector<Term> terms;
    const int nblk = MB * (MB - 1) / 2, nchunk = (nblk + HB - 1) / HB;
    const bool merge_diag = nblk > 0 && (nblk - HB * (nchunk - 1)) * 256 <= stage_d(NQ);      // = WGeo<MB>::MERGE_DIAG(NQ)
    const int diag_group = merge_diag ? nchunk - 1 : nchunk, ngroup = merge_diag ? nchunk : nchunk + 1;
    if (ngroup + 1 > META_N - META_SEG || stage_d(NQ) + MB * WL > 65535) { delete P; return 1; }
    for (int j = 0; j < n; j++)
        for (int a = cptr[j]; a < cptr[j + 1]; a++)
            for (int b2 = cptr[j]; b2 < a; b2++) {
                const int i = crow[a], k = crow[b2];   // rows ascend inside a column: i > k
                const int K = k / 16, I = i / 16, il = i % 16, kl = k % 16;
                if (I == K) {          // diagonal block K: element [il][kl] of the packed lower triangle in slot K
                    terms.push_back({diag_group, stage_d(NQ) + K * WL + il * (il + 1) / 2 + kl, posof[j], csc_val[a] * csc_val[b2], csc_src[a], csc_src[b2]});
                } else {               // block (K, I) of U: element [kl][il] of block bix % HB of chunk bix / HB
                    const int bx = K * MB - K * (K + 1) / 2 + (I - K - 1);
                    terms.push_back({bx / HB, (bx % HB) * 256 + kl * 16 + il, posof[j], csc_val[a] * csc_val[b2], csc_src[a], csc_src[b2]});
                }
                if (terms.size() > ((size_t)1 << 22)) { delete P; return 1; }
            }
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
    T.wave_doubles = stage_d(NQ) + 64 * NQ + 5 * MP + MB * WL + T.nnzp + (bd ? 2 * NP : 0);
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
        if (!(pa || bd) || wpb == 1) { delete P; return 1; }
        wpb--;
    }
    // ---- device copies ----
    std::vector<char> host;
    const size_t a1 = put(host, csr_val), a2 = put(host, ec_val), a3 = put(host, t_w), a4 = put(host, lev),
                 a5 = put(host, csr_col), a6 = put(host, csr_ptr), a7 = put(host, csr_len), a8 = put(host, ec_row),
                 a9 = put(host, colmap), a11 = put(host, t_cd), a12 = put(host, ec_src), a13 = put(host, t_ab);
    hipError_t e = hipMalloc(&P->dev_blob, host.size());
    if (e == hipSuccess) e = hipMemcpyAsync(P->dev_blob, host.data(), host.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { if (P->dev_blob) (void)hipFree(P->dev_blob); delete P; return 1000 + (int)e; }
    char* db = (char*)P->dev_blob;
    T.csr_val = (const double*)(db + a1); T.ec_val = (const double*)(db + a2); T.t_w = (const double*)(db + a3);
    T.lev = (const int*)(db + a4);
    T.csr_col = (const unsigned short*)(db + a5); T.csr_ptr = (const unsigned short*)(db + a6);
    T.csr_len = (const unsigned short*)(db + a7); T.ec_row = (const unsigned short*)(db + a8);
    T.colmap = (const unsigned*)(db + a9);
    T.t_cd = (const unsigned*)(db + a11);
    T.ec_src = (const unsigned short*)(db + a12); T.t_ab = (const unsigned*)(db + a13);
    P->mb = MB; P->nq = NQ; P->pa = pa; P->bd = bd; T.wpb = wpb;
    *out = P;
    return 0;
}

void wreg_plan_free(WregPlan* p) {
    if (!p) return;
    if (p->dev_blob) (void)hipFree(p->dev_blob);
    delete p;
}

int wreg_lds_bytes(const WregPlan* p) { return p ? p->tab.lds_bytes : 0; }
int wreg_block_threads(const WregPlan* p) { return p ? 64 * p->tab.wpb : 0; }
int wreg_variant(const WregPlan* p) { return p ? (p->da ? 2 : 1) : 0; }
int wreg_image_cols(const WregPlan* p) { return (p && p->da) ? p->tab.nd : 0; }
void wreg_shape(const WregPlan* p, int* mb, int* nq) {
    if (mb) *mb = p ? p->mb : 0;
    if (nq) *nq = p ? p->nq : 0;
}
int wreg_has_predcorr(const WregPlan* p) { return p ? 1 : 0; }

// the launchers of the plan's (MB, NQ) among the plain (pc: predictor-corrector, bd: bounded) kernels of its kind, or null
static const WVariant* plan_launchers(const WregPlan* p, bool bd, bool pc = false) {
    if (!p || p->bd != bd) return nullptr;
    const WVariants& t = table_of(p->da, p->pa, p->bd, pc);
    for (int i = 0; i < t.n; i++)
        if (t.v[i].mb == p->mb && t.v[i].nq == p->nq) return &t.v[i];
    return nullptr;
}

// persistent grid of the solve kernels: one workgroup per CU left to the solve; the m <= 64 variants need fewer than half the
// registers (234 of 512 per lane): two workgroups per CU -- two waves per SIMD -- where the LDS allows it
static int solve_grid(const WregPlan* p, long B, const DevOpts& o, int num_cu) {
    long cus = (long)num_cu - o.reserve_cus > 0 ? (long)num_cu - o.reserve_cus : 1;
    if (p->mb <= 4 && 2 * (long)p->tab.lds_bytes <= 160 * 1024 && p->tab.wpb == 4) cus *= 2;
    const long grid = std::min(cus, (B + p->tab.wpb - 1) / p->tab.wpb);
    return grid < 1 ? 1 : (int)grid;
}

hipError_t wreg_launch_solve(WregPlan* p, long B, const double* a_batch, const double* b, const double* c, double* x, double* y, double* z,
                             double* pobj, double* dobj, int* status, int* iters, int* qhead, int* defer, DevOpts o,
                             int num_cu, hipStream_t st, int* grid_out) {
    const WVariant* v = plan_launchers(p, false);
    if (!v || (p->pa != (a_batch != nullptr))) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(defer, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    const int grid = solve_grid(p, B, o, num_cu);
    if (grid_out) *grid_out = grid;
    wsolve_fn fn = (o.flags & PYCLLP_FLAG_HSD) ? v->solve_hsd : v->solve;
    if ((o.flags & PYCLLP_FLAG_PREDCORR) && !(o.flags & PYCLLP_FLAG_HSD)) {
        const WVariant* pc = plan_launchers(p, false, true);
        if (!pc) return hipErrorNotSupported;
        fn = pc->solve;
    }
    if (!fn) return hipErrorNotSupported;      // (a kind without that kernel: per-problem dense matrices have the plain one only)
    return fn(p->tab, B, a_batch, b, c, x, y, z, pobj, dobj, status, iters, qhead, defer, o, grid, st);
}

hipError_t wreg_launch_solve_bounded(WregPlan* p, long B, const double* a_batch, const double* b, const double* c, const double* u, double* x, double* y,
                                     double* z, double* s, double* pobj, double* dobj, int* status, int* iters, int* qhead,
                                     DevOpts o, int num_cu, hipStream_t st, int* grid_out) {
    const WVariant* v = plan_launchers(p, true);
    if (!v || (p->pa != (a_batch != nullptr))) return hipErrorInvalidValue;
    const int grid = solve_grid(p, B, o, num_cu);
    if (grid_out) *grid_out = grid;
    if (a_batch) return v->solve_bounded_pa(p->tab, B, a_batch, b, c, u, x, y, z, s, pobj, dobj, status, iters, qhead, o, grid, st);
    return v->solve_bounded(p->tab, B, b, c, u, x, y, z, s, pobj, dobj, status, iters, qhead, o, grid, st);
}

hipError_t wreg_launch_newton(WregPlan* p, long B, const double* x, const double* z, const double* y, const double* b,
                              const double* c, double mu, double* dy, int* nref, DevOpts o, int num_cu, hipStream_t st,
                              int* grid_out) {
    const WVariant* v = plan_launchers(p, false);
    if (!v || !v->newton) return hipErrorInvalidValue;
    int* qhead = nullptr;
    hipError_t e = hipMallocAsync((void**)&qhead, sizeof(int), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(qhead, 0, sizeof(int), st);
    long grid = std::min((long)num_cu, (B + p->tab.wpb - 1) / p->tab.wpb);
    if (grid < 1) grid = 1;
    if (grid_out) *grid_out = (int)grid;
    if (e == hipSuccess) e = v->newton(p->tab, B, x, z, y, b, c, mu, dy, nref, qhead, o, (int)grid, st);
    hipError_t e2 = hipFreeAsync(qhead, st);
    return e != hipSuccess ? e : e2;
}

hipError_t wreg_launch_ldl_solve(int n, long B, const double* A, const double* rhs, double* out, double floor_,
                                 int num_cu, hipStream_t st) {
    if (n > 128) return hipErrorInvalidValue;
    int* qhead = nullptr;
    hipError_t e = hipMallocAsync((void**)&qhead, sizeof(int), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(qhead, 0, sizeof(int), st);
    long grid = std::min((long)num_cu, (B + 3) / 4);
    if (grid < 1) grid = 1;
    const int lds = (int)(sizeof(double) * 4 * WGeo<8>::WAVE_D(1));
    if (e == hipSuccess) e = set_dyn_lds((const void*)ldl_solve_wreg_kernel<8>, lds);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((ldl_solve_wreg_kernel<8>), dim3((unsigned)grid), dim3(256), lds, st, n, B, A, rhs, out, floor_, qhead);
        e = hipGetLastError();
    }
    hipError_t e2 = hipFreeAsync(qhead, st);
    return e != hipSuccess ? e : e2;
}

extern "C" int pycllp_hip_debug_wreg_selftest(double* out_dev, void* stream) {
    hipLaunchKernelGGL(wreg_selftest_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out_dev);
    return (int)hipGetLastError();
}
