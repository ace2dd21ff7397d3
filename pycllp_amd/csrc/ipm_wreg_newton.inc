// ipm_wreg_newton.inc -- the stand-alone Newton step of the wavefront-per-LP family, on wreg_wave.h
namespace {

// ------------------------------------------------------------------------------------------------------------------
// stand-alone Newton step: sparse_solve_primal_normal (ldl.cl:656-712) as launched by the reference's
// tests/test_ldl.py:276-361, one state per wavefront
// ------------------------------------------------------------------------------------------------------------------
template <int MB, int NQ, bool DA>
__global__ void __launch_bounds__(256, 1)
newton_wreg_kernel(WregTab T, long B, const double* __restrict__ xg, const double* __restrict__ zg,
                   const double* __restrict__ yg, const double* __restrict__ bg, const double* __restrict__ cg, double mu,
                   double* __restrict__ dyg, int* __restrict__ nrefg, int* __restrict__ queue, DevOpts o) {
    using G = WGeo<MB>;
    constexpr int MR = G::MR, MP = G::MP;
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, NQ, DA> w;
    USE_AGPR_FORM();
    wreg_setup(w, T, lraw, threadIdx.x);
    const int& lane = w.lane; const int m = w.m, n = w.n;
    double* vx = w.stage_();
    bool okc[NQ], okr[MR];
    w.masks(okc, okr);
    long lp = next_item(queue, lane);
    while (lp < B) {
        double x[NQ], z[NQ], t[NQ], v[NQ];
        double b2 = 0.0;
#pragma unroll
        for (int r2 = 0; r2 < MR; r2++) {
            const int i = lane + 64 * r2;
            const double bi = okr[r2] ? bg[lp * m + i] : 0.0;
            b2 = fma(bi, bi, b2);
            if (i < MP) { w.bs_()[i] = bi; w.ys_()[i] = okr[r2] ? yg[lp * m + i] : 0.0; }
        }
        wave_lds_sync();
        const double etol = o.refine_tol * (1.0 + sqrt(wsum(b2)));
        w.At(w.ys_(), v);
#pragma unroll
        for (int qq = 0; qq < NQ; qq++) {
            const int j = lane + 64 * qq;
            const unsigned jo = w.coff(qq);
            x[qq] = okc[qq] ? buf_ld(row_rsrc(xg + lp * n, n), jo) : 1.0;
            z[qq] = okc[qq] ? buf_ld(row_rsrc(zg + lp * n, n), jo) : 1.0;
            const double cj = buf_ld(row_rsrc(cg + lp * n, n), jo);
            t[qq] = okc[qq] ? cj - v[qq] + mu * fast_rcp(x[qq]) : 0.0;
            vx[j] = okc[qq] ? x[qq] : 0.0;
            w.vd_()[j] = okc[qq] ? x[qq] * fast_rcp(z[qq]) : 0.0;
        }
        wave_lds_sync();
        double rho[MR], Ax[MR], Adt[MR], Md[MR];
        w.template Arow<false>(vx, Ax, Md);
        wave_lds_sync();
#pragma unroll
        for (int qq = 0; qq < NQ; qq++) vx[lane + 64 * qq] = w.vd_()[lane + 64 * qq] * t[qq];
        wave_lds_sync();
        w.template Arow<true>(vx, Adt, Md);
        double bmax = 0.0;
#pragma unroll
        for (int r2 = 0; r2 < MR; r2++) {
            const int i = lane + 64 * r2;
            rho[r2] = okr[r2] ? w.bs_()[i] - Ax[r2] : 0.0;
            if (i < MP) w.um_()[i] = okr[r2] ? Adt[r2] - rho[r2] : 0.0;
            bmax = fmax(bmax, okr[r2] ? fabs(Md[r2]) : 0.0);
        }
        const double beta2 = wmax(bmax);
        wave_lds_sync();
        w.gram(Md);
#pragma unroll
        for (int qq = 0; qq < NQ; qq++) w.stage_()[lane + 64 * qq] = t[qq];
        STAMP_DECL
        (void)w.template factor<false>(beta2, o.pivot_floor STAMP_PASS);
        double dy[MR], wv[NQ], dx[NQ];
        bool bad;
        double ed[MR];
        const int nref = newton_solve<false>(w, okc, okr, rho, etol, o.max_refine, mu, dy, dx, wv, ed, bad, nullptr STAMP_PASS);
#pragma unroll
        for (int r2 = 0; r2 < MR; r2++) if (okr[r2]) dyg[lp * m + lane + 64 * r2] = dy[r2];
        if (nrefg && lane == 0) nrefg[lp] = nref;
        wave_lds_sync();
        lp = next_item(queue, lane);
    }
}

}  // namespace
