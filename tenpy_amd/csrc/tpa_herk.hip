// K1h: grouped + chained WEIGHTED Hermitian rank-k update on fp64 MFMA (v_mfma_f64_16x16x4_f64), gfx950.
//
//        C_t (m x n, row stride ldc)  =  [C_t +]  sum_{l in chain(t)} sum_kk  s_l(kk) A_l(i, kk) conj(B_l(j, kk))
//
// The contraction in the middle of the density-matrix mixer (reference DensityMatrixMixer.mix_rho, mps_common.py:2002-2026:
// rho = X diag(mix) X^dagger per charge sector).  Same work decomposition and k loop as gemm_chain_kernel (tpa_gemm.hip): one workgroup
// per 64 x 64 tile of one C block, 4 waves (2 x 2), a wave owns 2 x 2 MFMA tiles, operands staged global -> registers -> LDS with a
// register prefetch that runs across link boundaries.  What is different:
//  * both operands are indexed (row, k) and staged the same way; B is conjugated (complex data) by the sign of its imaginary plane;
//  * the real weight s_l(kk) is fetched with the prefetch and multiplied into A when A is written to LDS: one multiply per staged
//    element, none in the MFMA loop;
//  * a Hermitian task is given only the tiles on or below the diagonal of its tile grid; the epilogue writes C[i, j] (i >= j) and
//    the mirror C[j, i] = conj(C[i, j]) from the same accumulator, and Im C[i, i] = 0;
//  * a general task writes its rectangle and (mirror_off >= 0) the conjugate transpose at the mirror offset.
// A diagonal tile stages its operand twice (as A and as B): staging it once would save one of two global reads on T of T (T + 1) / 2
// tiles and has not been measured.
#include "tpa_common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

namespace {

struct HLink {  // int64[12]
    int64_t a_off, b_off, k, a_rs, a_ks, b_rs, b_ks, w_off, w_len, w_inner, pad0, pad1;
};
struct HTask {  // int64[10]
    int64_t c_off, m, n, ldc, link_begin, link_count, accumulate, herm, mirror_off, mirror_ldc;
};

template <bool CPLX>
struct HCfg {
    static constexpr int BT = 64, BK = 16, TM = 2, TN = 2;
    static constexpr int WM = BT / (TM * 16), WN = BT / (TN * 16), NT = WM * WN * 64;
    static constexpr int PAD = 16;
    // LDS doubles per plane of one operand: max over the two layouts ([row][BK + 1] for k-fast data, [k][BT + PAD] for row-fast data)
    static constexpr int OP_LDS = (BT * (BK + 1) > BK * (BT + PAD)) ? BT * (BK + 1) : BK * (BT + PAD);
    static constexpr int PLANES = CPLX ? 2 : 1;
    static constexpr int EO = BT * BK / NT;  // elements of one operand staged per thread per k-tile
    static_assert(NT % BK == 0 && NT % BT == 0, "staging offsets must be affine in the element index");
};

template <bool CPLX>
__global__ __launch_bounds__((HCfg<CPLX>::NT)) void herk_chain_kernel(
    const HTask *__restrict__ tasks, const HLink *__restrict__ links, const int4 *__restrict__ tiles,
    const double *__restrict__ Abase, const double *__restrict__ Bbase, const double *__restrict__ wvec, double *__restrict__ Cbase) {
    using C = HCfg<CPLX>;
    constexpr int NT = C::NT, EO = C::EO, PL = C::PLANES, BK = C::BK, BT = C::BT, TM = C::TM, TN = C::TN;
    constexpr int ES = CPLX ? 2 : 1;  // doubles per element
    __shared__ double lds[2 * PL * C::OP_LDS];
    double *As = lds;
    double *Bs = lds + PL * C::OP_LDS;

    const int4 tile = tiles[blockIdx.x];
    const HTask tk = tasks[tile.x];
    const bool herm = tk.herm != 0;
    if (herm && tile.y < tile.z) return;      // (workgroup-uniform) a Hermitian task is covered by its lower tiles
    const int m = (int)tk.m, n = (int)tk.n;
    const int row0 = tile.y * BT, col0 = tile.z * BT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / C::WN, wc = wave % C::WN;
    const int l15 = lane & 15, l4 = lane >> 4;

    d4 acc[PL][TM][TN];
#pragma unroll
    for (int p = 0; p < PL; ++p)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[p][i][j] = d4{0, 0, 0, 0};

    const int nl = (int)tk.link_count;
    const HLink *lk = links + tk.link_begin;

    // what a thread needs to stage its share of one k-tile of one operand of one link: element r of the thread sits at
    // (global) p + r * gstep, (LDS) lbase + r * lstep; its k index inside the tile is kk0 + r * kkstep, its row i0 + r * istep
    struct Stage {
        const double *p;      // advances by kstep per k-tile
        int64_t gstep, kstep;
        int lbase, lstep, kk0, kkstep, i0, istep, lim;
    };
    struct LinkView {
        Stage a, b;
        int K, sa_i, sa_k, sb_j, sb_k;
        int w_len, w_inner;
        const double *w;      // NULL: weight 1
    };
    auto open_operand = [&](Stage &s, int &s_i, int &s_k, const double *base, int64_t off, int64_t rs, int64_t ks, int first, int lim) {
        const bool kfast = (ks == 1) && (rs != 1);
        s_i = kfast ? (BK + 1) : 1;
        s_k = kfast ? 1 : (BT + C::PAD);
        // element e = tid + r NT;  k-fast: (i, kk) = (e / BK, e % BK);  else (e % BT, e / BT)
        const int i = kfast ? (tid / BK) : (tid % BT), kk = kfast ? (tid % BK) : (tid / BT);
        const int di = kfast ? (NT / BK) : 0, dk = kfast ? 0 : (NT / BT);
        s.p = base + ES * (off + (int64_t)(first + i) * rs + (int64_t)kk * ks);
        s.gstep = ES * ((int64_t)di * rs + (int64_t)dk * ks);
        s.kstep = ES * (int64_t)BK * ks;
        s.lbase = i * s_i + kk * s_k;
        s.lstep = di * s_i + dk * s_k;
        s.kk0 = kk;
        s.kkstep = dk;
        s.i0 = first + i;
        s.istep = di;
        s.lim = lim;
    };
    auto open_link = [&](int li, LinkView &v) {
        const HLink L = lk[li];
        v.K = (int)L.k;
        v.w = (L.w_off < 0) ? nullptr : wvec + L.w_off;
        v.w_len = max(1, (int)L.w_len);
        v.w_inner = max(1, (int)L.w_inner);
        open_operand(v.a, v.sa_i, v.sa_k, Abase, L.a_off, L.a_rs, L.a_ks, row0, m);
        open_operand(v.b, v.sb_j, v.sb_k, Bbase, L.b_off, L.b_rs, L.b_ks, col0, n);
    };
    double ra[PL][EO], rb[PL][EO], rw[EO];
    auto load_operand = [&](Stage &s, double (&reg)[PL][EO], int krem, double sgn) {
        const bool full = (krem >= BK);
#pragma unroll
        for (int r = 0; r < EO; ++r) {
            const bool ok = (s.i0 + r * s.istep < s.lim) && (full || s.kk0 + r * s.kkstep < krem);
            const double *q = s.p + r * s.gstep;
            if (CPLX) {
                double2 x = ok ? *reinterpret_cast<const double2 *>(q) : double2{0, 0};
                reg[0][r] = x.x;
                reg[PL - 1][r] = sgn * x.y;
            } else {
                reg[0][r] = ok ? *q : 0.0;
            }
        }
        s.p += s.kstep;
    };
    auto load_tile = [&](LinkView &v, int k0) {      // registers <- k-tile k0 of link v (and the weights of A's elements); advances the pointers
        load_operand(v.a, ra, v.K - k0, 1.0);
        load_operand(v.b, rb, v.K - k0, -1.0);       // conj(B)
        if (v.w == nullptr) {
#pragma unroll
            for (int r = 0; r < EO; ++r) rw[r] = 1.0;
        } else if (v.w_len == 1) {                   // a scalar weight per link: the common case of 1-wide MPO bond blocks
            const double s = v.w[0];
#pragma unroll
            for (int r = 0; r < EO; ++r) rw[r] = s;
        } else {                                     // the index is inside [0, w_len) for every kk, also beyond K
#pragma unroll
            for (int r = 0; r < EO; ++r) rw[r] = v.w[((k0 + v.a.kk0 + r * v.a.kkstep) / v.w_inner) % v.w_len];
        }
    };
    auto store_tile = [&](const LinkView &v) {       // registers -> LDS in link v's layouts; A is weighted here
#pragma unroll
        for (int r = 0; r < EO; ++r)
#pragma unroll
            for (int p = 0; p < PL; ++p) As[p * C::OP_LDS + v.a.lbase + r * v.a.lstep] = rw[r] * ra[p][r];
#pragma unroll
        for (int r = 0; r < EO; ++r)
#pragma unroll
            for (int p = 0; p < PL; ++p) Bs[p * C::OP_LDS + v.b.lbase + r * v.b.lstep] = rb[p][r];
    };
    auto mma_tile = [&](const double *Aw, const double *Bw, int sa_i, int sa_k, int sb_j, int sb_k) {
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            double a[PL][TM], b[PL][TN];
#pragma unroll
            for (int p = 0; p < PL; ++p) {
#pragma unroll
                for (int i = 0; i < TM; ++i) a[p][i] = Aw[p * C::OP_LDS + i * 16 * sa_i + ks * 4 * sa_k];
#pragma unroll
                for (int j = 0; j < TN; ++j) b[p][j] = Bw[p * C::OP_LDS + j * 16 * sb_j + ks * 4 * sb_k];
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (CPLX) {
                        acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][i], b[0][j], acc[0][i][j], 0, 0, 0);
                        acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[PL - 1][i], b[PL - 1][j], acc[0][i][j], 0, 0, 0);
                        acc[PL - 1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][i], b[PL - 1][j], acc[PL - 1][i][j], 0, 0, 0);
                        acc[PL - 1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[PL - 1][i], b[0][j], acc[PL - 1][i][j], 0, 0, 0);
                    } else {
                        acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][i], b[0][j], acc[0][i][j], 0, 0, 0);
                    }
                }
        }
    };

    int li = 0;
    while (li < nl && lk[li].k <= 0) ++li;
    if (li < nl) {
        LinkView cur, nxt;
        open_link(li, cur);
        load_tile(cur, 0);
        while (true) {
            // the next non-empty link is opened BEFORE the k loop of this one: the last k-tile of this link prefetches the first
            // k-tile of the next (no drained load pipeline at a link boundary)
            int lj = li + 1;
            while (lj < nl && lk[lj].k <= 0) ++lj;
            const bool has_next = lj < nl;
            if (has_next) open_link(lj, nxt);
            const int K = cur.K;
            const int sa_i = cur.sa_i, sa_k = cur.sa_k, sb_j = cur.sb_j, sb_k = cur.sb_k;
            const int fa = (wr * TM * 16 + l15) * sa_i + l4 * sa_k, fb = (wc * TN * 16 + l15) * sb_j + l4 * sb_k;
            for (int k0 = 0; k0 < K; k0 += BK) {
                store_tile(cur);
                __syncthreads();
                if (k0 + BK < K)
                    load_tile(cur, k0 + BK);      // prefetch the next k-tile into registers
                else if (has_next)
                    load_tile(nxt, 0);            // ... or the first k-tile of the next link
                mma_tile(As + fa, Bs + fb, sa_i, sa_k, sb_j, sb_k);
                __syncthreads();
            }
            if (!has_next) break;
            cur = nxt;
            li = lj;
        }
    }

    // ---- epilogue: C/D layout of v_mfma_f64_16x16x4_f64: col = lane&15, row = (lane>>4) + 4*reg.  Every element is stored by
    //      exactly one thread, the mirror from the same registers: ordinary vector stores only.
    double *Cp = Cbase + ES * tk.c_off;
    const bool accum = tk.accumulate != 0;
    const bool diag = herm && tile.y == tile.z;
    const bool mirror = herm || tk.mirror_off >= 0;
    double *Mp = herm ? Cp : Cbase + ES * tk.mirror_off;
    const int64_t mld = herm ? tk.ldc : tk.mirror_ldc;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + wr * TM * 16 + i * 16 + l4 + 4 * r;
                const int col = col0 + wc * TN * 16 + j * 16 + l15;
                if (row < m && col < n && !(diag && row < col)) {
                    const int64_t g = (int64_t)row * tk.ldc + col;
                    const int64_t gm = (int64_t)col * mld + row;
                    const bool on_diag = herm && row == col;
                    if (CPLX) {
                        double2 v{acc[0][i][j][r], acc[PL - 1][i][j][r]};
                        double2 *dst = reinterpret_cast<double2 *>(Cp + 2 * g);
                        if (accum) {
                            double2 o = *dst;
                            v.x += o.x;
                            v.y += o.y;
                        }
                        if (on_diag) v.y = 0.0;
                        *dst = v;
                        if (mirror && !on_diag) *reinterpret_cast<double2 *>(Mp + 2 * gm) = double2{v.x, -v.y};
                    } else {
                        double v = acc[0][i][j][r];
                        if (accum) v += Cp[g];
                        Cp[g] = v;
                        if (mirror && !on_diag) Mp[gm] = v;
                    }
                }
            }
}

}  // namespace

extern "C" int tpa_herk_tile_shape(int dtype, int *bt) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(bt != nullptr);
    *bt = (dtype == TPA_F64) ? HCfg<false>::BT : HCfg<true>::BT;
    return 0;
}

extern "C" int tpa_herk_chain(int dtype, const int64_t *tasks_dev, const int64_t *links_dev, const int32_t *tiles_dev, int n_tiles,
                              const void *Abase, const void *Bbase, const double *wvec_dev, void *Cbase, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_tiles <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        herk_chain_kernel<false><<<n_tiles, HCfg<false>::NT, 0, st>>>((const HTask *)tasks_dev, (const HLink *)links_dev, (const int4 *)tiles_dev,
                                                                     (const double *)Abase, (const double *)Bbase, wvec_dev, (double *)Cbase);
    else
        herk_chain_kernel<true><<<n_tiles, HCfg<true>::NT, 0, st>>>((const HTask *)tasks_dev, (const HLink *)links_dev, (const int4 *)tiles_dev,
                                                                   (const double *)Abase, (const double *)Bbase, wvec_dev, (double *)Cbase);
    TPA_LAUNCH_CHECK();
    return 0;
}
