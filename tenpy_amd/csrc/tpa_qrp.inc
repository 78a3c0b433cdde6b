// Householder family of tpa_svd.hip: pivoted QR, compact-WY trailing update, blocked application of Q (included by tpa_svd.hip
// before tpa_qr_la.inc).  Drivers: `svd_run_qrp` (rank-revealing preconditioner of tpa_svd_batch) and `qr_run_wy` (blocked
// tpa_qr_batch).  Every kernel but the panel factorisation is ONE template on the scalar type T = double or cd; the two
// panel kernels (`qrp_panel_kernel`, `qrp_panel_kernel_c`) are different algorithms and stay separate.
//
// ===================================================================================================
// Rank-revealing preconditioner: Householder QR with column pivoting (BLAS-2, batched over the charge blocks).
//
// DMRG wave-function blocks are numerically rank deficient (rank <= chi of d*chi; measured sigma from 1 down
// to 1e-27 with a cliff) and strongly graded.  Plain one-sided Jacobi then needs ~25 sweeps over ALL rows.
// With X P = Q [R; 0] (X = A or A^T, tall M x N) the Jacobi iteration only has to diagonalise the r x N factor
// R (r = numerical rank): ~7 sweeps over ~half the rows (numpy experiment on real theta blocks: 25 -> 7 sweeps).
//     X = (Q_r U_R) Sigma (VH_R P^T),   SVD(R) = U_R Sigma VH_R  by the block-Jacobi kernels above.
// Per step k two launches for all blocks together: `qrp_pivot_kernel` (one workgroup per block: pivot search on
// the exact residual column norms, column swap, Householder vector; X is kept column-major so that this is coalesced) and `qrp_update_kernel` (column tiles: rank-1
// update of the trailing matrix and exact recomputation of the residual norms in the same pass).
//
// Complex data (interleaved double2 storage), same structure:
//   X = A (m >= n) or A^H (m < n), column-major;   X P = Q [R; 0],   H = I - tau v v^H (LAPACK zlarfg: beta real),
//   the factorisation applies H^H from the left, blocks H_0 .. H_{l-1} = I - V T V^H (zlarft, forward / columnwise).
//   A = X:    U = Q_r U_R,          VH[jj][cperm[c]] = VH_R[jj][c]
//   A = X^H:  U[cperm[c]][jj] = conj(VH_R[jj][c]),   VH[jj][c] = conj((Q_r U_R)[c][jj])
// Complex products on the matrix cores are 4 real MFMAs on the (re, im) planes of the fragments.
struct QrpJob {  // int64[8]
    int64_t x_off, M, N, c_off, tr, r_off, pad0, pad1;   // c_off: offset into cn / tau / cperm ; tr: X = A^T
};
struct QrpState {  // per job
    int rank, done, nbk, last;   // nbk: size of the current panel; last: that panel was the final one
};

typedef double2 cd;
__device__ __forceinline__ cd c_mul(cd a, cd b) { return cd{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd c_mulc(cd a, cd b) { return cd{a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x}; }   // conj(a) * b
__device__ __forceinline__ cd c_fma(cd a, cd b, cd acc) { return cd{acc.x + a.x * b.x - a.y * b.y, acc.y + a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd c_fmac(cd a, cd b, cd acc) { return cd{acc.x + a.x * b.x + a.y * b.y, acc.y + a.x * b.y - a.y * b.x}; }  // acc + conj(a) b

// ---- scalar layer: what the templated kernels need from T.  Acc is the MFMA accumulator of a 16 x 16 tile: one d4 for real
//      data, the (re, im) planes for complex data; mfma<CONJ> adds a * b (CONJ: conj(a) * b) to it.  Zero is written T(0.0) in
//      the kernels: a literal for double, (0, 0) for cd.
template <class T>
struct Sc;
template <>
struct Sc<double> {
    static constexpr bool cplx = false;
    typedef d4 Acc;
    static __device__ __forceinline__ double conj(double a) { return a; }
    static __device__ __forceinline__ double neg(double a) { return -a; }
    static __device__ __forceinline__ double abs2(double v, double acc) { return ::fma(v, v, acc); }      // acc + |v|^2
    static __device__ __forceinline__ double nmul(double a, double b) { return -a * b; }      // -(a b)
    static __device__ __forceinline__ double fma(double a, double b, double acc) { return ::fma(a, b, acc); }
    static __device__ __forceinline__ double fmac(double a, double b, double acc) { return ::fma(a, b, acc); }   // acc + conj(a) b
    static __device__ __forceinline__ double get(const Acc &c, int reg) { return c[reg]; }
    static __device__ __forceinline__ void set(Acc &c, int reg, double v) { c[reg] = v; }
    template <bool CONJ>
    static __device__ __forceinline__ void mfma(double a, double b, Acc &c) {
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
};
template <>
struct Sc<cd> {
    static constexpr bool cplx = true;
    struct Acc {
        d4 r, i;
    };
    static __device__ __forceinline__ cd conj(cd a) { return cd{a.x, -a.y}; }
    static __device__ __forceinline__ cd neg(cd a) { return cd{-a.x, -a.y}; }
    static __device__ __forceinline__ double abs2(cd v, double acc) { return ::fma(v.x, v.x, ::fma(v.y, v.y, acc)); }
    static __device__ __forceinline__ cd nmul(cd a, cd b) { return neg(c_mul(a, b)); }
    static __device__ __forceinline__ cd fma(cd a, cd b, cd acc) { return c_fma(a, b, acc); }
    static __device__ __forceinline__ cd fmac(cd a, cd b, cd acc) { return c_fmac(a, b, acc); }
    static __device__ __forceinline__ cd get(const Acc &c, int reg) { return cd{c.r[reg], c.i[reg]}; }
    static __device__ __forceinline__ void set(Acc &c, int reg, cd v) {
        c.r[reg] = v.x;
        c.i[reg] = v.y;
    }
    template <bool CONJ>
    static __device__ __forceinline__ void mfma(cd a, cd b, Acc &c) {      // 4 real MFMAs on the (re, im) planes
        c.r = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, c.r, 0, 0, 0);
        c.r = __builtin_amdgcn_mfma_f64_16x16x4f64(CONJ ? a.y : -a.y, b.y, c.r, 0, 0, 0);
        c.i = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, c.i, 0, 0, 0);
        c.i = __builtin_amdgcn_mfma_f64_16x16x4f64(CONJ ? -a.y : a.y, b.x, c.i, 0, 0, 0);
    }
};

template <class T>
__global__ __launch_bounds__(NT) void qrp_init_kernel(const QrpJob *__restrict__ jobs, const SvdJob *__restrict__ sj,
                                                      const T *__restrict__ A, T *__restrict__ X,
                                                      double *__restrict__ cn, int64_t *__restrict__ cperm,
                                                      QrpState *__restrict__ state) {
    // grid (column tiles of 64, jobs): X = A or A^H stored COLUMN-major (X[j*M + i]), exact column norms^2,
    // identity permutation.  Wave w owns the columns j0 + 16 w .. +15 of the tile, lanes run along the rows
    // (contiguous in X); for X = A the 64 x 64 tile is transposed through LDS so that both sides stay coalesced.
    constexpr bool CX = Sc<T>::cplx;
    __shared__ double tre[64][65], tim[CX ? 64 : 1][65];      // (re, im) planes; real data never touches tim, which then takes no LDS
    const QrpJob J = jobs[blockIdx.y];
    const SvdJob S = sj[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    if (j0 >= J.N) return;
    double acc[16];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0;
    for (int64_t i0 = 0; i0 < J.M; i0 += 64) {
        if (!J.tr) {
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int64_t i = i0 + wave * 16 + rr, j = j0 + lane;
                const T v = (i < J.M && j < J.N) ? A[S.a_off + i * S.n + j] : T(0.0);
                if constexpr (CX) {
                    tre[wave * 16 + rr][lane] = v.x;
                    tim[wave * 16 + rr][lane] = v.y;
                } else
                    tre[wave * 16 + rr][lane] = v;
            }
            __syncthreads();
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int64_t j = j0 + wave * 16 + rr, i = i0 + lane;
            if (j < J.N && i < J.M) {
                T v;
                if constexpr (CX) {
                    if (J.tr)          // X = A^H:  X[i][j] = conj(A[j][i])
                        v = Sc<T>::conj(A[S.a_off + j * S.n + i]);
                    else
                        v = cd{tre[lane][wave * 16 + rr], tim[lane][wave * 16 + rr]};
                } else
                    v = J.tr ? A[S.a_off + j * S.n + i] : tre[lane][wave * 16 + rr];
                X[J.x_off + j * J.M + i] = v;
                acc[rr] = Sc<T>::abs2(v, acc[rr]);
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const double t = wave_sum(acc[rr]);
        const int64_t j = j0 + wave * 16 + rr;
        if (lane == 0 && j < J.N) {
            cn[J.c_off + j] = t;
            cperm[J.c_off + j] = j;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) state[blockIdx.y] = QrpState{0, 0, 0, 0};
}

constexpr int NTP_MAX = 256;   // threads of the panel kernel: 64 (one wavefront, no cross-wave barriers) or 256
constexpr int PNB = 8;    // pivot columns factorised per launch (panel pivoting: the PNB largest residual columns)
constexpr int RPT_MAX = 32;  // rows / candidate columns per thread held in registers (template RPT = 8, 16, 32)  ->  max(m, n) <= 8192

// sum the values v[q], q < n or q == extra, over the workgroup (NTP threads); results valid in every thread.  The callers
// sit in fully unrolled loops, so n / extra are constants after unrolling and the unused entries cost nothing.
template <int NTP, int K>
__device__ __forceinline__ void block_sum_vec(double (&v)[K], double (*red)[PNB + 1], int n, int extra) {
#pragma unroll
    for (int q = 0; q < K; ++q)
        if (q < n || q == extra) v[q] = wave_sum(v[q]);
    if (NTP == 64) return;   // a single wavefront: wave_sum already left the total in every lane
    lds_barrier();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (q < n || q == extra) red[threadIdx.x >> 6][q] = v[q];
    }
    lds_barrier();
#pragma unroll
    for (int q = 0; q < K; ++q)
        if (q < n || q == extra) {
            double t = 0;
#pragma unroll
            for (int w = 0; w < NTP / 64; ++w) t += red[w][q];
            v[q] = t;
        }
}

// One workgroup per block: pick the (up to) PNB unprocessed columns with the largest residual norms and factorise
// that panel (Householder vectors -> Vall, R entries -> X, compact-WY factor -> Tpan).  Columns are never moved:
// cperm[k + l] records which physical column became logical column k + l, cn[j] = -1 marks column j as done, and the
// trailing update walks over the physical columns skipping the marked ones.  Greedy pivoting is exact for the first
// column of a panel and by pre-panel norms for the others; the rank decision is unaffected because the trailing update
// recomputes every residual norm exactly.
// (A one-wavefront variant with the whole panel in the registers of one SIMD was 1.6x slower: the per-lane serial work
// outweighs the saved barriers.)
template <int NTP, int RPT>
__global__ __launch_bounds__(NTP) void qrp_panel_kernel(const QrpJob *__restrict__ jobs, int k, double *__restrict__ X,
                                                       double *__restrict__ Vall, double *__restrict__ cn,
                                                       double *__restrict__ tau, int64_t *__restrict__ cperm,
                                                       QrpState *__restrict__ state, const double *__restrict__ fro2,
                                                       double tol2, double *__restrict__ Tpan, int pivot) {
    __shared__ double rv[2 * (NTP / 64)];
    __shared__ int64_t ri[2 * (NTP / 64)];
    __shared__ double red[NTP / 64][PNB + 1];
    __shared__ int64_t s_p[PNB];
    __shared__ int s_nbk;
    __shared__ double s_alpha, s_vrow[PNB], Tf[PNB][PNB];
    const int b = blockIdx.x;
    const QrpJob J = jobs[b];
    const QrpState st0 = state[b];
    if (st0.done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t M = J.M, N = J.N;
    const int64_t Kmax = (M < N) ? M : N;      // number of reflectors (N <= M in the pivoted use)
    if (st0.last || k >= Kmax) {
        if (tid == 0) state[b] = QrpState{st0.last ? st0.rank : (int)Kmax, 1, 0, 0};
        return;
    }
    // ---- the PNB largest residual norms among the unprocessed columns (ties -> smallest index: deterministic)
    double cand[RPT];
#pragma unroll
    for (int t = 0; t < RPT; ++t) {
        const int64_t j = tid + (int64_t)t * NTP;
        cand[t] = (j < N) ? cn[J.c_off + j] : -4.0;       // processed columns hold -1
    }
    const double thresh = tol2 * fro2[b];
    if (tid == 0) s_nbk = 0;
    if (!pivot) {   // plain QR: the next PNB columns in their natural order, no rank test
        if (tid == 0) {
            const int nb_ = (int)((Kmax - k < PNB) ? (Kmax - k) : PNB);
            for (int l = 0; l < nb_; ++l) s_p[l] = (int64_t)k + l;
            s_nbk = nb_;
        }
        lds_barrier();
    } else {
        // One barrier per pivot: every wavefront finds its best candidate (value by wave_max, smallest index among equal values
        // by wave_min), publishes it in a double-buffered LDS slot, and EVERY thread merges the NTP/64 entries itself.
        int nsel = 0;
        for (int l = 0; l < PNB; ++l) {
            double bv = -3.0;
            int bidx = 0x7fffffff;
#pragma unroll
            for (int t = 0; t < RPT; ++t)
                if (cand[t] > bv) {
                    bv = cand[t];
                    bidx = tid + t * NTP;
                }
            const double wv = wave_max(bv);
            const int wi = wave_min((bv == wv) ? bidx : 0x7fffffff);
            if (lane == 0) {
                rv[(l & 1) * (NTP / 64) + wave] = wv;
                ri[(l & 1) * (NTP / 64) + wave] = wi;
            }
            lds_barrier();
            double v0 = rv[(l & 1) * (NTP / 64)];
            int64_t i0 = ri[(l & 1) * (NTP / 64)];
#pragma unroll
            for (int w = 1; w < NTP / 64; ++w) {
                const double vw = rv[(l & 1) * (NTP / 64) + w];
                const int64_t iw = ri[(l & 1) * (NTP / 64) + w];
                if (vw > v0 || (vw == v0 && iw < i0)) {
                    v0 = vw;
                    i0 = iw;
                }
            }
            if (!(v0 > thresh)) break;   // uniform: every thread merged the same entries
            if (tid == 0) s_p[l] = i0;
            nsel = l + 1;
#pragma unroll
            for (int t = 0; t < RPT; ++t)
                if (tid + t * NTP == (int)i0) cand[t] = -4.0;
        }
        if (tid == 0) s_nbk = nsel;
        lds_barrier();
    }
    const int nbk = s_nbk;
    if (nbk == 0) {
        if (tid == 0) state[b] = QrpState{k, 1, 0, 0};
        return;
    }
    if (tid == 0) {
        const bool last = (nbk < PNB);
        state[b] = QrpState{last ? k + nbk : 0, 0, nbk, last ? 1 : 0};
        for (int x = 0; x < PNB; ++x)
            for (int y = 0; y < PNB; ++y) Tf[x][y] = 0.0;
    }
    if (tid < nbk) {
        cperm[J.c_off + k + tid] = s_p[tid];
        cn[J.c_off + s_p[tid]] = -1.0;     // processed
    }
    lds_barrier();
    double *Xb = X + J.x_off;
    // ---- gather the panel into registers (X is column-major: contiguous loads)
    double c[PNB][RPT];
#pragma unroll
    for (int t = 0; t < RPT; ++t) {
        const int64_t i = tid + (int64_t)t * NTP;
#pragma unroll
        for (int l = 0; l < PNB; ++l) c[l][t] = (i < M && l < nbk) ? Xb[s_p[l] * M + i] : 0.0;
    }
    // ---- factorise the panel, column by column (must be fully unrolled: c[l] has to stay in registers)
#pragma clang loop unroll(full)
    for (int l = 0; l < PNB; ++l) {
        if (l < nbk) {   // uniform
            const int64_t kl = (int64_t)k + l;
            if (l > 0) {
                // c_l <- (I - V Tf^T V^T) c_l  with the l reflectors found so far (their vectors sit in c[0..l-1])
                double y[PNB];
#pragma unroll
                for (int m = 0; m < PNB; ++m) {
                    y[m] = 0.0;
                    if (m < l) {
#pragma unroll
                        for (int t = 0; t < RPT; ++t) y[m] = fma(c[m][t], c[l][t], y[m]);
                    }
                }
                block_sum_vec<NTP, PNB>(y, red, l, -1);
                double z[PNB];
#pragma unroll
                for (int m = 0; m < PNB; ++m) {
                    z[m] = 0.0;
                    if (m < l) {
#pragma unroll
                        for (int mm = 0; mm < PNB; ++mm)
                            if (mm <= m) z[m] = fma(Tf[mm][m], y[mm], z[m]);
                    }
                }
#pragma unroll
                for (int m = 0; m < PNB; ++m)
                    if (m < l) {
#pragma unroll
                        for (int t = 0; t < RPT; ++t) c[l][t] = fma(-c[m][t], z[m], c[l][t]);
                    }
            }
            // norm below the diagonal and inner products with the earlier vectors (for Tf) in one reduction; the diagonal
            // element alpha and row kl of the earlier vectors are broadcast through LDS by the thread that owns row kl
            double g[PNB + 1];
#pragma unroll
            for (int q = 0; q <= PNB; ++q) g[q] = 0.0;
#pragma unroll
            for (int t = 0; t < RPT; ++t) {
                const int64_t i = tid + (int64_t)t * NTP;
                if (i > kl && i < M) {
                    g[PNB] = fma(c[l][t], c[l][t], g[PNB]);
#pragma unroll
                    for (int m = 0; m < PNB; ++m)
                        if (m < l) g[m] = fma(c[m][t], c[l][t], g[m]);
                } else if (i == kl) {
                    s_alpha = c[l][t];
#pragma unroll
                    for (int m = 0; m < PNB; ++m)
                        if (m < l) s_vrow[m] = c[m][t];
                }
            }
            block_sum_vec<NTP, PNB + 1>(g, red, l, PNB);
            const double s2 = g[PNB], alpha = s_alpha;
            // beta = -sign(alpha) |x|,  tau = (beta - alpha) / beta = 1 + |alpha| / |x|,  scale = 1 / (alpha - beta): one reciprocal
            // square root and one reciprocal, both from the hardware seed + Newton steps (~1 ulp; a Householder vector does not need
            // correctly rounded divisions, and these sit on the serial path of every column)
            double beta = alpha, tk = 0.0, scale = 0.0;
            if (s2 > 0.0) {
                const double x2 = fma(alpha, alpha, s2);
                double r = __builtin_amdgcn_rsq(x2);
                r = r * fma(-0.5 * x2 * r, r, 1.5);
                r = r * fma(-0.5 * x2 * r, r, 1.5);          // 1 / |x|
                const double nx = x2 * r;                   // |x|
                beta = -copysign(nx, alpha);
                tk = fma(fabs(alpha), r, 1.0);
                const double d = alpha - beta;              // = sign(alpha) (|alpha| + |x|): no cancellation
                double q = __builtin_amdgcn_rcp(d);
                q = q * fma(-d, q, 2.0);
                scale = q * fma(-d, q, 2.0);
            }
            // column l of the compact-WY factor: Tf[i2][l] = -tau sum_{m=i2}^{l-1} Tf[i2][m] (v_m^T v_l), thread i2 each
            if (tid < l) {
                double acc = 0;
#pragma unroll
                for (int m = 0; m < PNB; ++m)
                    if (m >= tid && m < l) acc = fma(Tf[tid][m], g[m] * scale + s_vrow[m], acc);
                Tf[tid][l] = -tk * acc;
            } else if (tid == l) {
                Tf[l][l] = tk;
                tau[J.c_off + kl] = tk;
            }
            double *vk = Vall + J.x_off + kl * M;
            double *xc = Xb + s_p[l] * M;
#pragma unroll
            for (int t = 0; t < RPT; ++t) {
                const int64_t i = tid + (int64_t)t * NTP;
                if (i < M) {   // (selects, no divergent branches)
                    const double cv = c[l][t];
                    const double v = (i > kl) ? cv * scale : ((i == kl) ? 1.0 : 0.0);
                    xc[i] = (i < kl) ? cv : ((i == kl) ? beta : 0.0);   // R entry (rows k .. kl-1 were changed by this panel's earlier reflectors)
                    vk[i] = v;
                    c[l][t] = v;
                }
            }
            lds_barrier();   // Tf column l, s_alpha / s_vrow reuse
        }
    }
    if (tid < PNB * PNB) Tpan[(int64_t)b * PNB * PNB + tid] = Tf[tid / PNB][tid % PNB];
}

// ---- complex panel kernel (LAPACK zlarfg / zlarft: beta real, the factorisation applies H^H from the left) ----------------------
constexpr int KC = 2 * PNB + 1;   // real values reduced together in the complex panel kernel

template <int NTP, int K>
__device__ __forceinline__ void block_sum_arr(double (&v)[K], double (*red)[KC]) {
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) red[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
        double t = 0;
#pragma unroll
        for (int w = 0; w < NTP / 64; ++w) t += red[w][q];
        v[q] = t;
    }
}

template <int NTP, int RPT>
__global__ __launch_bounds__(NTP) void qrp_panel_kernel_c(const QrpJob *__restrict__ jobs, int k, cd *__restrict__ X,
                                                          cd *__restrict__ Vall, double *__restrict__ cn,
                                                          cd *__restrict__ tau, int64_t *__restrict__ cperm,
                                                          QrpState *__restrict__ state, const double *__restrict__ fro2,
                                                          double tol2, cd *__restrict__ Tpan, int pivot) {
    __shared__ double rv[NTP / 64];
    __shared__ int64_t ri[NTP / 64];
    __shared__ double red[NTP / 64][KC];
    __shared__ int64_t s_p[PNB];
    __shared__ int s_nbk;
    __shared__ cd s_alpha, s_vrow[PNB], Tf[PNB][PNB];
    const int b = blockIdx.x;
    const QrpJob J = jobs[b];
    const QrpState st0 = state[b];
    if (st0.done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t M = J.M, N = J.N;
    const int64_t Kmax = (M < N) ? M : N;      // number of reflectors (N <= M in the pivoted use)
    if (st0.last || k >= Kmax) {
        if (tid == 0) state[b] = QrpState{st0.last ? st0.rank : (int)Kmax, 1, 0, 0};
        return;
    }
    double cand[RPT];
#pragma unroll
    for (int t = 0; t < RPT; ++t) {
        const int64_t j = tid + (int64_t)t * NTP;
        cand[t] = (j < N) ? cn[J.c_off + j] : -4.0;
    }
    const double thresh = tol2 * fro2[b];
    if (tid == 0) s_nbk = 0;
    if (!pivot) {   // plain QR: the next PNB columns in their natural order, no rank test
        if (tid == 0) {
            const int nb_ = (int)((Kmax - k < PNB) ? (Kmax - k) : PNB);
            for (int l = 0; l < nb_; ++l) s_p[l] = (int64_t)k + l;
            s_nbk = nb_;
        }
        __syncthreads();
    } else
    for (int l = 0; l < PNB; ++l) {
        double bv = -3.0;
        int64_t bidx = N;
#pragma unroll
        for (int t = 0; t < RPT; ++t)
            if (cand[t] > bv) {
                bv = cand[t];
                bidx = tid + (int64_t)t * NTP;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int64_t oi = __shfl_xor(bidx, off, 64);
            if (ov > bv || (ov == bv && oi < bidx)) {
                bv = ov;
                bidx = oi;
            }
        }
        __syncthreads();
        if (lane == 0) {
            rv[wave] = bv;
            ri[wave] = bidx;
        }
        __syncthreads();
        if (tid == 0) {
            double v0 = rv[0];
            int64_t i0 = ri[0];
            for (int w = 1; w < NTP / 64; ++w)
                if (rv[w] > v0 || (rv[w] == v0 && ri[w] < i0)) {
                    v0 = rv[w];
                    i0 = ri[w];
                }
            if (v0 > thresh && s_nbk == l) {
                s_p[l] = i0;
                s_nbk = l + 1;
            }
        }
        __syncthreads();
        if (s_nbk <= l) break;
        const int64_t w = s_p[l];
#pragma unroll
        for (int t = 0; t < RPT; ++t)
            if (tid + (int64_t)t * NTP == w) cand[t] = -4.0;
    }
    const int nbk = s_nbk;
    if (nbk == 0) {
        if (tid == 0) state[b] = QrpState{k, 1, 0, 0};
        return;
    }
    if (tid == 0) {
        const bool last = (nbk < PNB);
        state[b] = QrpState{last ? k + nbk : 0, 0, nbk, last ? 1 : 0};
        for (int x = 0; x < PNB; ++x)
            for (int y = 0; y < PNB; ++y) Tf[x][y] = cd{0.0, 0.0};
    }
    if (tid < nbk) {
        cperm[J.c_off + k + tid] = s_p[tid];
        cn[J.c_off + s_p[tid]] = -1.0;
    }
    __syncthreads();
    cd *Xb = X + J.x_off;
    cd c[PNB][RPT];
#pragma unroll
    for (int t = 0; t < RPT; ++t) {
        const int64_t i = tid + (int64_t)t * NTP;
#pragma unroll
        for (int l = 0; l < PNB; ++l) c[l][t] = (i < M && l < nbk) ? Xb[s_p[l] * M + i] : cd{0.0, 0.0};
    }
#pragma clang loop unroll(full)
    for (int l = 0; l < PNB; ++l) {
        if (l < nbk) {
            const int64_t kl = (int64_t)k + l;
            if (l > 0) {
                // c_l <- (I - V T^H V^H) c_l :  y = V^H c_l,  z = T^H y,  c_l -= V z
                double y[2 * PNB];
#pragma unroll
                for (int m = 0; m < PNB; ++m) {
                    cd a{0.0, 0.0};
                    if (m < l) {
#pragma unroll
                        for (int t = 0; t < RPT; ++t) a = c_fmac(c[m][t], c[l][t], a);
                    }
                    y[2 * m] = a.x;
                    y[2 * m + 1] = a.y;
                }
                block_sum_arr<NTP, 2 * PNB>(y, red);
                cd z[PNB];
#pragma unroll
                for (int m = 0; m < PNB; ++m) {
                    z[m] = cd{0.0, 0.0};
                    if (m < l) {
#pragma unroll
                        for (int mm = 0; mm < PNB; ++mm)
                            if (mm <= m) z[m] = c_fmac(Tf[mm][m], cd{y[2 * mm], y[2 * mm + 1]}, z[m]);
                    }
                }
#pragma unroll
                for (int m = 0; m < PNB; ++m)
                    if (m < l) {
                        const cd zn{-z[m].x, -z[m].y};
#pragma unroll
                        for (int t = 0; t < RPT; ++t) c[l][t] = c_fma(c[m][t], zn, c[l][t]);
                    }
            }
            double g[KC];
#pragma unroll
            for (int q = 0; q < KC; ++q) g[q] = 0.0;
#pragma unroll
            for (int t = 0; t < RPT; ++t) {
                const int64_t i = tid + (int64_t)t * NTP;
                if (i > kl && i < M) {
                    g[2 * PNB] = fma(c[l][t].x, c[l][t].x, fma(c[l][t].y, c[l][t].y, g[2 * PNB]));
#pragma unroll
                    for (int m = 0; m < PNB; ++m)
                        if (m < l) {
                            const cd a = c_mulc(c[m][t], c[l][t]);
                            g[2 * m] += a.x;
                            g[2 * m + 1] += a.y;
                        }
                } else if (i == kl) {
                    s_alpha = c[l][t];
#pragma unroll
                    for (int m = 0; m < PNB; ++m)
                        if (m < l) s_vrow[m] = c[m][t];
                }
            }
            block_sum_arr<NTP, KC>(g, red);
            const double s2 = g[2 * PNB];
            const cd alpha = s_alpha;
            double beta = alpha.x;
            cd tk{0.0, 0.0}, scale{0.0, 0.0};
            if (s2 > 0.0 || alpha.y != 0.0) {       // zlarfg
                beta = -copysign(sqrt(alpha.x * alpha.x + alpha.y * alpha.y + s2), alpha.x);
                tk = cd{(beta - alpha.x) / beta, -alpha.y / beta};
                const double dr = alpha.x - beta, di = alpha.y, dn = dr * dr + di * di;
                scale = cd{dr / dn, -di / dn};      // 1 / (alpha - beta)
            }
            // column l of T:  T[i2][l] = -tau sum_{m=i2}^{l-1} T[i2][m] (v_m^H v_l),  v_m^H v_l = g_m scale + conj(v_m[kl])
            if (tid < l) {
                cd acc{0.0, 0.0};
#pragma unroll
                for (int m = 0; m < PNB; ++m)
                    if (m >= tid && m < l) {
                        cd sml = c_mul(cd{g[2 * m], g[2 * m + 1]}, scale);
                        sml.x += s_vrow[m].x;
                        sml.y -= s_vrow[m].y;
                        acc = c_fma(Tf[tid][m], sml, acc);
                    }
                const cd r = c_mul(tk, acc);
                Tf[tid][l] = cd{-r.x, -r.y};
            } else if (tid == l) {
                Tf[l][l] = tk;
                tau[J.c_off + kl] = tk;
            }
            cd *vk = Vall + J.x_off + kl * M;
            cd *xc = Xb + s_p[l] * M;
#pragma unroll
            for (int t = 0; t < RPT; ++t) {
                const int64_t i = tid + (int64_t)t * NTP;
                if (i < M) {
                    cd v;
                    if (i < kl) {
                        v = cd{0.0, 0.0};
                        xc[i] = c[l][t];
                    } else if (i == kl) {
                        xc[i] = cd{beta, 0.0};
                        v = cd{1.0, 0.0};
                    } else {
                        xc[i] = cd{0.0, 0.0};
                        v = c_mul(c[l][t], scale);
                    }
                    vk[i] = v;
                    c[l][t] = v;
                }
            }
            __syncthreads();
        }
    }
    if (tid < PNB * PNB) Tpan[(int64_t)b * PNB * PNB + tid] = Tf[tid / PNB][tid % PNB];
}

// ---- compact-WY block reflector applied to a 16-column tile of a row-major matrix, on the matrix cores ----------
//     C[k0:, tile] <- (I - V Tf' V^T) C[k0:, tile],    Tf' = Tf^T (TRANS: trailing update of the factorisation)
//                                                      or Tf (forming Q U_R),
// V[l*M + i] = component i of reflector l (0 above its diagonal), nb <= NB reflectors, Tf upper triangular in LDS.
// 1024 threads = 16 wavefronts, each owning 16-row slabs (slab s of wave w = rows k0 + 16 (w + 16 s) ...):
//   pass 1  Y  = V^T C      v_mfma_f64_16x16x4: A(l, i) = V, B(i, j) = C, K runs over the rows      -> LDS reduce
//   small   Z  = Tf' Y      (NB x 16, 256 threads)
//   pass 2  C -= V Z        A(i, l) = V, B(l, j) = -Z, accumulator preloaded with the C slab (NB/4 MFMAs per slab)
// Returns (NORMS) sum_{i >= kend} C[i, j]^2 of the updated tile column j = j0 + (lane & 15), valid in threads < 16.
// (Complex data: read ^T as ^H; every MFMA becomes four on the (re, im) planes of the fragments.)
constexpr int NTR = 1024, RCOLS = 16;

template <class T, int NB, int NTH = NTR>
struct WySmem {
    double red[Sc<T>::cplx ? 2 : 1][NTH / 64][NB][RCOLS];      // complex: (re, im) planes
    T Y[NB][RCOLS], Z[NB][RCOLS], Tf[NB][NB];
    double nrm[NTH / 64][RCOLS];
};

template <class T, int NB, bool TRANS, bool NORMS, int NTH = NTR>
__device__ __forceinline__ double wy_apply_tile(T *Cb, int64_t rs, int64_t cs, int64_t k0, int64_t M, int64_t j0, int64_t jend,
                                                const T *__restrict__ V, int nb, int64_t kend, WySmem<T, NB, NTH> &sm,
                                                bool col_ok = true) {
    typedef Sc<T> S;
    constexpr bool CX = Sc<T>::cplx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lo = lane & 15, kq = lane >> 4;
    const int64_t j = j0 + lo;
    const bool jok = (j < jend) && col_ok;
    // ---- pass 1: Y(l, j) = sum_i conj(V(l, i)) C(i, j)
    typename S::Acc acc{};
    for (int64_t i0 = k0 + 16 * wave; i0 < M; i0 += 16 * (NTH / 64)) {
        T a[4], bb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + 4 * kq + q;
            const bool iok = i < M;
            a[q] = (iok && lo < nb) ? V[(int64_t)lo * M + i] : T(0.0);
            bb[q] = (iok && jok) ? Cb[i * rs + j * cs] : T(0.0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) S::template mfma<true>(a[q], bb[q], acc);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
        if (kq + 4 * reg < NB) {
            if constexpr (CX) {
                sm.red[0][wave][kq + 4 * reg][lo] = acc.r[reg];
                sm.red[1][wave][kq + 4 * reg][lo] = acc.i[reg];
            } else
                sm.red[0][wave][kq + 4 * reg][lo] = acc[reg];
        }
    __syncthreads();
    if (threadIdx.x < NB * RCOLS) {
        const int l = threadIdx.x >> 4, c = threadIdx.x & 15;
        double tr = 0, ti = 0;
#pragma unroll
        for (int q = 0; q < NTH / 64; ++q) {
            tr += sm.red[0][q][l][c];
            if constexpr (CX) ti += sm.red[1][q][l][c];
        }
        if constexpr (CX)
            sm.Y[l][c] = cd{tr, ti};
        else
            sm.Y[l][c] = tr;
    }
    __syncthreads();
    if (threadIdx.x < NB * RCOLS) {
        const int l = threadIdx.x >> 4, c = threadIdx.x & 15;
        T t = T(0.0);
#pragma unroll
        for (int m = 0; m < NB; ++m) t = TRANS ? S::fmac(sm.Tf[m][l], sm.Y[m][c], t) : S::fma(sm.Tf[l][m], sm.Y[m][c], t);
        sm.Z[l][c] = S::neg(t);
    }
    __syncthreads();
    T zneg[NB / 4];
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) zneg[q] = sm.Z[4 * q + kq][lo];
    // ---- pass 2: C += V Zneg, two 16-row slabs per iteration (all loads before the stores: the compiler cannot prove that the
    //      stores of one slab do not alias the loads of the next)
    double nrm = 0;
    for (int64_t i0 = k0 + 16 * wave; i0 < M; i0 += 2 * 16 * (NTH / 64)) {
        typename S::Acc c[2];
        T av[2][NB / 4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t ib = i0 + (int64_t)h * 16 * (NTH / 64);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t i = ib + kq + 4 * reg;
                S::set(c[h], reg, (i < M && jok) ? Cb[i * rs + j * cs] : T(0.0));
            }
#pragma unroll
            for (int q = 0; q < NB / 4; ++q) {
                const int64_t i = ib + lo;
                const int l = 4 * q + kq;
                av[h][q] = (i < M && l < nb) ? V[(int64_t)l * M + i] : T(0.0);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int q = 0; q < NB / 4; ++q) S::template mfma<false>(av[h][q], zneg[q], c[h]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t ib = i0 + (int64_t)h * 16 * (NTH / 64);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t i = ib + kq + 4 * reg;
                if (i < M && jok) {
                    const T v = S::get(c[h], reg);
                    Cb[i * rs + j * cs] = v;
                    if (NORMS && i >= kend) nrm = S::abs2(v, nrm);
                }
            }
        }
    }
    if (!NORMS) return 0.0;
    nrm += __shfl_xor(nrm, 16, 64);
    nrm += __shfl_xor(nrm, 32, 64);
    if (lane < RCOLS) sm.nrm[wave][lo] = nrm;
    __syncthreads();
    double t = 0;
    if (threadIdx.x < RCOLS) {
#pragma unroll
        for (int q = 0; q < NTH / 64; ++q) t += sm.nrm[q][threadIdx.x];
    }
    return t;
}

// trailing update with the panel's nbk reflectors:  X[k:, j] <- (I - V Tf^T V^T) X[k:, j]  for every column j that has not
// been factorised yet (cn[j] >= 0; tiles walk over the physical columns), plus the exact residual norms (rows >= k + nbk).
template <class T>
__global__ __launch_bounds__(NTR) void qrp_update_kernel(const QrpJob *__restrict__ jobs, int k, T *__restrict__ X,
                                                         const T *__restrict__ Vall, double *__restrict__ cn,
                                                         const QrpState *__restrict__ state, const T *__restrict__ Tpan) {
    __shared__ WySmem<T, PNB> sm;
    const int b = blockIdx.y;
    const QrpState st = state[b];
    if (st.done || st.nbk == 0) return;
    const QrpJob J = jobs[b];
    const int nbk = st.nbk;
    const int64_t j0 = (int64_t)blockIdx.x * RCOLS;
    if (j0 >= J.N) return;
    const int64_t jl = j0 + (threadIdx.x & (RCOLS - 1));
    const bool col_ok = (jl < J.N) && (cn[J.c_off + jl] >= 0.0);
    if (__ballot(col_ok) == 0) return;   // same 16 columns in every wavefront: uniform over the workgroup
    if (threadIdx.x < PNB * PNB) sm.Tf[threadIdx.x / PNB][threadIdx.x % PNB] = Tpan[(int64_t)b * PNB * PNB + threadIdx.x];
    const double nrm = wy_apply_tile<T, PNB, true, true>(X + J.x_off, 1, J.M, k, J.M, j0, J.N, Vall + J.x_off + (int64_t)k * J.M,
                                                         nbk, (int64_t)k + nbk, sm, col_ok);
    if (threadIdx.x < RCOLS && col_ok) cn[J.c_off + jl] = nrm;
}

// after the factorisation: the columns that were never used as pivots become the logical columns r .. N-1 (in
// increasing physical order)
__global__ __launch_bounds__(NT) void qrp_finish_perm_kernel(const QrpJob *__restrict__ jobs, const QrpState *__restrict__ state,
                                                             const double *__restrict__ cn, int64_t *__restrict__ cperm) {
    __shared__ int cnt[NT];
    const QrpJob J = jobs[blockIdx.x];
    const int64_t N = J.N, r = state[blockIdx.x].rank;
    const int64_t per = (N + NT - 1) / NT, lo = (int64_t)threadIdx.x * per, hi = (lo + per < N) ? lo + per : N;
    int mine = 0;
    for (int64_t j = lo; j < hi; ++j) mine += (cn[J.c_off + j] >= 0.0) ? 1 : 0;
    cnt[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < NT; ++t) {
            const int c = cnt[t];
            cnt[t] = run;
            run += c;
        }
    }
    __syncthreads();
    int64_t pos = r + cnt[threadIdx.x];
    for (int64_t j = lo; j < hi; ++j)
        if (cn[J.c_off + j] >= 0.0) cperm[J.c_off + pos++] = j;
}

// R_top (r x N, contiguous, logical column order) = upper-trapezoidal part of the first r rows of X
template <class T>
__global__ __launch_bounds__(NT) void qrp_extract_kernel(const QrpJob *__restrict__ jobs, const QrpState *__restrict__ state,
                                                         const T *__restrict__ X, const int64_t *__restrict__ cperm,
                                                         T *__restrict__ Rtop) {
    const QrpJob J = jobs[blockIdx.y];
    const int64_t r = state[blockIdx.y].rank, N = J.N;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < r * N; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / N, j = e - i * N;
        Rtop[J.r_off + e] = (j >= i) ? X[J.x_off + cperm[J.c_off + j] * J.M + i] : T(0.0);
    }
}

// T (M x r, row-major, stored at x_off) = [U_R ; 0]
template <class T>
__global__ __launch_bounds__(NT) void qrp_form_t_kernel(const QrpJob *__restrict__ jobs, const QrpState *__restrict__ state,
                                                        const T *__restrict__ UR, T *__restrict__ Tm) {
    const QrpJob J = jobs[blockIdx.y];
    const int64_t r = state[blockIdx.y].rank, M = J.M;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < M * r; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / r;
        Tm[J.x_off + e] = (i < r) ? UR[J.r_off + e] : T(0.0);
    }
}

// ---- blocked application of Q_r = H_0 ... H_{r-1} (compact WY, 16 reflectors per launch) ------------------------
// H_{k0} ... H_{k0+15} = I - V Tf V^H  with Tf upper triangular (LAPACK dlarft / zlarft, forward / columnwise).
constexpr int QNB = 16;

// one workgroup per (block of 16 reflectors, job): Gram of the panel rows, then the Tf recurrence.  One launch
// covers every block of every job.
template <class T>
__global__ __launch_bounds__(NTR) void qrp_tfactor_kernel(const QrpJob *__restrict__ jobs, const QrpState *__restrict__ state,
                                                          const T *__restrict__ Vall, const T *__restrict__ tau,
                                                          T *__restrict__ Tfac) {
    __shared__ T S[QNB][QNB + 1];
    __shared__ T Tf[QNB][QNB + 1];
    const QrpJob J = jobs[blockIdx.y];
    const int64_t r = state[blockIdx.y].rank, M = J.M;
    const int64_t k0 = (int64_t)blockIdx.x * QNB;
    if (k0 >= r) return;
    const int nb = (int)((r - k0 < QNB) ? (r - k0) : QNB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T *V = Vall + J.x_off + k0 * M;
    // 16 waves x 16 (l, l') pairs each: pair index = wave * 16 + q  ->  l = wave, l' = q;  S[l][l'] = v_l^H v_l'
    for (int q = 0; q < QNB; ++q) {
        const int l = wave, lp = q;
        T acc = T(0.0);
        if (l < lp && lp < nb)
            for (int64_t i = k0 + lp + lane; i < M; i += 64) acc = Sc<T>::fmac(V[l * M + i], V[lp * M + i], acc);
        if constexpr (Sc<T>::cplx) {
            acc.x = wave_sum(acc.x);
            acc.y = wave_sum(acc.y);
        } else
            acc = wave_sum(acc);
        if (lane == 0) S[l][lp] = acc;
    }
    __syncthreads();
    if (threadIdx.x < QNB * QNB) Tf[threadIdx.x >> 4][threadIdx.x & 15] = T(0.0);
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        const T tj = tau[J.c_off + k0 + j];
        if (threadIdx.x < j) {
            const int i = threadIdx.x;
            T acc = T(0.0);
            for (int m = i; m < j; ++m) acc = Sc<T>::fma(Tf[i][m], S[m][j], acc);
            Tf[i][j] = Sc<T>::nmul(tj, acc);
        } else if (threadIdx.x == j)
            Tf[j][j] = tj;
        __syncthreads();
    }
    if (threadIdx.x < QNB * QNB)
        Tfac[(J.pad0 + blockIdx.x) * (QNB * QNB) + threadIdx.x] = Tf[threadIdx.x >> 4][threadIdx.x & 15];
}

// C[k0:, tile] <- (I - V Tf V^H) C[k0:, tile]   for one block of 16 reflectors and a 16-column tile of C (M x r)
template <class T>
__global__ __launch_bounds__(NTR) void qrp_apply_q_block_kernel(const QrpJob *__restrict__ jobs,
                                                                const QrpState *__restrict__ state, int blk,
                                                                T *__restrict__ C, const T *__restrict__ Vall,
                                                                const T *__restrict__ Tfac) {
    __shared__ WySmem<T, QNB> sm;
    const int b = blockIdx.y;
    const QrpJob J = jobs[b];
    const int64_t r = state[b].rank;
    const int64_t k0 = (int64_t)blk * QNB;
    if (k0 >= r) return;
    const int64_t j0 = (int64_t)blockIdx.x * RCOLS;
    if (j0 >= r) return;
    const int nb = (int)((r - k0 < QNB) ? (r - k0) : QNB);
    if (threadIdx.x < QNB * QNB) sm.Tf[threadIdx.x >> 4][threadIdx.x & 15] = Tfac[(J.pad0 + blk) * (QNB * QNB) + threadIdx.x];
    wy_apply_tile<T, QNB, false, false>(C + J.x_off, r, 1, k0, J.M, j0, r, Vall + J.x_off + k0 * J.M, nb, 0, sm);
}

// final outputs from Tm = Q_r U_R (M x r), S_R, VH_R (r x N) and the column permutation
template <class T>
__global__ __launch_bounds__(NT) void qrp_output_kernel(const QrpJob *__restrict__ jobs, const SvdJob *__restrict__ sj,
                                                        const QrpState *__restrict__ state, const T *__restrict__ Tm,
                                                        const double *__restrict__ SR, const T *__restrict__ VHR,
                                                        const int64_t *__restrict__ cperm, T *__restrict__ U,
                                                        double *__restrict__ S, T *__restrict__ VH) {
    const QrpJob J = jobs[blockIdx.y];
    const SvdJob O = sj[blockIdx.y];
    const int64_t r = state[blockIdx.y].rank, M = J.M, N = J.N, K = N;  // K = min(m, n)
    const int64_t stride = (int64_t)gridDim.x * NT, t0 = (int64_t)blockIdx.x * NT + threadIdx.x;
    const T zero = T(0.0);
    for (int64_t e = t0; e < K; e += stride) S[O.s_off + e] = (e < r) ? SR[J.c_off + e] : 0.0;
    if (!J.tr) {
        // A = X (m = M >= n = N):  U = Tm (M x K, zero padded),  VH[jj][cperm[c]] = VH_R[jj][c]
        for (int64_t e = t0; e < M * K; e += stride) {
            const int64_t i = e / K, jj = e - i * K;
            U[O.u_off + e] = (jj < r) ? Tm[J.x_off + i * r + jj] : zero;
        }
        for (int64_t e = t0; e < K * N; e += stride) {
            const int64_t jj = e / N, c = e - jj * N;
            VH[O.vh_off + jj * N + cperm[J.c_off + c]] = (jj < r) ? VHR[J.r_off + jj * N + c] : zero;
        }
    } else {
        // A = X^H (m = N < n = M):  U[cperm[c]][jj] = conj(VH_R[jj][c]),  VH[jj][c] = conj(Tm[c][jj])
        for (int64_t e = t0; e < N * K; e += stride) {
            const int64_t c = e / K, jj = e - c * K;
            U[O.u_off + cperm[J.c_off + c] * K + jj] = Sc<T>::conj((jj < r) ? VHR[J.r_off + jj * N + c] : zero);
        }
        for (int64_t e = t0; e < K * M; e += stride) {
            const int64_t jj = e / M, c = e - jj * M;
            VH[O.vh_off + e] = Sc<T>::conj((jj < r) ? Tm[J.x_off + c * r + jj] : zero);
        }
    }
}

// ---- host: which panel kernel factorises the next PNB columns (chosen per call from the largest block) ----------------------
extern int tpa_svd_small_panel;      // tpa_svd.hip, with the other switches
template <bool CPLX, class T>
void launch_qrp_panel(int64_t m_max, int64_t n_max, int n_jobs, hipStream_t st, const QrpJob *qjobs, int k, T *X, T *Vall,
                      double *cn, T *tau, int64_t *cperm, QrpState *state, const double *fro2, T *Tpan, double tol2, int pivot) {
    auto go = [&](auto kernel, int ntp) {
        kernel<<<n_jobs, ntp, 0, st>>>(qjobs, k, X, Vall, cn, tau, cperm, state, fro2, tol2, Tpan, pivot);
    };
    if constexpr (CPLX) {
        if (m_max <= 4 * 256) go(qrp_panel_kernel_c<256, 4>, 256);
        else go(qrp_panel_kernel_c<256, 8>, 256);
    } else if (pivot && m_max <= 8 * 64 && n_max <= 8 * 64 && tpa_svd_small_panel)
        // small blocks (chi <= 512, Hubbard ladders): the whole panel in ONE wavefront -- no workgroup barriers, no LDS stage in
        // the reductions (for >= 1000 rows this variant was 1.6x slower, here the barriers are all there is to save)
        go(qrp_panel_kernel<64, 8>, 64);
    else if (m_max <= 8 * 256) go(qrp_panel_kernel<256, 8>, 256);
    else if (m_max <= 16 * 256) go(qrp_panel_kernel<256, 16>, 256);
    else go(qrp_panel_kernel<256, 32>, 256);
}
