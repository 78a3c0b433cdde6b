// Unpivoted blocked Householder QR with ONE LAUNCH PER PANEL (round 5; included by tpa_svd.hip after the compact-WY machinery).
//
// `qr_run_wy` (np.linalg.qr per block, np_conserved.py:4190; since round 5 also the orthogonalisation of the sketch
// Y = X Omega^H of the warm-started block SVD, linalg/_svd_warm.py::svd_blocks_sketch) used to run the pivoted QR's two kernels per
// 8-column panel -- panel factorisation (one workgroup per block, ~27 us) THEN trailing update (~23 us): a chain of 2 K / 8
// dependent launches, 3.7 ms for the 1070 x 600 sketch of a chi = 2048 theta (profiles/r05_sketch_kernel_stats.csv).  Without
// pivoting the next panel's columns are known in advance, so the factorisation of panel k + 1 does not have to wait for the
// whole update with panel k: step k is ONE launch in which
//   * workgroup 0 of every block ("panel role") brings the 8 columns of panel k + 1 up to date with the reflectors of panel k
//     (64 inner products, in the registers that hold the panel anyway) and factorises them right away, while
//   * the other workgroups ("update role") apply the reflectors of panel k to the columns behind panel k + 1
//     (16-column tiles on the matrix cores: `wy_apply_tile`, as before).
// The chain per panel is max(panel role, update role) instead of their sum.  Same arithmetic per column as the two-kernel
// path (left-looking panel, compact-WY trailing update), so R and Q agree with it to rounding.
// Real data, blocks with at most 2048 rows; other calls keep the two-kernel path.  512 threads per workgroup: the panel role holds
// its 8 columns and the 8 reflectors of the previous panel in 2 x 8 x 4 registers per thread (1024 threads would leave 128 VGPRs
// per thread: the first version of this kernel spilled 747 of them).

constexpr int NTQ = 512;        // threads of both roles
constexpr int QLA_RPT = 4;      // rows per thread of the panel role: M <= 4 * NTQ = 2048

struct QlaPanelSmem {
    double red[NTQ / 64][PNB + 1];
    double big[NTQ / 64][PNB * PNB];    // partial sums of the 64 inner products V_k^T C
    double y[PNB * PNB], z[PNB * PNB];
    double Tk[PNB][PNB], Tf[PNB][PNB];
    double s_alpha, s_vrow[PNB];
};
union QlaSmem {
    QlaPanelSmem p;
    WySmem<double, PNB, NTQ> u;
};

// k: first column of the panel whose reflectors are APPLIED in this launch (k < 0: none yet -- the very first launch only factorises
// panel 0).  Tpan2: [2][n_jobs][PNB * PNB], panel k's factor in slot (k / PNB) & 1.  j_first: first column (multiple of RCOLS) the
// update role has to look at.
__global__ __launch_bounds__(NTQ) void qr_la_step_kernel(const QrpJob *__restrict__ jobs, int k, double *__restrict__ X,
                                                        double *__restrict__ Vall, double *__restrict__ tau,
                                                        double *__restrict__ Tpan2, int n_jobs, int64_t j_first) {
    __shared__ QlaSmem sm;
    const int b = blockIdx.y;
    const QrpJob J = jobs[b];
    const int64_t M = J.M, N = J.N;
    const int64_t Kmax = (M < N) ? M : N;
    const int tid = threadIdx.x;
    double *Xb = X + J.x_off;
    if (blockIdx.x > 0) {
        // ---------------------------------------------------------------- update role: columns >= k + 2 PNB, reflectors of panel k
        if (k < 0 || k >= Kmax) return;
        const int nbk = (int)((Kmax - k < PNB) ? (Kmax - k) : PNB);
        const int64_t j0 = j_first + (int64_t)(blockIdx.x - 1) * RCOLS;
        if (j0 >= N) return;
        const int64_t jl = j0 + (tid & (RCOLS - 1));
        const bool col_ok = (jl < N) && (jl >= (int64_t)k + 2 * PNB);
        if (__ballot(col_ok) == 0) return;      // the same 16 columns in every wavefront: uniform over the workgroup
        if (tid < PNB * PNB) sm.u.Tf[tid / PNB][tid % PNB] = Tpan2[((int64_t)((k / PNB) & 1) * n_jobs + b) * PNB * PNB + tid];
        wy_apply_tile<double, PNB, true, false, NTQ>(Xb, 1, M, k, M, j0, N, Vall + J.x_off + (int64_t)k * M, nbk, 0, sm.u, col_ok);
        return;
    }
    // -------------------------------------------------------------------- panel role: columns kp .. kp + nb - 1
    const int64_t kp = (int64_t)k + PNB;
    if (kp >= Kmax) return;
    const int nb = (int)((Kmax - kp < PNB) ? (Kmax - kp) : PNB);
    QlaPanelSmem &S = sm.p;
    double c[PNB][QLA_RPT];
#pragma unroll
    for (int t = 0; t < QLA_RPT; ++t) {
        const int64_t i = tid + (int64_t)t * NTQ;
#pragma unroll
        for (int l = 0; l < PNB; ++l) c[l][t] = (i < M && l < nb) ? Xb[(kp + l) * M + i] : 0.0;
    }
    if (tid < PNB * PNB) S.Tf[tid / PNB][tid % PNB] = 0.0;
    if (k >= 0) {
        // C <- (I - V_k T_k^T V_k^T) C for the panel's own columns (panel k is complete: another panel follows it)
        double v[PNB][QLA_RPT];
#pragma unroll
        for (int t = 0; t < QLA_RPT; ++t) {
            const int64_t i = tid + (int64_t)t * NTQ;
#pragma unroll
            for (int m = 0; m < PNB; ++m) v[m][t] = (i < M) ? Vall[J.x_off + ((int64_t)k + m) * M + i] : 0.0;
        }
        if (tid < PNB * PNB) S.Tk[tid / PNB][tid % PNB] = Tpan2[((int64_t)((k / PNB) & 1) * n_jobs + b) * PNB * PNB + tid];
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int m = 0; m < PNB; ++m)
#pragma unroll
            for (int l = 0; l < PNB; ++l) {
                double a = 0.0;
#pragma unroll
                for (int t = 0; t < QLA_RPT; ++t) a = fma(v[m][t], c[l][t], a);
                a = wave_sum(a);
                if (lane == 0) S.big[wave][m * PNB + l] = a;
            }
        lds_barrier();
        if (tid < PNB * PNB) {
            double a = 0.0;
#pragma unroll
            for (int w = 0; w < NTQ / 64; ++w) a += S.big[w][tid];
            S.y[tid] = a;
        }
        lds_barrier();
        if (tid < PNB * PNB) {      // z(m, l) = sum_mm T_k(mm, m) y(mm, l)   (T_k^T y; T_k upper triangular)
            const int m = tid / PNB, l = tid % PNB;
            double a = 0.0;
#pragma unroll
            for (int mm = 0; mm < PNB; ++mm)
                if (mm <= m) a = fma(S.Tk[mm][m], S.y[mm * PNB + l], a);
            S.z[tid] = a;
        }
        lds_barrier();
#pragma unroll
        for (int m = 0; m < PNB; ++m)
#pragma unroll
            for (int l = 0; l < PNB; ++l) {
                const double zz = S.z[m * PNB + l];
#pragma unroll
                for (int t = 0; t < QLA_RPT; ++t) c[l][t] = fma(-v[m][t], zz, c[l][t]);
            }
    }
    lds_barrier();
    // ---- factorise the panel, column by column: the loop of qrp_panel_kernel (left-looking inside the panel) on NTQ threads
#pragma clang loop unroll(full)
    for (int l = 0; l < PNB; ++l) {
        if (l < nb) {   // uniform
            const int64_t kl = kp + l;
            if (l > 0) {
                double y[PNB];
#pragma unroll
                for (int m = 0; m < PNB; ++m) {
                    y[m] = 0.0;
                    if (m < l) {
#pragma unroll
                        for (int t = 0; t < QLA_RPT; ++t) y[m] = fma(c[m][t], c[l][t], y[m]);
                    }
                }
                block_sum_vec<NTQ, PNB>(y, S.red, l, -1);
                double z[PNB];
#pragma unroll
                for (int m = 0; m < PNB; ++m) {
                    z[m] = 0.0;
                    if (m < l) {
#pragma unroll
                        for (int mm = 0; mm < PNB; ++mm)
                            if (mm <= m) z[m] = fma(S.Tf[mm][m], y[mm], z[m]);
                    }
                }
#pragma unroll
                for (int m = 0; m < PNB; ++m)
                    if (m < l) {
#pragma unroll
                        for (int t = 0; t < QLA_RPT; ++t) c[l][t] = fma(-c[m][t], z[m], c[l][t]);
                    }
            }
            double g[PNB + 1];
#pragma unroll
            for (int q = 0; q <= PNB; ++q) g[q] = 0.0;
#pragma unroll
            for (int t = 0; t < QLA_RPT; ++t) {
                const int64_t i = tid + (int64_t)t * NTQ;
                if (i > kl && i < M) {
                    g[PNB] = fma(c[l][t], c[l][t], g[PNB]);
#pragma unroll
                    for (int m = 0; m < PNB; ++m)
                        if (m < l) g[m] = fma(c[m][t], c[l][t], g[m]);
                } else if (i == kl) {
                    S.s_alpha = c[l][t];
#pragma unroll
                    for (int m = 0; m < PNB; ++m)
                        if (m < l) S.s_vrow[m] = c[m][t];
                }
            }
            block_sum_vec<NTQ, PNB + 1>(g, S.red, l, PNB);
            const double s2 = g[PNB], alpha = S.s_alpha;
            double beta = alpha, tk = 0.0, scale = 0.0;
            if (s2 > 0.0) {
                const double x2 = fma(alpha, alpha, s2);
                double r = __builtin_amdgcn_rsq(x2);
                r = r * fma(-0.5 * x2 * r, r, 1.5);
                r = r * fma(-0.5 * x2 * r, r, 1.5);          // 1 / |x|
                const double nx = x2 * r;                   // |x|
                beta = -copysign(nx, alpha);
                tk = fma(fabs(alpha), r, 1.0);
                const double d = alpha - beta;
                double q = __builtin_amdgcn_rcp(d);
                q = q * fma(-d, q, 2.0);
                scale = q * fma(-d, q, 2.0);
            }
            if (tid < l) {
                double acc = 0;
#pragma unroll
                for (int m = 0; m < PNB; ++m)
                    if (m >= tid && m < l) acc = fma(S.Tf[tid][m], g[m] * scale + S.s_vrow[m], acc);
                S.Tf[tid][l] = -tk * acc;
            } else if (tid == l) {
                S.Tf[l][l] = tk;
                tau[J.c_off + kl] = tk;
            }
            double *vk = Vall + J.x_off + kl * M;
            double *xc = Xb + kl * M;
#pragma unroll
            for (int t = 0; t < QLA_RPT; ++t) {
                const int64_t i = tid + (int64_t)t * NTQ;
                if (i < M) {
                    const double cv = c[l][t];
                    const double v = (i > kl) ? cv * scale : ((i == kl) ? 1.0 : 0.0);
                    xc[i] = (i < kl) ? cv : ((i == kl) ? beta : 0.0);
                    vk[i] = v;
                    c[l][t] = v;
                }
            }
            lds_barrier();
        }
    }
    if (tid < PNB * PNB) Tpan2[((int64_t)((kp / PNB) & 1) * n_jobs + b) * PNB * PNB + tid] = S.Tf[tid / PNB][tid % PNB];
}
