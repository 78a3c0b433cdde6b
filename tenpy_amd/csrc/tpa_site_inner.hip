// Measurement: <b| op |x_s> for a whole stack of x_s in one launch pair (tpa_site_inner_batch), gfx950.
//
// What it replaces: per started row i of MPS.correlation_function the pair tensordot(op2, C) + inner(B.conj(), Cij) of the reference
// (networks/mps.py:1312-1316) and the tensordot + inner of the one-site expectation value (:591-596) -- three passes over X = C . B per
// closing value and one host read each -- by ONE pass over the stacked X of all started rows and no host read.  HBM-bound: every x
// element is read once, every b element once per SI_S = 8 stack slots.
// Launch geometry (tests/test_conformance_site_inner.py names these numbers):
//   item     = 16 bytes in the VEC form (one complex element, or two real elements j, j + 1 of one row) -- 16-byte loads; the scalar
//              form (8-byte loads, item = one element) serves base addresses off a 16-byte boundary and, for real data, jobs with an
//              odd post, b_off, b_ld, x_off, x_ld or x_sstride (decided per job, uniform over the workgroup).
//   thread   = columns (i, item of j) of its job, grid-stride; per column and group of SI_S stack slots it loads the d_b items of b,
//              folds t_c = sum_o conj(b_o) coeff[o, c] (D = 2, 4, 8 or 16 registers pairs: the smallest that holds max_d), then streams
//              the d_x items of x of every slot of the group: acc_s += sum_c t_c x_{s, c}.  j is the fastest index: the loads of a
//              wavefront are contiguous.  coeff: the address does not depend on the lane -- uniform loads, no LDS.
//   reduce   : per group the 2 SI_S sums go through the DPP/shuffle sum of the wavefront, one LDS slot per wavefront, and threads
//              0 .. 2 SI_S - 1 add the four wavefronts in order and store the partials work[2 ((job gx + blockIdx.x) n_stack + s)].
//   grid     = (gx, n_jobs), gx = min(512, ceil(items of max_job_cols / (SI_PER_THREAD NT))); every workgroup writes all its
//              partials (zeros where it had no column).
//   pass 2   : one workgroup per output (s, k): thread t adds the partials t, t + 256, ... of the (job, workgroup) list whose job has
//              out_col == k, then the tree.  No floating-point atomics anywhere.
// Registers and occupancy: the table behind the kernel.
#include "tpa_common.h"

namespace {

constexpr int NT = 256;
constexpr int SI_S = 8;             // stack slots per pass over b
constexpr int SI_PER_THREAD = 4;    // columns per thread the grid is sized for
constexpr int SI_MAXG = 512;

struct SiJob {  // int64[12]
    int64_t b_off, b_ld, d_b, x_off, x_ld, x_sstride, d_x, pre, post, coeff_off, out_col, pad;
};

template <bool CPLX, bool VEC>
__device__ __forceinline__ double2 si_load(const double *p) {
    if (VEC) return *reinterpret_cast<const double2 *>(p);
    double2 v;
    v.x = p[0];
    v.y = CPLX ? p[1] : 0.;
    return v;
}

template <bool CPLX, int D, bool VEC>
__device__ __forceinline__ void site_inner_job(const SiJob &J, int max_d, int n_stack, const double *__restrict__ coeff,
                                               const double *b, const double *x, double *__restrict__ part, double (*red)[2 * SI_S]) {
    constexpr int W = (CPLX || VEC) ? 2 : 1;           // doubles per item
    constexpr int EPI = (!CPLX && VEC) ? 2 : 1;        // elements per item
    constexpr int CW = CPLX ? 2 : 1;                   // doubles per element
    const int d_b = (int)(J.d_b < max_d ? J.d_b : max_d), d_x = (int)(J.d_x < max_d ? J.d_x : max_d);
    const int64_t post_items = J.post > 0 ? J.post / EPI : 0;
    const int64_t n_cols = J.pre > 0 ? J.pre * post_items : 0;
    const int64_t row_d = J.post * CW;                 // doubles from (.., o, j) to (.., o + 1, j)
    const int64_t ss_d = J.x_sstride * CW;
    const double *cf = coeff + CW * J.coeff_off;
    const int ldc = (int)J.d_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s0 = 0; s0 < n_stack; s0 += SI_S) {
        const int ns = (n_stack - s0 < SI_S) ? n_stack - s0 : SI_S;
        double2 acc[SI_S];
#pragma unroll
        for (int ss = 0; ss < SI_S; ++ss) acc[ss] = double2{0., 0.};
        for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n_cols; e += (int64_t)gridDim.x * NT) {
            const int64_t i = e / post_items, jj = e - i * post_items;
            const double *bp = b + CW * (J.b_off + i * J.b_ld) + jj * W;
            double2 t[D];
#pragma unroll
            for (int c = 0; c < D; ++c) t[c] = double2{0., 0.};
#pragma unroll 1
            for (int o = 0; o < d_b; ++o) {
                const double2 bv = si_load<CPLX, VEC>(bp + o * row_d);
                const double *a = cf + CW * (o * ldc);
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    if (c < d_x) {
                        if (CPLX) {     // conj(b) a
                            t[c].x = fma(bv.x, a[2 * c], t[c].x);
                            t[c].x = fma(bv.y, a[2 * c + 1], t[c].x);
                            t[c].y = fma(bv.x, a[2 * c + 1], t[c].y);
                            t[c].y = fma(-bv.y, a[2 * c], t[c].y);
                        } else {
                            t[c].x = fma(bv.x, a[c], t[c].x);
                            if (VEC) t[c].y = fma(bv.y, a[c], t[c].y);
                        }
                    }
                }
            }
            // (the address of every load is stepped per lane: 8 D loop-invariant 64-bit offsets would not fit the scalar registers)
            const double *xs = x + CW * (J.x_off + i * J.x_ld + s0 * J.x_sstride) + jj * W;
#pragma unroll
            for (int ss = 0; ss < SI_S; ++ss) {
                if (ss < ns) {
                    const double *xc = xs;
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        if (c < d_x) {
                            const double2 xv = si_load<CPLX, VEC>(xc);
                            xc += row_d;
                            asm volatile("" : "+v"(xc));
                            if (CPLX) {
                                acc[ss].x = fma(t[c].x, xv.x, acc[ss].x);
                                acc[ss].x = fma(-t[c].y, xv.y, acc[ss].x);
                                acc[ss].y = fma(t[c].x, xv.y, acc[ss].y);
                                acc[ss].y = fma(t[c].y, xv.x, acc[ss].y);
                            } else {
                                acc[ss].x = fma(t[c].x, xv.x, acc[ss].x);
                                if (VEC) acc[ss].x = fma(t[c].y, xv.y, acc[ss].x);
                            }
                        }
                    }
                    xs += ss_d;
                    asm volatile("" : "+v"(xs));
                }
            }
        }
        // (all 256 threads are here: the loop over the columns has ended for every lane)
#pragma unroll
        for (int ss = 0; ss < SI_S; ++ss) {
            const double r = wave_sum(acc[ss].x);
            const double im = CPLX ? wave_sum(acc[ss].y) : 0.;
            if (lane == 0) {
                red[wave][2 * ss] = r;
                red[wave][2 * ss + 1] = im;
            }
        }
        __syncthreads();
        if (threadIdx.x < 2 * SI_S && (int)(threadIdx.x >> 1) < ns) {
            double v = red[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) v += red[w][threadIdx.x];
            part[2 * s0 + threadIdx.x] = v;
        }
        __syncthreads();
    }
}

template <bool CPLX, int D, bool VEC>
__global__ __launch_bounds__(NT) void site_inner_kernel(const SiJob *__restrict__ jobs, const double *__restrict__ coeff, int max_d,
                                                        int n_stack, const double *b, const double *x, double *__restrict__ work) {
    __shared__ double red[NT / 64][2 * SI_S];
    const SiJob J = jobs[blockIdx.y];
    double *part = work + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * n_stack;
    if (VEC && !CPLX) {         // two real elements per item: the whole job has to keep the items on 16-byte boundaries
        if ((J.post | J.b_off | J.b_ld | J.x_off | J.x_ld | J.x_sstride) & 1) {
            site_inner_job<CPLX, D, false>(J, max_d, n_stack, coeff, b, x, part, red);
            return;
        }
    }
    site_inner_job<CPLX, D, VEC>(J, max_d, n_stack, coeff, b, x, part, red);
}
// Resource usage on gfx950 (-Rpass-analysis=kernel-resource-usage): ScratchSize 0 and no VGPR spill in every instantiation.
//   VGPRs (waves per SIMD)   D = 2      D = 4      D = 8      D = 16
//   real,    16-byte form    47 (7)     55 (7)     72 (7)    104 (4)      (this kernel also holds the 8-byte form of the odd jobs)
//   real,     8-byte form    41 (8)     45 (8)     53 (8)     69 (7)
//   complex, either form     63 (8)     71 (7)     87 (5)    120 (4)
//   second pass: 22 VGPRs (8).  The 16-byte real form with D = 8 / 16 and the complex forms with D = 16 keep 8 / 24 and 6 scalar
//   registers in lanes of a vector register (SGPR spill to VGPR: no memory traffic).

__global__ __launch_bounds__(NT) void site_inner_final_kernel(const SiJob *__restrict__ jobs, int n_jobs, int gx, int n_stack, int n_out,
                                                              const double *__restrict__ work, double *__restrict__ out) {
    __shared__ double red[NT / 64];
    const int s = blockIdx.x / n_out, k = blockIdx.x - s * n_out;
    const int64_t total = (int64_t)n_jobs * gx;
    double sr = 0, si = 0;
    for (int64_t q = threadIdx.x; q < total; q += NT) {
        if (jobs[q / gx].out_col != k) continue;
        const double *p = work + 2 * (q * n_stack + s);
        sr += p[0];
        si += p[1];
    }
    sr = block_sum<NT>(sr, red);
    si = block_sum<NT>(si, red);
    if (threadIdx.x == 0) {
        out[2 * (int64_t)blockIdx.x] = sr;
        out[2 * (int64_t)blockIdx.x + 1] = si;
    }
}

inline int site_inner_grid(int64_t items) {
    int64_t g = (items + (int64_t)NT * SI_PER_THREAD - 1) / ((int64_t)NT * SI_PER_THREAD);
    if (g < 1) g = 1;
    if (g > SI_MAXG) g = SI_MAXG;
    return (int)g;
}

template <bool CPLX, bool VEC>
void site_inner_launch(int max_d, dim3 grid, hipStream_t st, const int64_t *jobs_dev, const void *coeff_dev, int n_stack, const void *b_base,
                       const void *x_base, double *work_dev) {
    const SiJob *jobs = (const SiJob *)jobs_dev;
    const double *coeff = (const double *)coeff_dev, *b = (const double *)b_base, *x = (const double *)x_base;
    if (max_d <= 2)
        site_inner_kernel<CPLX, 2, VEC><<<grid, NT, 0, st>>>(jobs, coeff, max_d, n_stack, b, x, work_dev);
    else if (max_d <= 4)
        site_inner_kernel<CPLX, 4, VEC><<<grid, NT, 0, st>>>(jobs, coeff, max_d, n_stack, b, x, work_dev);
    else if (max_d <= 8)
        site_inner_kernel<CPLX, 8, VEC><<<grid, NT, 0, st>>>(jobs, coeff, max_d, n_stack, b, x, work_dev);
    else
        site_inner_kernel<CPLX, 16, VEC><<<grid, NT, 0, st>>>(jobs, coeff, max_d, n_stack, b, x, work_dev);
}

}  // namespace

extern "C" int64_t tpa_site_inner_work(int n_jobs, int n_stack, int n_out, int64_t max_job_cols) {
    (void)n_out;
    if (n_jobs <= 0 || n_stack <= 0) return 0;
    return 2 * (int64_t)n_jobs * site_inner_grid(max_job_cols) * n_stack;
}

extern "C" int tpa_site_inner_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const void *coeff_dev, int max_d, int n_stack, int n_out,
                                    int64_t max_job_cols, const void *b_base, const void *x_base, double *out_dev, double *work_dev,
                                    void *stream) {
    static_assert(TPA_MPO_APPLY_MAXD == 16, "site_inner_launch dispatches up to 16 folded values");
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(max_d >= 1 && max_d <= TPA_MPO_APPLY_MAXD);
    TPA_ARG_CHECK(n_stack >= 1 && n_out >= 1 && out_dev != nullptr);
    hipStream_t st = (hipStream_t)stream;
    if (n_jobs <= 0) {
        TPA_HIP_CHECK(hipMemsetAsync(out_dev, 0, sizeof(double) * 2 * (size_t)n_stack * (size_t)n_out, st));
        return 0;
    }
    TPA_ARG_CHECK(n_jobs <= 65535);
    TPA_ARG_CHECK(jobs_dev != nullptr && coeff_dev != nullptr && b_base != nullptr && x_base != nullptr && work_dev != nullptr);
    TPA_ARG_CHECK((int64_t)n_stack * n_out <= 0x7fffffff);
    const bool aligned = (((uintptr_t)b_base | (uintptr_t)x_base) & 15) == 0;
    const int64_t items = (dtype == TPA_F64 && aligned) ? (max_job_cols + 1) / 2 : max_job_cols;
    const int gx = site_inner_grid(items);      // (<= the gx of tpa_site_inner_work: the partials fit)
    dim3 grid(gx, n_jobs);
    if (dtype == TPA_F64) {
        if (aligned)
            site_inner_launch<false, true>(max_d, grid, st, jobs_dev, coeff_dev, n_stack, b_base, x_base, work_dev);
        else
            site_inner_launch<false, false>(max_d, grid, st, jobs_dev, coeff_dev, n_stack, b_base, x_base, work_dev);
    } else {
        if (aligned)
            site_inner_launch<true, true>(max_d, grid, st, jobs_dev, coeff_dev, n_stack, b_base, x_base, work_dev);
        else
            site_inner_launch<true, false>(max_d, grid, st, jobs_dev, coeff_dev, n_stack, b_base, x_base, work_dev);
    }
    TPA_LAUNCH_CHECK();
    site_inner_final_kernel<<<n_stack * n_out, NT, 0, st>>>((const SiJob *)jobs_dev, n_jobs, gx, n_stack, n_out, work_dev, out_dev);
    TPA_LAUNCH_CHECK();
    return 0;
}
