// Measurement: the closing step of a reduced density matrix with the physical index pair left OPEN, for a whole stack of rows in one
// launch pair (tpa_site_rho_batch), gfx950.
//
// What it replaces: per pair (i, j) of MPS.mutinf_two_site the closing tensordot(rho, B.conj(), [['vR*', 'vR'], ['vL*', 'vR*']]) of the
// reference (networks/mps.py:4218-4232) -- a GEMM that is only d^2 rows tall, one per pair, followed by a host read -- and, with
// x = b = theta_i, the one-site density matrix of get_rho_segment (:4004).  Closing the stacked X = C . B_j of all open rows with
// tpa_site_inner_batch and the d^2 matrix units |o><c| would stream X d^2 times; here every x element is read ONCE per launch and every
// b element once per group of S stack slots, and all d_b d_x sums of a column are kept in registers.  HBM-bound.
// Launch geometry (tests/test_conformance_site_rho.py names these numbers):
//   item     = 16 bytes in the VEC form (one complex element, or two real elements j, j + 1 of one row) -- 16-byte loads; the scalar
//              form (8-byte loads, item = one element) serves base addresses off a 16-byte boundary and, for real data, jobs with an
//              odd post, b_off, b_ld, x_off, x_ld or x_sstride (decided per job, uniform over the workgroup).
//   thread   = columns (i, item of j) of its job, grid-stride; per column and group of S stack slots it loads the d_b items of b, then
//              streams the d_x items of x of every slot of the group: acc[s][o][c] += conj(b_o) x_{s, c} -- S D D accumulators, D = 1, 2
//              or 4 the smallest that holds max_d, S = 8, 4, 2 for D = 1, 2, 4.  j is the fastest index: the loads of a wavefront are
//              contiguous.
//   reduce   : per group the S D D sums go through the DPP/shuffle sum of the wavefront, one LDS slot per wavefront, and the first
//              threads add the four wavefronts in order and store the partials
//              work[2 (((job gx + blockIdx.x) n_stack + s) T + o d_x + c)], T = min(16, out_size).
//   grid     = (gx, n_jobs), gx = min(256, ceil(items of max_job_cols / (SR_PER_THREAD NT))); every workgroup writes all its partials
//              (zeros where it had no column).
//   pass 2   : one workgroup per output (s, e), e < out_size: thread t adds the partials t, t + 256, ... of the (job, workgroup) list
//              whose job's tile holds e (several jobs may), then the tree.  A gather: nothing outside out[0 : 2 n_stack out_size] can be
//              written whatever the table says.  No floating-point atomics anywhere.  Cost: every one of the n_stack out_size
//              workgroups scans the whole list of n_jobs gx entries and rereads the job table, n_stack out_size n_jobs gx tile tests in
//              all -- 256 workgroups x 5376 entries on the chi = 2048 chain of scripts/mutinf_bench.py, inside the 0.29 ms of the launch pair there; it grows
//              with the product, and a structure of tens of thousands of jobs under a ring of hundreds of d = 4 slots would spend
//              longer here than in the first pass (a job list per tile would bound it: not built, nothing of that shape is measured).
// Registers and occupancy: the table behind the kernel.
#include "tpa_common.h"

namespace {

constexpr int NT = 256;
constexpr int SR_PER_THREAD = 4;    // columns per thread the grid is sized for
constexpr int SR_MAXG = 256;
constexpr int SR_MAXD = 4;          // widest physical sector served
constexpr int SR_MAXT = SR_MAXD * SR_MAXD;

constexpr int sr_slots(int D) { return D == 1 ? 8 : D == 2 ? 4 : 2; }      // stack slots per pass over b

struct SrJob {  // int64[12]
    int64_t b_off, b_ld, d_b, x_off, x_ld, x_sstride, d_x, pre, post, out_off, out_ld, pad;
};

template <bool CPLX, bool VEC>
__device__ __forceinline__ double2 sr_load(const double *p) {
    if (VEC) return *reinterpret_cast<const double2 *>(p);
    double2 v;
    v.x = p[0];
    v.y = CPLX ? p[1] : 0.;
    return v;
}

template <bool CPLX, int D, bool VEC>
__device__ __forceinline__ void site_rho_job(const SrJob &J, int max_d, int n_stack, int T, const double *b, const double *x,
                                             double *__restrict__ part, double (*red)[2 * sr_slots(D) * D * D]) {
    constexpr int S = sr_slots(D);
    constexpr int W = (CPLX || VEC) ? 2 : 1;           // doubles per item
    constexpr int EPI = (!CPLX && VEC) ? 2 : 1;        // elements per item
    constexpr int CW = CPLX ? 2 : 1;                   // doubles per element
    const int d_b = (int)(J.d_b < max_d ? J.d_b : max_d), d_x = (int)(J.d_x < max_d ? J.d_x : max_d);
    const int64_t post_items = J.post > 0 ? J.post / EPI : 0;
    const int64_t n_cols = J.pre > 0 ? J.pre * post_items : 0;
    const int64_t row_d = J.post * CW;                 // doubles from (.., o, j) to (.., o + 1, j)
    const int64_t ss_d = J.x_sstride * CW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s0 = 0; s0 < n_stack; s0 += S) {
        const int ns = (n_stack - s0 < S) ? n_stack - s0 : S;
        double2 acc[S][D][D];
#pragma unroll
        for (int ss = 0; ss < S; ++ss)
#pragma unroll
            for (int o = 0; o < D; ++o)
#pragma unroll
                for (int c = 0; c < D; ++c) acc[ss][o][c] = double2{0., 0.};
        for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n_cols; e += (int64_t)gridDim.x * NT) {
            const int64_t i = e / post_items, jj = e - i * post_items;
            const double *bp = b + CW * (J.b_off + i * J.b_ld) + jj * W;
            double2 bv[D];
#pragma unroll
            for (int o = 0; o < D; ++o) {
                bv[o] = double2{0., 0.};
                if (o < d_b) bv[o] = sr_load<CPLX, VEC>(bp + o * row_d);
            }
            const double *xs = x + CW * (J.x_off + i * J.x_ld + s0 * J.x_sstride) + jj * W;
#pragma unroll
            for (int ss = 0; ss < S; ++ss) {
                if (ss < ns) {
                    const double *xc = xs;
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        if (c < d_x) {
                            const double2 xv = sr_load<CPLX, VEC>(xc);
                            xc += row_d;
#pragma unroll
                            for (int o = 0; o < D; ++o) {       // (rows o >= d_b: bv = 0, their sums are never stored)
                                if (CPLX) {     // conj(b) x
                                    acc[ss][o][c].x = fma(bv[o].x, xv.x, acc[ss][o][c].x);
                                    acc[ss][o][c].x = fma(bv[o].y, xv.y, acc[ss][o][c].x);
                                    acc[ss][o][c].y = fma(bv[o].x, xv.y, acc[ss][o][c].y);
                                    acc[ss][o][c].y = fma(-bv[o].y, xv.x, acc[ss][o][c].y);
                                } else {
                                    acc[ss][o][c].x = fma(bv[o].x, xv.x, acc[ss][o][c].x);
                                    if (VEC) acc[ss][o][c].x = fma(bv[o].y, xv.y, acc[ss][o][c].x);
                                }
                            }
                        }
                    }
                    xs += ss_d;
                }
            }
        }
        // (all 256 threads are here: the loop over the columns has ended for every lane)
#pragma unroll
        for (int ss = 0; ss < S; ++ss)
#pragma unroll
            for (int o = 0; o < D; ++o)
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const double r = wave_sum(acc[ss][o][c].x);
                    const double im = CPLX ? wave_sum(acc[ss][o][c].y) : 0.;
                    if (lane == 0) {
                        red[wave][2 * ((ss * D + o) * D + c)] = r;
                        red[wave][2 * ((ss * D + o) * D + c) + 1] = im;
                    }
                }
        __syncthreads();
        if (threadIdx.x < 2 * S * D * D) {
            const int q = threadIdx.x >> 1, ss = q / (D * D), o = (q / D) % D, c = q % D;
            const int t = o * d_x + c;
            if (ss < ns && o < d_b && c < d_x && t < T) {
                double v = red[0][threadIdx.x];
#pragma unroll
                for (int w = 1; w < NT / 64; ++w) v += red[w][threadIdx.x];
                part[2 * ((int64_t)(s0 + ss) * T + t) + (threadIdx.x & 1)] = v;
            }
        }
        __syncthreads();
    }
}

template <bool CPLX, int D, bool VEC>
__global__ __launch_bounds__(NT) void site_rho_kernel(const SrJob *__restrict__ jobs, int max_d, int n_stack, int T, const double *b,
                                                      const double *x, double *__restrict__ work) {
    __shared__ double red[NT / 64][2 * sr_slots(D) * D * D];
    const SrJob J = jobs[blockIdx.y];
    double *part = work + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * n_stack * T;
    if (VEC && !CPLX) {         // two real elements per item: the whole job has to keep the items on 16-byte boundaries
        if ((J.post | J.b_off | J.b_ld | J.x_off | J.x_ld | J.x_sstride) & 1) {
            site_rho_job<CPLX, D, false>(J, max_d, n_stack, T, b, x, part, red);
            return;
        }
    }
    site_rho_job<CPLX, D, VEC>(J, max_d, n_stack, T, b, x, part, red);
}
// Resource usage on gfx950 (-Rpass-analysis=kernel-resource-usage): ScratchSize 0 and no VGPR spill in every instantiation.
//   VGPRs (waves per SIMD)   D = 1, S = 8   D = 2, S = 4   D = 4, S = 2
//   real,    16-byte form      44 (8)         61 (8)        106 (4)      (this kernel also holds the 8-byte form of the odd jobs)
//   real,     8-byte form      39 (8)         57 (8)         93 (5)
//   complex, either form       60 (8)         93 (5)        170 (2)
//   second pass: 26 VGPRs (8).  S from the accumulators, 2 S D D registers for real and 4 S D D for complex data: 16 / 32 / 64 and
//   32 / 64 / 128 of them.  S = 4 at D = 4 would take 256 accumulator registers for complex data (one wave per SIMD); with S = 2 the
//   widest form still runs two, each with up to S d_x = 8 independent 16-byte loads in flight per lane.

// The entry (o, c) of the tile of job J that is the output entry e, as its index in the job's partials; -1: the tile does not hold e.
__device__ __forceinline__ int sr_tile_entry(const SrJob &J, int max_d, int T, int e) {
    const int64_t r = (int64_t)e - J.out_off;
    if (r < 0 || J.out_ld <= 0 || J.pre <= 0 || J.post <= 0) return -1;
    const int64_t o = r / J.out_ld, c = r - o * J.out_ld;
    const int64_t d_b = J.d_b < max_d ? J.d_b : max_d, d_x = J.d_x < max_d ? J.d_x : max_d;
    if (o >= d_b || c >= d_x) return -1;
    const int64_t t = o * d_x + c;
    return t < T ? (int)t : -1;
}

__global__ __launch_bounds__(NT) void site_rho_final_kernel(const SrJob *__restrict__ jobs, int n_jobs, int gx, int max_d, int n_stack,
                                                            int out_size, int T, const double *__restrict__ work,
                                                            double *__restrict__ out) {
    __shared__ double red[NT / 64];
    const int s = blockIdx.x / out_size, e = blockIdx.x - s * out_size;
    const int64_t total = (int64_t)n_jobs * gx;
    double sr = 0, si = 0;
    for (int64_t q = threadIdx.x; q < total; q += NT) {
        const int t = sr_tile_entry(jobs[q / gx], max_d, T, e);
        if (t < 0) continue;
        const double *p = work + 2 * ((q * n_stack + s) * T + t);
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

inline int site_rho_grid(int64_t items) {
    int64_t g = (items + (int64_t)NT * SR_PER_THREAD - 1) / ((int64_t)NT * SR_PER_THREAD);
    if (g < 1) g = 1;
    if (g > SR_MAXG) g = SR_MAXG;
    return (int)g;
}

inline int site_rho_tile(int out_size) { return out_size < SR_MAXT ? out_size : SR_MAXT; }

template <bool CPLX, bool VEC>
void site_rho_launch(int max_d, dim3 grid, hipStream_t st, const int64_t *jobs_dev, int n_stack, int T, const void *b_base,
                     const void *x_base, double *work_dev) {
    const SrJob *jobs = (const SrJob *)jobs_dev;
    const double *b = (const double *)b_base, *x = (const double *)x_base;
    if (max_d <= 1)
        site_rho_kernel<CPLX, 1, VEC><<<grid, NT, 0, st>>>(jobs, max_d, n_stack, T, b, x, work_dev);
    else if (max_d <= 2)
        site_rho_kernel<CPLX, 2, VEC><<<grid, NT, 0, st>>>(jobs, max_d, n_stack, T, b, x, work_dev);
    else
        site_rho_kernel<CPLX, 4, VEC><<<grid, NT, 0, st>>>(jobs, max_d, n_stack, T, b, x, work_dev);
}

}  // namespace

extern "C" int64_t tpa_site_rho_work(int n_jobs, int n_stack, int out_size, int64_t max_job_cols) {
    if (n_jobs <= 0 || n_stack <= 0 || out_size <= 0) return 0;
    return 2 * (int64_t)n_jobs * site_rho_grid(max_job_cols) * n_stack * site_rho_tile(out_size);
}

extern "C" int tpa_site_rho_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int max_d, int n_stack, int out_size,
                                  int64_t max_job_cols, const void *b_base, const void *x_base, double *out_dev, double *work_dev,
                                  void *stream) {
    static_assert(TPA_SITE_RHO_MAXD == SR_MAXD, "site_rho_launch dispatches sectors up to 4 wide");
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(max_d >= 1 && max_d <= TPA_SITE_RHO_MAXD);
    TPA_ARG_CHECK(n_stack >= 1 && out_size >= 1 && out_dev != nullptr);
    TPA_ARG_CHECK((int64_t)n_stack * out_size <= 0x7fffffff);
    hipStream_t st = (hipStream_t)stream;
    if (n_jobs <= 0) {
        TPA_HIP_CHECK(hipMemsetAsync(out_dev, 0, sizeof(double) * 2 * (size_t)n_stack * (size_t)out_size, st));
        return 0;
    }
    TPA_ARG_CHECK(n_jobs <= 65535);
    TPA_ARG_CHECK(jobs_dev != nullptr && b_base != nullptr && x_base != nullptr && work_dev != nullptr);
    const bool aligned = (((uintptr_t)b_base | (uintptr_t)x_base) & 15) == 0;
    const int64_t items = (dtype == TPA_F64 && aligned) ? (max_job_cols + 1) / 2 : max_job_cols;
    const int gx = site_rho_grid(items);        // (<= the gx of tpa_site_rho_work: the partials fit)
    const int T = site_rho_tile(out_size);
    dim3 grid(gx, n_jobs);
    if (dtype == TPA_F64) {
        if (aligned)
            site_rho_launch<false, true>(max_d, grid, st, jobs_dev, n_stack, T, b_base, x_base, work_dev);
        else
            site_rho_launch<false, false>(max_d, grid, st, jobs_dev, n_stack, T, b_base, x_base, work_dev);
    } else {
        if (aligned)
            site_rho_launch<true, true>(max_d, grid, st, jobs_dev, n_stack, T, b_base, x_base, work_dev);
        else
            site_rho_launch<true, false>(max_d, grid, st, jobs_dev, n_stack, T, b_base, x_base, work_dev);
    }
    TPA_LAUNCH_CHECK();
    site_rho_final_kernel<<<n_stack * out_size, NT, 0, st>>>((const SrJob *)jobs_dev, n_jobs, gx, max_d, n_stack, out_size, T, work_dev,
                                                             out_dev);
    TPA_LAUNCH_CHECK();
    return 0;
}
