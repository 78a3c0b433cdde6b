// Projective sampling of an MPS: the Born probabilities and the outcome of every row of a stack in one launch
// (tpa_sample_select_batch) and the chosen, normalised slices written into the next stack (tpa_sample_gather_batch), gfx950.
//
// What it replaces: per (sample, site) of MPS.sample_measurements (reference networks/mps.py:4403-4433) the statements
// tensordot(theta.conj(), theta) + to_ndarray (a host read) + rng.choice + take_slice + norm (a host read) + theta / norm -- about ten
// launches on a vector of chi numbers -- by two launches per SITE for all samples.  HBM-bound: every x element is read once by the
// select kernel, the chosen 1 / d of them a second time by the gather kernel.
// Launch geometry of the select kernel (tests/test_conformance_sample.py names these numbers):
//   workgroup = 256 threads = 4 wavefronts, one ROW of the stack at a time, grid-stride over the rows (grid = min(n_rows_total, 2048)).
//               The group of a row is found by a scan of the group table (addresses do not depend on the lane: uniform loads).
//   item      = 16 bytes in the VEC form (one complex element, or two real elements j, j + 1 of one slice) -- 16-byte loads; the
//               8-byte form (item = one real number) serves an x_base off a 16-byte boundary and, for real data, segs with an odd
//               post, x_off or x_ld (decided per seg, uniform over the workgroup).
//   thread    = items t, t + 256, ... of the slice (seg, c) -- j is the fastest index: the loads of a wavefront are contiguous --
//               summed as fma(re, re, acc), fma(im, im, acc) in one accumulator.
//   reduce    : per slice the DPP/shuffle sum of the wavefront, lane 0 stores LDS pw[wave][sigma]; pw is zeroed per row, so a sigma
//               that no seg covers keeps an exact 0.  After one barrier thread 0 adds the four wavefronts in order, p[sigma] =
//               ((pw0 + pw1) + pw2) + pw3, then total, the cdf and the outcome sequentially in ascending sigma, and stores the row of out.
//   No floating-point atomics, no work area: two identical calls give identical bits.
// Gather kernel: one wavefront per row of the table (4 per workgroup of 256 threads, grid = min(ceil(n_rows / 4), 2048), grid-stride),
// lane l the doubles l, l + 64, ...; 16-byte loads and stores where source and destination of the row are both 16-byte aligned.
// Registers: the note behind each kernel.
#include <math.h>

#include "tpa_common.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int SAMPLE_MAXG = 2048;

struct SampleSeg {  // int64[8]
    int64_t x_off, x_ld, d, post, sigma0, pad0, pad1, pad2;
};
struct SampleGroup {  // int64[4]
    int64_t seg_first, seg_count, row_first, n_rows;
};
struct GatherRow {  // int64[4]
    int64_t src_off, len, dst_off, out_row;
};

template <bool VEC>
__device__ __forceinline__ double slice_sqnorm(const double *p, int64_t n_doubles) {
    double acc = 0.;
    if (VEC) {
        const int64_t n_items = n_doubles >> 1;
        for (int64_t t = threadIdx.x; t < n_items; t += NT) {
            const double2 v = *reinterpret_cast<const double2 *>(p + 2 * t);
            acc = fma(v.x, v.x, acc);
            acc = fma(v.y, v.y, acc);
        }
    } else {
        for (int64_t t = threadIdx.x; t < n_doubles; t += NT) {
            const double v = p[t];
            acc = fma(v, v, acc);
        }
    }
    return acc;
}

template <bool CPLX>
__global__ __launch_bounds__(NT) void sample_select_kernel(const SampleSeg *__restrict__ segs, int n_segs,
                                                           const SampleGroup *__restrict__ groups, int n_groups, int dim,
                                                           int64_t n_rows_total, const double *x, const double *__restrict__ u,
                                                           double *__restrict__ out) {
    constexpr int CW = CPLX ? 2 : 1;  // doubles per element
    __shared__ double pw[NW][TPA_SAMPLE_MAX_DIM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool base_aligned = ((uintptr_t)x & 15) == 0;
    for (int64_t r = blockIdx.x; r < n_rows_total; r += gridDim.x) {
        static_assert(NW * TPA_SAMPLE_MAX_DIM == NT, "one thread zeroes one slot of pw");
        pw[threadIdx.x / TPA_SAMPLE_MAX_DIM][threadIdx.x % TPA_SAMPLE_MAX_DIM] = 0.;
        __syncthreads();
        int g = -1;
        for (int k = 0; k < n_groups; ++k) {
            const int64_t r0 = groups[k].row_first;
            if (g < 0 && r >= r0 && r - r0 < groups[k].n_rows) g = k;
        }
        if (g >= 0) {
            const SampleGroup G = groups[g];
            const int64_t i = r - G.row_first;
            for (int64_t s = G.seg_first; s < G.seg_first + G.seg_count; ++s) {
                if (s < 0 || s >= n_segs) continue;
                const SampleSeg S = segs[s];
                if (S.post <= 0) continue;
                const bool vec = base_aligned && (CPLX || ((S.post | S.x_off | S.x_ld) & 1) == 0);
                for (int64_t c = 0; c < S.d; ++c) {
                    const int64_t sigma = S.sigma0 + c;
                    if (sigma < 0 || sigma >= dim) continue;  // (never outside pw)
                    const double *p = x + CW * (S.x_off + i * S.x_ld + c * S.post);
                    const double part = vec ? slice_sqnorm<true>(p, CW * S.post) : slice_sqnorm<false>(p, CW * S.post);
                    const double sum = wave_sum(part);  // (all 64 lanes are here: the conditions above are uniform)
                    if (lane == 0) pw[wave][sigma] = sum;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double total = 0.;
            for (int s = 0; s < dim; ++s) {
                double p = pw[0][s];
#pragma unroll
                for (int w = 1; w < NW; ++w) p += pw[w][s];
                pw[0][s] = p;
                total += p;
            }
            double sigma = -1., wgt = 0.;
            if (total > 0. && isfinite(total)) {
                const double uu = u[r];
                double run = 0.;
                int count = 0, last = 0;
                for (int s = 0; s < dim; ++s) {
                    const double p = pw[0][s];
                    run += p;
                    if (run / total <= uu) ++count;
                    if (p > 0.) last = s;
                }
                const int pick = count < last ? count : last;
                sigma = (double)pick;
                wgt = sqrt(pw[0][pick]);
            }
            double *o = out + 4 * r;
            o[0] = sigma;
            o[1] = wgt;
            o[2] = total;
            o[3] = 0.;
        }
        __syncthreads();  // (pw is zeroed again for the next row)
    }
}
// Resource usage on gfx950 (-Rpass-analysis=kernel-resource-usage): 86 VGPRs (5 waves per SIMD), 2048 bytes of LDS, ScratchSize 0 and no
// spill in both instantiations; the gather kernel below: 48 VGPRs (8 waves per SIMD), no LDS, ScratchSize 0.

__global__ __launch_bounds__(NT) void sample_gather_kernel(const GatherRow *__restrict__ rows, int64_t n_rows, int cw, const double *src,
                                                           const double *__restrict__ out, double *dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = (int64_t)blockIdx.x * NW + wave; q < n_rows; q += (int64_t)gridDim.x * NW) {
        const GatherRow R = rows[q];
        if (R.len <= 0) continue;
        const double w = out[4 * R.out_row + 1];
        const double *s = src + cw * R.src_off;
        double *d = dst + cw * R.dst_off;
        const int64_t n = cw * R.len;
        if (((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0) {
            const int64_t n2 = n >> 1;
            for (int64_t t = lane; t < n2; t += 64) {
                double2 v = *reinterpret_cast<const double2 *>(s + 2 * t);
                v.x /= w;
                v.y /= w;
                *reinterpret_cast<double2 *>(d + 2 * t) = v;
            }
            if ((n & 1) && lane == 0) d[n - 1] = s[n - 1] / w;
        } else {
            for (int64_t t = lane; t < n; t += 64) d[t] = s[t] / w;
        }
    }
}

}  // namespace

extern "C" int tpa_sample_select_batch(int dtype, const int64_t *segs_dev, int n_segs, const int64_t *groups_dev, int n_groups, int dim,
                                       int64_t n_rows_total, const void *x_base, const double *u_dev, double *out_dev, void *stream) {
    static_assert(TPA_SAMPLE_MAX_DIM == 64, "the select kernel zeroes its LDS table with one thread per slot");
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(dim >= 1 && dim <= TPA_SAMPLE_MAX_DIM);
    TPA_ARG_CHECK(n_segs >= 0 && n_groups >= 0);
    if (n_rows_total <= 0) return 0;
    TPA_ARG_CHECK(segs_dev != nullptr && groups_dev != nullptr && x_base != nullptr && u_dev != nullptr && out_dev != nullptr);
    const int grid = (int)(n_rows_total < SAMPLE_MAXG ? n_rows_total : SAMPLE_MAXG);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        sample_select_kernel<false><<<grid, NT, 0, st>>>((const SampleSeg *)segs_dev, n_segs, (const SampleGroup *)groups_dev, n_groups, dim,
                                                         n_rows_total, (const double *)x_base, u_dev, out_dev);
    else
        sample_select_kernel<true><<<grid, NT, 0, st>>>((const SampleSeg *)segs_dev, n_segs, (const SampleGroup *)groups_dev, n_groups, dim,
                                                        n_rows_total, (const double *)x_base, u_dev, out_dev);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_sample_gather_batch(int dtype, const int64_t *rows_dev, int64_t n_rows, const void *src_base, const double *out_dev,
                                       void *dst_base, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_rows <= 0) return 0;
    TPA_ARG_CHECK(rows_dev != nullptr && src_base != nullptr && out_dev != nullptr && dst_base != nullptr);
    TPA_ARG_CHECK(src_base != dst_base);
    const int64_t blocks = (n_rows + NW - 1) / NW;
    const int grid = (int)(blocks < SAMPLE_MAXG ? blocks : SAMPLE_MAXG);
    sample_gather_kernel<<<grid, NT, 0, (hipStream_t)stream>>>((const GatherRow *)rows_dev, n_rows, dtype == TPA_C128 ? 2 : 1,
                                                              (const double *)src_base, out_dev, (double *)dst_base);
    TPA_LAUNCH_CHECK();
    return 0;
}
