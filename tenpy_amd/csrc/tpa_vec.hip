// K2-K4: vector kernels over packed block arenas (HBM-bound), gfx950.
//
// An Array's blocks are packed back to back in one arena, so when two Arrays share the same block
// structure (always true inside a Lanczos run) the block-wise BLAS-1 loops of the reference
// (_inner_worker _npc_helper.pyx:1791-1875, _blas_inpl_add :316, _blas_inpl_scale :339,
// Array.norm np_conserved.py:2241-2255) collapse to ONE flat pass over the arena.
// Reductions are deterministic: pass 1 writes one partial per workgroup, pass 2 (one workgroup)
// sums them in a fixed order.
#include "tpa_common.h"
#include <vector>

namespace {

constexpr int NT = 256;
constexpr int MAXBLK = 1024;  // partials per reduction (<= TPA_RED_SCRATCH / 2)

__host__ inline int grid_for(int64_t n, int per_thread) {
    int64_t g = (n + (int64_t)NT * per_thread - 1) / ((int64_t)NT * per_thread);
    if (g < 1) g = 1;
    if (g > MAXBLK) g = MAXBLK;
    return (int)g;
}

// ---- y += alpha x ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void axpy_f64(int64_t n, double a, const double *__restrict__ x,
                                               double *__restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        y[i] = fma(a, x[i], y[i]);
}
__global__ __launch_bounds__(NT) void axpy_c128(int64_t n, double ar, double ai,
                                                const double2 *__restrict__ x,
                                                double2 *__restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        double2 xv = x[i], yv = y[i];
        yv.x += ar * xv.x - ai * xv.y;
        yv.y += ar * xv.y + ai * xv.x;
        y[i] = yv;
    }
}
__global__ __launch_bounds__(NT) void scal_f64(int64_t n, double a, double *__restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        x[i] *= a;
}
__global__ __launch_bounds__(NT) void scal_c128(int64_t n, double ar, double ai,
                                                double2 *__restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        double2 v = x[i];
        x[i] = double2{ar * v.x - ai * v.y, ar * v.y + ai * v.x};
    }
}

// ---- reductions -------------------------------------------------------------------------------
// mode 0: dot(x,y) real; 1: sum conj(x) y (complex); 2: sum x y (complex, no conj); 3: sum |x|^2
template <int MODE>
__global__ __launch_bounds__(NT) void reduce_pass1(int64_t n, const double *__restrict__ x,
                                                   const double *__restrict__ y,
                                                   double *__restrict__ partial) {
    __shared__ double red[NT / 64];
    double sr = 0, si = 0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        if (MODE == 0) {
            sr = fma(x[i], y[i], sr);
        } else if (MODE == 3) {
            sr = fma(x[i], x[i], sr);
        } else {
            const double2 a = reinterpret_cast<const double2 *>(x)[i];
            const double2 b = reinterpret_cast<const double2 *>(y)[i];
            if (MODE == 1) {  // conj(a) * b
                sr += a.x * b.x + a.y * b.y;
                si += a.x * b.y - a.y * b.x;
            } else {
                sr += a.x * b.x - a.y * b.y;
                si += a.x * b.y + a.y * b.x;
            }
        }
    }
    sr = block_sum<NT>(sr, red);
    if (MODE == 1 || MODE == 2) si = block_sum<NT>(si, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sr;
        partial[2 * blockIdx.x + 1] = si;
    }
}

__global__ __launch_bounds__(NT) void reduce_pass2(int nblk, const double *__restrict__ partial,
                                                   double *__restrict__ out) {
    __shared__ double red[NT / 64];
    double sr = 0, si = 0;
    for (int i = threadIdx.x; i < nblk; i += NT) {
        sr += partial[2 * i];
        si += partial[2 * i + 1];
    }
    sr = block_sum<NT>(sr, red);
    si = block_sum<NT>(si, red);
    if (threadIdx.x == 0) {
        out[0] = sr;
        out[1] = si;
    }
}

// ---- fused Lanczos three-term recurrence: w -= a v1 ; w -= b v0 ; partial |w|^2 ----------------
template <bool CPLX, bool HAVE_V0>
__global__ __launch_bounds__(NT) void lanczos_update_kernel(int64_t n, double *__restrict__ w,
                                                            double ar, double ai,
                                                            const double *__restrict__ v1, double br,
                                                            double bi, const double *__restrict__ v0,
                                                            double *__restrict__ partial) {
    __shared__ double red[NT / 64];
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        if (!CPLX) {
            double t = w[i];
            t = fma(-ar, v1[i], t);
            if (HAVE_V0) t = fma(-br, v0[i], t);
            w[i] = t;
            s = fma(t, t, s);
        } else {
            double2 t = reinterpret_cast<double2 *>(w)[i];
            const double2 p = reinterpret_cast<const double2 *>(v1)[i];
            t.x -= ar * p.x - ai * p.y;
            t.y -= ar * p.y + ai * p.x;
            if (HAVE_V0) {
                const double2 q = reinterpret_cast<const double2 *>(v0)[i];
                t.x -= br * q.x - bi * q.y;
                t.y -= br * q.y + bi * q.x;
            }
            reinterpret_cast<double2 *>(w)[i] = t;
            s += t.x * t.x + t.y * t.y;
        }
    }
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s;
        partial[2 * blockIdx.x + 1] = 0;
    }
}

// ---- one Lanczos step with device-resident scalars (no host round trip between the kernels) ----------------------------
// alpha comes from ab[0] (written by the dot reduction just before), beta_prev = sqrt(bsq_prev[0]) from the previous step.
template <bool CPLX, bool HAVE_V0>
__global__ __launch_bounds__(NT) void lanczos_update_dev_kernel(int64_t n, double *__restrict__ w,
                                                                const double *__restrict__ ab,
                                                                const double *__restrict__ v1,
                                                                const double *__restrict__ bsq_prev,
                                                                const double *__restrict__ v0,
                                                                double *__restrict__ partial) {
    __shared__ double red[NT / 64];
    const double ar = ab[0];
    const double br = HAVE_V0 ? sqrt(bsq_prev[0]) : 0.0;
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        if (!CPLX) {
            double t = w[i];
            t = fma(-ar, v1[i], t);
            if (HAVE_V0) t = fma(-br, v0[i], t);
            w[i] = t;
            s = fma(t, t, s);
        } else {
            double2 t = reinterpret_cast<double2 *>(w)[i];
            const double2 p = reinterpret_cast<const double2 *>(v1)[i];
            t.x -= ar * p.x;
            t.y -= ar * p.y;
            if (HAVE_V0) {
                const double2 q = reinterpret_cast<const double2 *>(v0)[i];
                t.x -= br * q.x;
                t.y -= br * q.y;
            }
            reinterpret_cast<double2 *>(w)[i] = t;
            s += t.x * t.x + t.y * t.y;
        }
    }
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s;
        partial[2 * blockIdx.x + 1] = 0;
    }
}

// second pass of the norm: out[1] = sum of the partials (out[0] keeps alpha)
__global__ __launch_bounds__(NT) void reduce_pass2_to(int nblk, const double *__restrict__ partial, double *__restrict__ out) {
    __shared__ double red[NT / 64];
    double sr = 0;
    for (int i = threadIdx.x; i < nblk; i += NT) sr += partial[2 * i];
    sr = block_sum<NT>(sr, red);
    if (threadIdx.x == 0) out[0] = sr;
}

// x *= 1 / sqrt(bsq[0])  (x as flat doubles; nothing happens for bsq <= 0)
__global__ __launch_bounds__(NT) void scal_rsqrt_dev_kernel(int64_t nd, double *__restrict__ x, const double *__restrict__ bsq) {
    const double b = bsq[0];
    if (!(b > 0.0)) return;
    const double f = 1.0 / sqrt(b);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nd; i += (int64_t)gridDim.x * NT) x[i] *= f;
}

// ---- dst = src - sum_j <b_j|src> b_j over m packed vectors (classical Gram-Schmidt, coefficients stay on the device) ---------------
// What it replaces: the m (npc.inner + iadd_prefactor_other) pairs of OrthogonalNpcLinearOperator.matvec (reference sparse.py:243-255)
// and of the re-orthogonalisation of a Lanczos step (reference krylov_based.py:667-669) -- m host reads, 5 m itemsize n bytes -- by three passes
// over itemsize n (2 m + ceil(m / PJ_J) + 2) bytes without a host read.
// Launch geometry (tests/test_conformance_project.py computes its bounds from these numbers):
//   item     = 16 bytes (one complex element, or two real ones) in the VEC form -- 16-byte loads and stores; the scalar form (8-byte
//              loads; item = one element) serves base addresses that are not 16-byte aligned and real data with odd n or odd stride:
//              every second b_j then starts 8 bytes off a 16-byte boundary (the reason krylov_combine_z_kernel keeps one too).
//   workgroup= NT = 256 threads, PJ_PER_THREAD = 4 items per thread; grid g = min(PJ_MAXBLK = 1024, ceil(items / 1024)), grid-stride.
//   pass 1   : grid (g, ceil(m / PJ_J)); a workgroup reads its items of src ONCE for PJ_J = 8 basis vectors and leaves one (re, im)
//              partial per vector: work[2 (j g + blockIdx.x)].
//   pass 2   : one workgroup per vector adds its g partials in fixed order (thread t: t, t + 256, ...; then the tree) -> coeff[2 j].
//   pass 3   : grid g; the m coefficients go to LDS once per workgroup; per item one read of src and of every b_j, a chain of fused
//              multiply-adds t -= c_j b_j in ascending j, one write of dst; |dst|^2 partials at work[2 PJ_MAXBLK PJ_MAX + 2 blockIdx.x].
//   pass 4   : reduce_pass2 over the g partials of pass 3 (only with nrm2_out).
// No floating-point atomics anywhere: the same call on the same data gives the same bits.
constexpr int PJ_J = 8;
constexpr int PJ_PER_THREAD = 4;
constexpr int PJ_MAXBLK = 1024;
constexpr int PJ_MAX = TPA_PROJECT_MAX;
static_assert(TPA_PROJECT_WORK >= 2 * PJ_MAXBLK * (PJ_MAX + 1), "TPA_PROJECT_WORK too small for the partials");

template <bool CPLX, bool VEC>
__device__ __forceinline__ double2 pj_load(const double *p) {
    if (VEC) return *reinterpret_cast<const double2 *>(p);
    double2 v;
    v.x = p[0];
    v.y = CPLX ? p[1] : 0.;
    return v;
}

template <bool CPLX, bool VEC>
__global__ __launch_bounds__(NT) void project_dots_kernel(int64_t n_items, int m, const double *__restrict__ B, int64_t stride_d,
                                                          const double *__restrict__ src, double *__restrict__ partial) {
    __shared__ double red[NT / 64];
    constexpr int W = (CPLX || VEC) ? 2 : 1;       // doubles per item
    const int j0 = blockIdx.y * PJ_J;
    const int nj = (m - j0 < PJ_J) ? m - j0 : PJ_J;
    const double *Bj = B + (int64_t)j0 * stride_d;
    double sr[PJ_J], si[PJ_J];
#pragma unroll
    for (int jj = 0; jj < PJ_J; ++jj) sr[jj] = si[jj] = 0.;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * NT) {
        const double2 x = pj_load<CPLX, VEC>(src + W * i);
#pragma unroll
        for (int jj = 0; jj < PJ_J; ++jj) {
            if (jj < nj) {
                const double2 b = pj_load<CPLX, VEC>(Bj + jj * stride_d + W * i);
                if (CPLX) {         // conj(b) x
                    sr[jj] = fma(b.x, x.x, sr[jj]);
                    sr[jj] = fma(b.y, x.y, sr[jj]);
                    si[jj] = fma(b.x, x.y, si[jj]);
                    si[jj] = fma(-b.y, x.x, si[jj]);
                } else {
                    sr[jj] = fma(b.x, x.x, sr[jj]);
                    if (VEC) sr[jj] = fma(b.y, x.y, sr[jj]);
                }
            }
        }
    }
#pragma unroll
    for (int jj = 0; jj < PJ_J; ++jj) {
        if (jj < nj) {          // (uniform over the workgroup: the barriers of block_sum are reached by all threads or by none)
            const double r = block_sum<NT>(sr[jj], red);
            const double im = CPLX ? block_sum<NT>(si[jj], red) : 0.;
            if (threadIdx.x == 0) {
                double *p = partial + 2 * ((int64_t)(j0 + jj) * gridDim.x + blockIdx.x);
                p[0] = r;
                p[1] = im;
            }
        }
    }
}

__global__ __launch_bounds__(NT) void project_coeff_kernel(int g, const double *__restrict__ partial, double *__restrict__ coeff) {
    __shared__ double red[NT / 64];
    const double *p = partial + 2 * (int64_t)blockIdx.x * g;
    double sr = 0, si = 0;
    for (int i = threadIdx.x; i < g; i += NT) {
        sr += p[2 * i];
        si += p[2 * i + 1];
    }
    sr = block_sum<NT>(sr, red);
    si = block_sum<NT>(si, red);
    if (threadIdx.x == 0) {
        coeff[2 * blockIdx.x] = sr;
        coeff[2 * blockIdx.x + 1] = si;
    }
}

// (src and dst may be the same vector: every item is read and written by the same thread; no __restrict__ on the two)
template <bool CPLX, bool VEC>
__global__ __launch_bounds__(NT) void project_update_kernel(int64_t n_items, int m, const double *__restrict__ B, int64_t stride_d,
                                                            const double *__restrict__ coeff, const double *src, double *dst,
                                                            double *__restrict__ partial) {
    __shared__ double red[NT / 64];
    __shared__ double2 cs[PJ_MAX];
    constexpr int W = (CPLX || VEC) ? 2 : 1;
    for (int j = threadIdx.x; j < m; j += NT) cs[j] = double2{coeff[2 * j], coeff[2 * j + 1]};
    __syncthreads();
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * NT) {
        double2 t = pj_load<CPLX, VEC>(src + W * i);
        const double *p = B + W * i;
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const double2 c = cs[j];
            const double2 b = pj_load<CPLX, VEC>(p + j * stride_d);
            if (CPLX) {
                t.x = fma(-c.x, b.x, t.x);
                t.x = fma(c.y, b.y, t.x);
                t.y = fma(-c.x, b.y, t.y);
                t.y = fma(-c.y, b.x, t.y);
            } else {
                t.x = fma(-c.x, b.x, t.x);
                if (VEC) t.y = fma(-c.x, b.y, t.y);
            }
        }
        if (VEC) {
            *reinterpret_cast<double2 *>(dst + W * i) = t;
        } else {
            dst[W * i] = t.x;
            if (CPLX) dst[W * i + 1] = t.y;
        }
        s = fma(t.x, t.x, s);
        if (CPLX || VEC) s = fma(t.y, t.y, s);
    }
    if (partial != nullptr) {
        s = block_sum<NT>(s, red);
        if (threadIdx.x == 0) {
            partial[2 * blockIdx.x] = s;
            partial[2 * blockIdx.x + 1] = 0.;
        }
    }
}

}  // namespace

extern "C" int tpa_project_out(int dtype, int64_t n, const void *basis_dev, int m, int64_t stride, const void *src_dev, void *dst_dev,
                               double *coeff_dev, double *nrm2_out_dev, double *work_dev, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(m >= 0 && m <= PJ_MAX);
    TPA_ARG_CHECK(m == 0 || (coeff_dev != nullptr && (n <= 0 || (basis_dev != nullptr && stride >= n))));
    TPA_ARG_CHECK(n <= 0 || (src_dev != nullptr && dst_dev != nullptr && work_dev != nullptr));
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) {
        if (m > 0) TPA_HIP_CHECK(hipMemsetAsync(coeff_dev, 0, sizeof(double) * 2 * m, st));
        if (nrm2_out_dev) TPA_HIP_CHECK(hipMemsetAsync(nrm2_out_dev, 0, sizeof(double) * 2, st));
        return 0;
    }
    const bool cplx = (dtype == TPA_C128);
    const int64_t isz = cplx ? 16 : 8;
    if (m > 0) {        // dst must not overlap the basis
        const uintptr_t b0 = (uintptr_t)basis_dev, b1 = b0 + (uintptr_t)(((int64_t)(m - 1) * stride + n) * isz);
        const uintptr_t d0 = (uintptr_t)dst_dev, d1 = d0 + (uintptr_t)(n * isz);
        TPA_ARG_CHECK((d1 <= b0 || b1 <= d0) && "tpa_project_out: dst overlaps the basis");
    }
    const bool aligned = (((uintptr_t)src_dev | (uintptr_t)dst_dev | (m > 0 ? (uintptr_t)basis_dev : 0)) & 15) == 0;
    const bool vec = aligned && (cplx || (n % 2 == 0 && (m <= 1 || stride % 2 == 0)));
    const int64_t n_items = (!cplx && vec) ? n / 2 : n;
    const int64_t stride_d = cplx ? 2 * stride : stride;        // doubles from b_j to b_{j+1}
    int64_t g64 = (n_items + (int64_t)NT * PJ_PER_THREAD - 1) / ((int64_t)NT * PJ_PER_THREAD);
    const int g = (int)(g64 > PJ_MAXBLK ? PJ_MAXBLK : g64);
    const double *B = (const double *)basis_dev, *src = (const double *)src_dev;
    double *dst = (double *)dst_dev;
    double *npart = nrm2_out_dev ? work_dev + 2 * (int64_t)PJ_MAXBLK * PJ_MAX : nullptr;
    if (m == 0 && src == dst && !nrm2_out_dev) return 0;
    if (m > 0) {
        const dim3 grid1(g, (m + PJ_J - 1) / PJ_J);
        if (cplx && vec)
            project_dots_kernel<true, true><<<grid1, NT, 0, st>>>(n_items, m, B, stride_d, src, work_dev);
        else if (cplx)
            project_dots_kernel<true, false><<<grid1, NT, 0, st>>>(n_items, m, B, stride_d, src, work_dev);
        else if (vec)
            project_dots_kernel<false, true><<<grid1, NT, 0, st>>>(n_items, m, B, stride_d, src, work_dev);
        else
            project_dots_kernel<false, false><<<grid1, NT, 0, st>>>(n_items, m, B, stride_d, src, work_dev);
        TPA_LAUNCH_CHECK();
        project_coeff_kernel<<<m, NT, 0, st>>>(g, work_dev, coeff_dev);
        TPA_LAUNCH_CHECK();
    }
    if (cplx && vec)
        project_update_kernel<true, true><<<g, NT, 0, st>>>(n_items, m, B, stride_d, coeff_dev, src, dst, npart);
    else if (cplx)
        project_update_kernel<true, false><<<g, NT, 0, st>>>(n_items, m, B, stride_d, coeff_dev, src, dst, npart);
    else if (vec)
        project_update_kernel<false, true><<<g, NT, 0, st>>>(n_items, m, B, stride_d, coeff_dev, src, dst, npart);
    else
        project_update_kernel<false, false><<<g, NT, 0, st>>>(n_items, m, B, stride_d, coeff_dev, src, dst, npart);
    TPA_LAUNCH_CHECK();
    if (nrm2_out_dev) {
        reduce_pass2<<<1, NT, 0, st>>>(g, npart, nrm2_out_dev);
        TPA_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int tpa_axpy(int dtype, int64_t n, double ar, double ai, const void *x, void *y,
                        void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int g = grid_for(n, 4) * 2;
    if (dtype == TPA_F64)
        axpy_f64<<<g, NT, 0, st>>>(n, ar, (const double *)x, (double *)y);
    else
        axpy_c128<<<g, NT, 0, st>>>(n, ar, ai, (const double2 *)x, (double2 *)y);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_scal(int dtype, int64_t n, double ar, double ai, void *x, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int g = grid_for(n, 4) * 2;
    if (dtype == TPA_F64)
        scal_f64<<<g, NT, 0, st>>>(n, ar, (double *)x);
    else
        scal_c128<<<g, NT, 0, st>>>(n, ar, ai, (double2 *)x);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_dot(int dtype, int64_t n, const void *x, const void *y, int do_conj,
                       double *out, double *scratch, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    hipStream_t st = (hipStream_t)stream;
    const int g = (n > 0) ? grid_for(n, 8) : 1;
    if (dtype == TPA_F64)
        reduce_pass1<0><<<g, NT, 0, st>>>(n, (const double *)x, (const double *)y, scratch);
    else if (do_conj)
        reduce_pass1<1><<<g, NT, 0, st>>>(n, (const double *)x, (const double *)y, scratch);
    else
        reduce_pass1<2><<<g, NT, 0, st>>>(n, (const double *)x, (const double *)y, scratch);
    TPA_LAUNCH_CHECK();
    reduce_pass2<<<1, NT, 0, st>>>(g, scratch, out);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_nrm2sq(int dtype, int64_t n, const void *x, double *out, double *scratch,
                          void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nd = (dtype == TPA_C128) ? 2 * n : n;  // |z|^2 = re^2 + im^2: flat real pass
    const int g = (nd > 0) ? grid_for(nd, 8) : 1;
    reduce_pass1<3><<<g, NT, 0, st>>>(nd, (const double *)x, (const double *)x, scratch);
    TPA_LAUNCH_CHECK();
    reduce_pass2<<<1, NT, 0, st>>>(g, scratch, out);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_lanczos_update(int dtype, int64_t n, void *w, double ar, double ai,
                                  const void *v1, double br, double bi, const void *v0, double *out,
                                  double *scratch, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(v1 != nullptr);
    hipStream_t st = (hipStream_t)stream;
    const int g = (n > 0) ? grid_for(n, 8) : 1;
    if (dtype == TPA_F64) {
        if (v0)
            lanczos_update_kernel<false, true><<<g, NT, 0, st>>>(n, (double *)w, ar, ai, (const double *)v1, br, bi, (const double *)v0, scratch);
        else
            lanczos_update_kernel<false, false><<<g, NT, 0, st>>>(n, (double *)w, ar, ai, (const double *)v1, br, bi, nullptr, scratch);
    } else {
        if (v0)
            lanczos_update_kernel<true, true><<<g, NT, 0, st>>>(n, (double *)w, ar, ai, (const double *)v1, br, bi, (const double *)v0, scratch);
        else
            lanczos_update_kernel<true, false><<<g, NT, 0, st>>>(n, (double *)w, ar, ai, (const double *)v1, br, bi, nullptr, scratch);
    }
    TPA_LAUNCH_CHECK();
    reduce_pass2<<<1, NT, 0, st>>>(g, scratch, out);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_fill_zero(void *dst, int64_t n_bytes, void *stream) {
    if (n_bytes <= 0) return 0;
    TPA_HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)n_bytes, (hipStream_t)stream));
    return 0;
}

// One Lanczos step of krylov_based.py:655-672 with the scalars kept on the device, so that the host can enqueue the next
// matvec without waiting:   alpha = Re <w|v1> ;  w -= alpha v1 ;  w -= beta_prev v0 ;  bsq = |w|^2 ;  w /= sqrt(bsq).
// ab_out[0] = alpha, ab_out[1] = bsq (= beta^2 of this step; the NEXT step passes &ab_out[1] as bsq_prev).
extern "C" int tpa_lanczos_step(int dtype, int64_t n, void *w, const void *v1, const void *v0,
                                const double *bsq_prev, double *ab_out, double *scratch, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(v1 != nullptr && ab_out != nullptr && (v0 == nullptr || bsq_prev != nullptr));
    hipStream_t st = (hipStream_t)stream;
    const bool cplx = (dtype == TPA_C128);
    const int g = (n > 0) ? grid_for(n, 8) : 1;
    if (!cplx)
        reduce_pass1<0><<<g, NT, 0, st>>>(n, (const double *)w, (const double *)v1, scratch);
    else
        reduce_pass1<1><<<g, NT, 0, st>>>(n, (const double *)w, (const double *)v1, scratch);
    reduce_pass2<<<1, NT, 0, st>>>(g, scratch, ab_out);          // ab_out[0] = Re <w|v1>, ab_out[1] = Im (overwritten below)
    double *part2 = scratch + 2 * MAXBLK;
    if (!cplx) {
        if (v0)
            lanczos_update_dev_kernel<false, true><<<g, NT, 0, st>>>(n, (double *)w, ab_out, (const double *)v1, bsq_prev, (const double *)v0, part2);
        else
            lanczos_update_dev_kernel<false, false><<<g, NT, 0, st>>>(n, (double *)w, ab_out, (const double *)v1, nullptr, nullptr, part2);
    } else {
        if (v0)
            lanczos_update_dev_kernel<true, true><<<g, NT, 0, st>>>(n, (double *)w, ab_out, (const double *)v1, bsq_prev, (const double *)v0, part2);
        else
            lanczos_update_dev_kernel<true, false><<<g, NT, 0, st>>>(n, (double *)w, ab_out, (const double *)v1, nullptr, nullptr, part2);
    }
    reduce_pass2_to<<<1, NT, 0, st>>>(g, part2, ab_out + 1);
    const int64_t nd = cplx ? 2 * n : n;
    scal_rsqrt_dev_kernel<<<grid_for(nd, 8), NT, 0, st>>>(nd, (double *)w, ab_out + 1);
    TPA_LAUNCH_CHECK();
    return 0;
}

// ================================================================================================================
// LanczosGroundState.run as ONE host call (reference krylov_based.py:645-700 `_build_krylov`, :223-240 `_calc_result_full`).
//
// Why: at chi <= 512 a bond update is bounded by host time, not by the kernels -- every Krylov step costs ~0.5 ms of
// interpreter work (Array objects, argument checks, ctypes marshalling for the 2-3 launches of a matvec and the 5 of
// the recurrence) against ~0.1 ms of kernels.  Here the host side of a step is a C++ loop: replay the matvec "program"
// (the cached plans of TwoSiteH: grouped GEMM / block linear combination / grouped GEMM) on raw arenas, run the fused
// recurrence with alpha, beta kept on the device, and hand (alpha, beta^2) of the PREVIOUS step to a callback that does
// the reference's tridiagonal eigen-solve and stopping test (numpy.linalg.eigh, so that iteration counts and signs are
// those of the reference) while the device is already busy with the next matvec.
// ================================================================================================================
namespace {

constexpr int LZ_MAX_COMBINE = 64;
struct LzCoeff {
    double c[LZ_MAX_COMBINE];
};

// out = sum_k c_k V_k (V_k = krylov + k n), partial |out|^2 per workgroup: one pass over N + 1 vectors instead of N axpys
template <bool CPLX>
__global__ __launch_bounds__(NT) void krylov_combine_kernel(int64_t nd, int N, LzCoeff C, const double *__restrict__ V, int64_t stride,
                                                            double *__restrict__ out, double *__restrict__ partial) {
    __shared__ double red[NT / 64];
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nd; i += (int64_t)gridDim.x * NT) {
        double t = 0;
        for (int k = 0; k < N; ++k) t = fma(C.c[k], V[k * stride + i], t);
        out[i] = t;
        s = fma(t, t, s);
    }
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s;
        partial[2 * blockIdx.x + 1] = 0.;
    }
}

// ---- the same combination with COMPLEX coefficients: exp(delta h) e_0 of LanczosEvolution --------------------------------------
// Replaces, for `LanczosEvolution.run` (reference krylov_based.py:757-795), the N flat axpy passes (or, real Krylov vectors
// with an imaginary delta, the N generic iadd_prefactor_other calls) of `_calc_result_full` (reference :160-198):
//     out = scale * sum_{k<N} c_k V_k ,  partial |sum_k c_k V_k|^2 per workgroup (BEFORE the scale).
// One pass over the N + 1 vectors, HBM bound (itemsize n (N + 1) bytes).  The basis is real or complex (template, no branch per
// element), `out` is always complex.  VEC: 16-byte loads -- one complex or two real elements of every V_k per thread and step,
// 16-byte stores; the coefficients are kernel arguments (k is uniform: scalar loads from the argument segment).  The scalar
// form (8-byte loads) serves a real basis with odd n -- every second V_k then starts 8 bytes off a 16-byte boundary, there is no
// aligned body to peel a tail from -- and base addresses that are not 16-byte aligned.
// `scale` is applied here because its value (|psi0| |exp(delta h) e_0|, or 1) is known before the pass and costs no traffic; the
// division by the returned norm is the caller's (`tpa_scal`): it has to look at that norm on the host anyway (ill-conditioned
// warning, degenerate fallback to the start vector), so a second device pass fed from device memory would save no wait.
struct LzCoeffZ {
    double2 c[LZ_MAX_COMBINE];
};

template <bool CPLX, bool VEC>
__global__ __launch_bounds__(NT) void krylov_combine_z_kernel(int64_t n_items, int N, LzCoeffZ C, double scale, const double *__restrict__ V,
                                                              int64_t stride, double *__restrict__ out, double *__restrict__ partial) {
    __shared__ double red[NT / 64];
    constexpr int W = (CPLX || VEC) ? 2 : 1;       // doubles of one V_k per item
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * NT) {
        const double *p = V + W * i;
        double re0 = 0, im0 = 0, re1 = 0, im1 = 0;
#pragma unroll 4
        for (int k = 0; k < N; ++k) {
            const double2 c = C.c[k];
            double2 v;
            if (VEC) {
                v = *reinterpret_cast<const double2 *>(p + k * stride);
            } else {
                v.x = p[k * stride];
                v.y = CPLX ? p[k * stride + 1] : 0.;
            }
            if (CPLX) {
                re0 = fma(c.x, v.x, re0);
                re0 = fma(-c.y, v.y, re0);
                im0 = fma(c.x, v.y, im0);
                im0 = fma(c.y, v.x, im0);
            } else {
                re0 = fma(c.x, v.x, re0);
                im0 = fma(c.y, v.x, im0);
                if (VEC) {
                    re1 = fma(c.x, v.y, re1);
                    im1 = fma(c.y, v.y, im1);
                }
            }
        }
        s = fma(re0, re0, s);
        s = fma(im0, im0, s);
        if (!CPLX && VEC) {
            s = fma(re1, re1, s);
            s = fma(im1, im1, s);
            reinterpret_cast<double2 *>(out)[2 * i] = double2{scale * re0, scale * im0};
            reinterpret_cast<double2 *>(out)[2 * i + 1] = double2{scale * re1, scale * im1};
        } else if (VEC) {
            reinterpret_cast<double2 *>(out)[i] = double2{scale * re0, scale * im0};
        } else {
            out[2 * i] = scale * re0;
            out[2 * i + 1] = scale * im0;
        }
    }
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s;
        partial[2 * blockIdx.x + 1] = 0.;
    }
}

__global__ void lz_post_scalars_kernel(const double *__restrict__ src, double *__restrict__ dst_host) {
    dst_host[0] = src[0];
    dst_host[1] = src[1];
    __threadfence_system();
}

__global__ __launch_bounds__(NT) void lz_copy_scaled_kernel(int64_t nd, const double *__restrict__ x, const double *__restrict__ nrm2,
                                                            double *__restrict__ y) {
    const double f = 1. / sqrt(nrm2[0]);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nd; i += (int64_t)gridDim.x * NT) y[i] = f * x[i];
}

struct LzHost {          // per-thread persistent host resources
    double *pinned = nullptr;        // mapped host memory: 2 doubles per step
    int capacity = 0;
    std::vector<hipEvent_t> ev;      // one per step (no timing)
    std::vector<hipEvent_t> tev;     // timing events for the GEMM launches (only when asked for)
};
thread_local LzHost lz_host;

int lz_reserve(int steps) {
    LzHost &H = lz_host;
    if (H.capacity < steps + 2) {
        if (H.pinned) TPA_HIP_CHECK(hipHostFree(H.pinned));
        H.capacity = 2 * (steps + 2);
        TPA_HIP_CHECK(hipHostMalloc((void **)&H.pinned, sizeof(double) * 2 * H.capacity, hipHostMallocDefault));
    }
    while ((int)H.ev.size() < steps + 2) {
        hipEvent_t e;
        TPA_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        H.ev.push_back(e);
    }
    return 0;
}

inline void *lz_slot(int64_t s, void *const *bufs, int n_bufs, const void *in, void *out) {
    if (s == -1) return const_cast<void *>(in);
    if (s == -2) return out;
    return (s >= 0 && s < n_bufs) ? bufs[s] : nullptr;
}

}  // namespace

// collective hook of the launch programs (op kind 3): set by the caller around a run, per host thread
static thread_local tpa_collective_callback lz_collective = nullptr;
static thread_local void *lz_collective_user = nullptr;
extern "C" int tpa_lanczos_set_collective(tpa_collective_callback cb, void *user) {
    lz_collective = cb;
    lz_collective_user = user;
    return 0;
}

// Step k >= 1 of the loop with full re-orthogonalisation (flag bit 0; reference krylov_based.py:660-672 with `reortho`):
//   alpha = Re <w|v_k> ;  w -= alpha v_k ;  w -= sum_{j<k} <v_j|w> v_j (tpa_project_out on the Krylov buffer itself, stride n; the
//   beta v_{k-1} term of the three-term recurrence is part of that sum) ;  bsq = |w|^2 from the same pass ;  w /= sqrt(bsq).
// pw: 2 TPA_PROJECT_MAX + 2 + TPA_PROJECT_WORK doubles (coefficients | unused | partials).  ab_out[2] (the alpha slot of the NEXT
// step, rewritten by it) receives the zero that tpa_project_out posts behind the norm.
static int lz_step_reortho(int dtype, int64_t n, double *w, const double *V, int k, double *ab_out, double *scratch, double *pw, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const bool cplx = (dtype == TPA_C128);
    const int64_t nd = cplx ? 2 * n : n;
    const double *vk = V + (int64_t)k * nd;
    const int g = grid_for(n, 8);
    double *part2 = scratch + 2 * MAXBLK;
    if (!cplx) {
        reduce_pass1<0><<<g, NT, 0, st>>>(n, w, vk, scratch);
        reduce_pass2<<<1, NT, 0, st>>>(g, scratch, ab_out);
        lanczos_update_dev_kernel<false, false><<<g, NT, 0, st>>>(n, w, ab_out, vk, nullptr, nullptr, part2);
    } else {
        reduce_pass1<1><<<g, NT, 0, st>>>(n, w, vk, scratch);
        reduce_pass2<<<1, NT, 0, st>>>(g, scratch, ab_out);
        lanczos_update_dev_kernel<true, false><<<g, NT, 0, st>>>(n, w, ab_out, vk, nullptr, nullptr, part2);
    }
    TPA_LAUNCH_CHECK();
    if (int rc = tpa_project_out(dtype, n, V, k, n, w, w, pw, ab_out + 1, pw + 2 * PJ_MAX + 2, stream)) return rc;
    scal_rsqrt_dev_kernel<<<grid_for(nd, 8), NT, 0, st>>>(nd, w, ab_out + 1);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_lanczos_run(int dtype, int64_t n, const int64_t *ops, int n_ops, void *const *bufs, int n_bufs,
                               void *krylov_dev, const void *psi0_dev, int N_max, double cutoff, int has_shift, double E_shift,
                               double *scalars_dev, double *scratch_dev, tpa_lanczos_callback cb, void *user,
                               int time_gemms, double *info, void *stream) {
    return tpa_lanczos_run_ex(dtype, n, ops, n_ops, bufs, n_bufs, krylov_dev, psi0_dev, N_max, cutoff, has_shift, E_shift, scalars_dev,
                              scratch_dev, cb, user, time_gemms, info, 0, nullptr, stream);
}

extern "C" int tpa_lanczos_run_ex(int dtype, int64_t n, const int64_t *ops, int n_ops, void *const *bufs, int n_bufs,
                                  void *krylov_dev, const void *psi0_dev, int N_max, double cutoff, int has_shift, double E_shift,
                                  double *scalars_dev, double *scratch_dev, tpa_lanczos_callback cb, void *user,
                                  int time_gemms, double *info, int flags, double *project_work_dev, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK((flags & ~1) == 0 && (!(flags & 1) || (project_work_dev != nullptr && N_max <= PJ_MAX)));
    const bool reortho = (flags & 1) != 0;
    TPA_ARG_CHECK(n > 0 && N_max >= 1 && n_ops >= 1 && ops != nullptr && krylov_dev != nullptr && psi0_dev != nullptr);
    TPA_ARG_CHECK(scalars_dev != nullptr && scratch_dev != nullptr && cb != nullptr && info != nullptr);
    hipStream_t st = (hipStream_t)stream;
    const bool cplx = (dtype == TPA_C128);
    const int64_t nd = cplx ? 2 * n : n;
    double *V = (double *)krylov_dev;
    if (int rc = lz_reserve(N_max)) return rc;
    LzHost &H = lz_host;
    // beta_0 = |psi0| ; V_0 = psi0 / beta_0     (reference :650-653)
    double *sc0 = scalars_dev + 2 * (N_max + 1);        // |psi0|^2 lives behind the per-step scalars
    if (int rc = tpa_nrm2sq(dtype, n, psi0_dev, sc0, scratch_dev, stream)) return rc;
    lz_copy_scaled_kernel<<<grid_for(nd, 8), NT, 0, st>>>(nd, (const double *)psi0_dev, sc0, V);
    lz_post_scalars_kernel<<<1, 1, 0, st>>>(sc0, H.pinned + 2 * (N_max + 1));
    TPA_HIP_CHECK(hipEventRecord(H.ev[N_max + 1], st));
    size_t n_tev = 0;
    int n_matvec = 0, N = 0;
    bool stopped = false;
    for (int k = 0; k < N_max; ++k) {
        const double *vin = V + (int64_t)k * nd;
        double *w = V + (int64_t)(k + 1) * nd;
        for (int o = 0; o < n_ops; ++o) {
            const int64_t *op = ops + 12 * o;
            void *a = lz_slot(op[6], bufs, n_bufs, vin, w), *b = lz_slot(op[7], bufs, n_bufs, vin, w), *c = lz_slot(op[8], bufs, n_bufs, vin, w);
            if (op[0] == 0 || op[0] == 7) {     // 7: kind 0 through tpa_gemm_chain_ex (op[9] = slot of A2, op[10] = alphas)
                TPA_ARG_CHECK(a != nullptr && b != nullptr && c != nullptr);
                const void *a2 = op[0] == 7 ? lz_slot(op[9], bufs, n_bufs, vin, w) : nullptr;
                TPA_ARG_CHECK(op[0] == 0 || (a2 != nullptr && op[10] != 0));
                if (time_gemms) {
                    while (H.tev.size() < n_tev + 2) {
                        hipEvent_t e;
                        TPA_HIP_CHECK(hipEventCreate(&e));
                        H.tev.push_back(e);
                    }
                    TPA_HIP_CHECK(hipEventRecord(H.tev[n_tev], st));
                }
                if (int rc = op[0] == 0 ? tpa_gemm_chain(dtype, (int)op[1], (const int64_t *)op[2], (const int64_t *)op[3],
                                                         (const int32_t *)op[4], (int)op[5], a, b, c, stream)
                                        : tpa_gemm_chain_ex(dtype, (int)op[1], (const int64_t *)op[2], (const int64_t *)op[3],
                                                            (const int32_t *)op[4], (int)op[5], a, a2, b, c, (const double *)op[10], stream))
                    return rc;
                if (time_gemms) {
                    TPA_HIP_CHECK(hipEventRecord(H.tev[n_tev + 1], st));
                    n_tev += 2;
                }
            } else if (op[0] == 1) {
                TPA_ARG_CHECK(a != nullptr && c != nullptr);
                if (int rc = tpa_lincomb_batch(dtype, (const int64_t *)op[2], (int)op[5], (const int64_t *)op[3], op[9], a, c, stream)) return rc;
                // cfg = 1: the reduction of the split-K partial blocks of the GEMM just launched -- part of that GEMM's time
                if (time_gemms && op[1] == 1 && n_tev >= 2) TPA_HIP_CHECK(hipEventRecord(H.tev[n_tev - 1], st));
            } else if (op[0] == 2) {        // batched strided copy (pack / unpack of the row panels of a sharded matvec)
                TPA_ARG_CHECK(a != nullptr && c != nullptr);
                if (int rc = tpa_copy_batch(dtype, (const int64_t *)op[2], (int)op[5], op[9], a, c, stream)) return rc;
            } else if (op[0] == 3) {        // collective of the caller (all-gather of the row panels): enqueued by the host callback
                TPA_ARG_CHECK(lz_collective != nullptr);
                if (int rc = lz_collective((int)op[1], lz_collective_user)) {
                    snprintf(tpa_errbuf, sizeof(tpa_errbuf), "tpa_lanczos_run: the collective callback of op %d failed (%d)", o, rc);
                    return TPA_E_BADARG;
                }
            } else if (op[0] == 4) {        // dst = src - sum_j <b_j|src> b_j over `count` packed vectors (the projector of an excited-state search)
                TPA_ARG_CHECK(a != nullptr && b != nullptr && c != nullptr && op[2] != 0 && op[5] >= 0 && op[5] <= PJ_MAX);
                double *pw = (double *)op[2];
                if (int rc = tpa_project_out(dtype, n, a, (int)op[5], op[3], b, c, pw, nullptr, pw + 2 * op[5] + 2, stream)) return rc;
            } else if (op[0] == 5) {        // MPO step with small dense matrices on the physical index (op[7] holds max_d, not a slot)
                TPA_ARG_CHECK(a != nullptr && c != nullptr);
                if (int rc = tpa_mpo_apply_batch(dtype, (const int64_t *)op[2], (int)op[5], (const int64_t *)op[3], (const void *)op[4],
                                                 (int)op[7], op[9], a, c, stream))
                    return rc;
            } else if (op[0] == 6) {        // MPO step entry by entry (wide MPO bond blocks or wide sectors): p1 = rows, p2 = terms
                TPA_ARG_CHECK(a != nullptr && c != nullptr);
                if (int rc = tpa_mpo_entry_apply_batch(dtype, (const int64_t *)op[2], (int)op[5], (const int64_t *)op[3], (const int64_t *)op[4],
                                                       op[9], a, c, stream))
                    return rc;
            } else {
                TPA_ARG_CHECK(false && "unknown op kind");
            }
        }
        ++n_matvec;
        if (has_shift)
            if (int rc = tpa_axpy(dtype, n, E_shift, 0., vin, w, stream)) return rc;
        if (reortho && k > 0) {
            if (int rc = lz_step_reortho(dtype, n, w, V, k, scalars_dev + 2 * k, scratch_dev, project_work_dev, stream)) return rc;
        } else if (int rc = tpa_lanczos_step(dtype, n, w, vin, k > 0 ? (const void *)(V + (int64_t)(k - 1) * nd) : nullptr,
                                             k > 0 ? scalars_dev + 2 * (k - 1) + 1 : nullptr, scalars_dev + 2 * k, scratch_dev, stream))
            return rc;
        lz_post_scalars_kernel<<<1, 1, 0, st>>>(scalars_dev + 2 * k, H.pinned + 2 * k);
        TPA_HIP_CHECK(hipEventRecord(H.ev[k], st));
        if (k == 0) {       // |psi0| (reference :650: "norm of psi0 too small" is the caller's error; step 0 is in flight meanwhile)
            TPA_HIP_CHECK(hipEventSynchronize(H.ev[N_max + 1]));
            info[3] = sqrt(H.pinned[2 * (N_max + 1)]);
            if (!(info[3] >= cutoff)) {
                info[0] = 0.;
                info[1] = 1.;
                info[2] = 0.;
                TPA_HIP_CHECK(hipStreamSynchronize(st));
                return 0;
            }
        }
        if (k > 0) {
            TPA_HIP_CHECK(hipEventSynchronize(H.ev[k - 1]));
            if (cb(k - 1, H.pinned[2 * (k - 1)], H.pinned[2 * (k - 1) + 1], user)) {
                N = k;      // step k in flight is not part of the result (same Krylov space as the step-by-step loop)
                stopped = true;
                break;
            }
        }
        N = k + 1;
    }
    if (!stopped) {
        TPA_HIP_CHECK(hipEventSynchronize(H.ev[N_max - 1]));
        cb(N_max - 1, H.pinned[2 * (N_max - 1)], H.pinned[2 * (N_max - 1) + 1], user);
    }
    double ms = 0.;
    if (time_gemms && n_tev) {
        TPA_HIP_CHECK(hipEventSynchronize(H.tev[n_tev - 1]));
        for (size_t i = 0; i < n_tev; i += 2) {
            float t = 0.f;
            TPA_HIP_CHECK(hipEventElapsedTime(&t, H.tev[i], H.tev[i + 1]));
            ms += t;
        }
    }
    info[0] = (double)N;
    info[1] = (double)n_matvec;
    info[2] = ms;
    return 0;
}

// psi = sum_k coeff_k V_k, then |psi| (returned in out_host[0], blocking) -- the first half of `_calc_result_full`
// (krylov_based.py:223-236); the caller decides about the ill-conditioned / degenerate cases and scales.
extern "C" int tpa_krylov_combine(int dtype, int64_t n, const void *krylov_dev, int N, const double *coeff, void *out_dev,
                                  double *red_out_dev, double *scratch_dev, double *norm_host, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(n > 0 && N >= 1 && N <= LZ_MAX_COMBINE && coeff != nullptr && out_dev != nullptr && norm_host != nullptr);
    hipStream_t st = (hipStream_t)stream;
    const bool cplx = (dtype == TPA_C128);
    const int64_t nd = cplx ? 2 * n : n;
    LzCoeff C;
    for (int k = 0; k < LZ_MAX_COMBINE; ++k) C.c[k] = k < N ? coeff[k] : 0.;
    const int g = grid_for(nd, 4);
    if (cplx)
        krylov_combine_kernel<true><<<g, NT, 0, st>>>(nd, N, C, (const double *)krylov_dev, nd, (double *)out_dev, scratch_dev);
    else
        krylov_combine_kernel<false><<<g, NT, 0, st>>>(nd, N, C, (const double *)krylov_dev, nd, (double *)out_dev, scratch_dev);
    reduce_pass2<<<1, NT, 0, st>>>(g, scratch_dev, red_out_dev);
    TPA_LAUNCH_CHECK();
    if (int rc = lz_reserve(1)) return rc;
    lz_post_scalars_kernel<<<1, 1, 0, st>>>(red_out_dev, lz_host.pinned);
    TPA_HIP_CHECK(hipEventRecord(lz_host.ev[0], st));
    TPA_HIP_CHECK(hipEventSynchronize(lz_host.ev[0]));
    norm_host[0] = sqrt(lz_host.pinned[0]);
    return 0;
}

// out = scale * sum_{k < N} c_k v_k with complex c_k (host: N pairs re, im), basis F64 or C128, out C128; norm_host[0] = |sum_k c_k v_k|
// (before `scale`, blocking).  See krylov_combine_z_kernel for what it replaces and why the normalisation stays with the caller.
extern "C" int tpa_krylov_combine_z(int basis_dtype, int64_t n, const void *krylov_dev, int N, const double *coeff, double scale,
                                    void *out_dev, double *red_out_dev, double *scratch_dev, double *norm_host, void *stream) {
    TPA_ARG_CHECK(basis_dtype == TPA_F64 || basis_dtype == TPA_C128);
    TPA_ARG_CHECK(n > 0 && N >= 1 && N <= LZ_MAX_COMBINE && krylov_dev != nullptr && coeff != nullptr && out_dev != nullptr);
    TPA_ARG_CHECK(red_out_dev != nullptr && scratch_dev != nullptr && norm_host != nullptr);
    hipStream_t st = (hipStream_t)stream;
    const bool cplx = (basis_dtype == TPA_C128);
    LzCoeffZ C;
    for (int k = 0; k < LZ_MAX_COMBINE; ++k) C.c[k] = k < N ? double2{coeff[2 * k], coeff[2 * k + 1]} : double2{0., 0.};
    const bool aligned = (((uintptr_t)krylov_dev | (uintptr_t)out_dev) & 15) == 0;
    const bool vec = aligned && (cplx || n % 2 == 0);
    const int64_t n_items = (!cplx && vec) ? n / 2 : n;
    const int64_t stride = cplx ? 2 * n : n;            // doubles from V_k to V_{k+1}
    int64_t g64 = (n_items + NT - 1) / NT;
    const int g = (int)(g64 > 2 * MAXBLK ? 2 * MAXBLK : g64);       // 2 doubles per workgroup in scratch_dev (TPA_RED_SCRATCH = 4 MAXBLK)
    const double *V = (const double *)krylov_dev;
    double *out = (double *)out_dev;
    if (cplx && vec)
        krylov_combine_z_kernel<true, true><<<g, NT, 0, st>>>(n_items, N, C, scale, V, stride, out, scratch_dev);
    else if (cplx)
        krylov_combine_z_kernel<true, false><<<g, NT, 0, st>>>(n_items, N, C, scale, V, stride, out, scratch_dev);
    else if (vec)
        krylov_combine_z_kernel<false, true><<<g, NT, 0, st>>>(n_items, N, C, scale, V, stride, out, scratch_dev);
    else
        krylov_combine_z_kernel<false, false><<<g, NT, 0, st>>>(n_items, N, C, scale, V, stride, out, scratch_dev);
    TPA_LAUNCH_CHECK();
    reduce_pass2<<<1, NT, 0, st>>>(g, scratch_dev, red_out_dev);
    TPA_LAUNCH_CHECK();
    if (int rc = lz_reserve(1)) return rc;
    lz_post_scalars_kernel<<<1, 1, 0, st>>>(red_out_dev, lz_host.pinned);
    TPA_HIP_CHECK(hipEventRecord(lz_host.ev[0], st));
    TPA_HIP_CHECK(hipEventSynchronize(lz_host.ev[0]));
    norm_host[0] = sqrt(lz_host.pinned[0]);
    return 0;
}
