// Library/device info entry points.
#include "tpa_common.h"
#include <string.h>

extern "C" int tpa_device_info(char *name, int name_len, int *n_cu, int64_t *hbm_bytes) {
    int dev = 0;
    TPA_HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t p;
    TPA_HIP_CHECK(hipGetDeviceProperties(&p, dev));
    if (name && name_len > 0) {
        strncpy(name, p.gcnArchName, (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    return 0;
}

// ---- largest |B - 1| entry over a list of square blocks (the unit channels of the environments: TwoSiteH.matvec_program) ---------
// A maximum only, so the answer is exact and independent of the order: per thread, per wavefront (wave_max), then one atomic
// maximum per wavefront on the bit pattern of the non-negative double (which orders like the unsigned integer).  A NaN entry
// gives +inf (fmax would drop it).
namespace {
constexpr int UD_NT = 256;
struct UnitJob {  // int64[4]
    int64_t off, n, ld, pad;
};

template <bool CPLX>
__global__ __launch_bounds__(UD_NT) void unit_defect_kernel(const UnitJob *__restrict__ jobs, const double *__restrict__ src,
                                                            unsigned long long *__restrict__ out) {
    const UnitJob J = jobs[blockIdx.y];
    const int64_t total = J.n * J.n;
    double worst = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * UD_NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * UD_NT) {
        const int64_t r = e / J.n, c = e - r * J.n;
        const int64_t g = J.off + r * J.ld + c;
        const double one = (r == c) ? 1.0 : 0.0;
        double d;
        if (CPLX)
            d = hypot(src[2 * g] - one, src[2 * g + 1]);
        else
            d = fabs(src[g] - one);
        if (!(d == d)) d = __builtin_huge_val();
        worst = fmax(worst, d);
    }
    worst = wave_max(worst);
    if ((threadIdx.x & 63) == 0 && worst > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(worst));
}
}  // namespace

extern "C" int tpa_unit_defect_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const void *src_base, double *out_dev, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(n_jobs >= 0 && n_jobs <= 65535 && out_dev != nullptr);
    hipStream_t st = (hipStream_t)stream;
    TPA_HIP_CHECK(hipMemsetAsync(out_dev, 0, sizeof(double), st));
    if (n_jobs == 0) return 0;
    TPA_ARG_CHECK(jobs_dev != nullptr && src_base != nullptr);
    const dim3 grid(16, n_jobs);
    if (dtype == TPA_F64)
        unit_defect_kernel<false><<<grid, UD_NT, 0, st>>>((const UnitJob *)jobs_dev, (const double *)src_base, (unsigned long long *)out_dev);
    else
        unit_defect_kernel<true><<<grid, UD_NT, 0, st>>>((const UnitJob *)jobs_dev, (const double *)src_base, (unsigned long long *)out_dev);
    TPA_LAUNCH_CHECK();
    return 0;
}
