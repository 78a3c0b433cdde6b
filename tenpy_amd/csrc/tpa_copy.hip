// K8/K9/K10: data-movement kernels (HBM-bound), gfx950.
//
//  * tpa_copy_batch      : batched N-d strided sub-block copy.  One job = one (old block -> slice of
//                          new block) memcpy of the reference's combine/split workers
//                          (_npc_helper.pyx:1112-1123, :1235-1240 via _sliced_strided_copy :368) or one
//                          per-block transpose of itranspose (:853).  The host builds the copy plan
//                          from the integer bookkeeping; the device only moves bytes.
//  * tpa_lincomb_batch / tpa_mpo_apply_batch / tpa_mpo_entry_apply_batch: the MPO step of the factored effective Hamiltonians
//                          (block combinations, small matrices on the physical index, single entries); tpa_mpo_expand_batch: the
//                          entry-by-entry step with a destination offset per row -- the expanded matrix of the subspace expansion
//                          of single-site DMRG in one pass (reference mps_common.py:2140-2168, :2170-2199); tpa_mpo_cell_apply_batch:
//                          a cell of that matrix as one small dense product, every source row loaded once -- the zip-up application
//                          of an MPO that is dense in the bond index (reference mpo.py:1733-1757).
//  * tpa_scale_axis_batch: iscale_axis (np_conserved.py:2132-2140).
//  * tpa_gather_axis_batch: iproject's np.compress along one axis (np_conserved.py:1982).
#include "tpa_common.h"

namespace {
constexpr int NT = 256;
constexpr int MAXD = TPA_COPY_MAXDIM;

struct CopyJob {  // int64[4 + 3*MAXD]
    int64_t dst_off, src_off, ndim, flags;
    int64_t shape[MAXD], dstr[MAXD], sstr[MAXD];
};

template <bool CPLX>
__global__ __launch_bounds__(NT) void copy_batch_kernel(const CopyJob *__restrict__ jobs,
                                                        const double *__restrict__ src,
                                                        double *__restrict__ dst) {
    const CopyJob &J = jobs[blockIdx.y];
    const int nd = (int)J.ndim;
    int64_t total = 1;
    for (int d = 0; d < nd; ++d) total *= J.shape[d];
    const bool conj = CPLX && (J.flags & 1);
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        int64_t rem = e, so = J.src_off, dof = J.dst_off;
        for (int d = nd - 1; d >= 0; --d) {
            const int64_t s = J.shape[d];
            const int64_t q = rem / s;
            const int64_t i = rem - q * s;
            rem = q;
            so += i * J.sstr[d];
            dof += i * J.dstr[d];
        }
        if (CPLX) {
            double2 v = reinterpret_cast<const double2 *>(src)[so];
            if (conj) v.y = -v.y;
            reinterpret_cast<double2 *>(dst)[dof] = v;
        } else {
            dst[dof] = src[so];
        }
    }
}


// dst slab = sum_t alpha_t * src_t slab  (row-major slabs with their own row strides; coalesced along the columns)
struct LinJob {   // int64[8]
    int64_t dst_off, rows, cols, dst_ld, term_begin, term_count, pad0, pad1;
};
struct LinTerm {  // int64[4]
    int64_t src_off, src_ld;
    double a_re, a_im;
};

template <bool CPLX>
__global__ __launch_bounds__(NT) void lincomb_kernel(const LinJob *__restrict__ jobs, const LinTerm *__restrict__ terms,
                                                     const double *__restrict__ src, double *__restrict__ dst) {
    const LinJob J = jobs[blockIdx.y];
    const int64_t total = J.rows * J.cols;
    const LinTerm *T = terms + J.term_begin;
    const int nt = (int)J.term_count;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t r = e / J.cols, c = e - r * J.cols;
        if (!CPLX) {
            double v = 0.0;
            for (int t = 0; t < nt; ++t) v = fma(T[t].a_re, src[T[t].src_off + r * T[t].src_ld + c], v);
            dst[J.dst_off + r * J.dst_ld + c] = v;
        } else {
            double2 v{0.0, 0.0};
            for (int t = 0; t < nt; ++t) {
                const double2 x = reinterpret_cast<const double2 *>(src)[T[t].src_off + r * T[t].src_ld + c];
                v.x += T[t].a_re * x.x - T[t].a_im * x.y;
                v.y += T[t].a_re * x.y + T[t].a_im * x.x;
            }
            reinterpret_cast<double2 *>(dst)[J.dst_off + r * J.dst_ld + c] = v;
        }
    }
}

// ---- dst slab (pre, d_out, post) = sum_t M_t (d_out x d_in_t) applied on the middle index of src_t slab (pre, d_in_t, post) --------
// What it replaces: the W0 / W1 tensordots of TwoSiteH.matvec (reference mps_common.py:1321-1348) and the W0 tensordot of
// OneSiteH.matvec (:1146-1149) for MPO tensors whose bond legs have 1-wide blocks while a physical charge sector holds several
// states (spinful fermions with N only, spin-1 / bosons with parity, grouped sites): the MPO step of the factored matvec is then
// small dense matrices on the physical index instead of the single numbers of lincomb_kernel.  HBM-bound: every source element is
// read once per term, every destination element is written once.
// Launch geometry (tests/test_conformance_mpo_apply.py repeats it):
//   item     = 16 bytes in the VEC form (one complex element, or two real elements j, j + 1 of one row) -- 16-byte loads and stores;
//              the scalar form (8-byte accesses, item = one element) serves base addresses off a 16-byte boundary and, for real data,
//              jobs with an odd post, dst_off or src_off (decided per job, uniform over the workgroup).
//   thread   = one column (i, item of j): d_out accumulators in registers (D = 2, 4, 8 or 16 of them: the smallest that holds the
//              max_d of the call), one read of its d_in items per term, terms in table order, c ascending, one chain of fused
//              multiply-adds per component.  j is the fastest index: loads and stores of a wavefront are contiguous.
//   coeff    : the address does not depend on the lane -- uniform (scalar) loads, no LDS.
//   grid     = (min(512, ceil(max_job_elems / (max_d NT))), n_jobs), grid-stride over the columns of the job.
struct MpoJob {   // int64[8]
    int64_t dst_off, pre, d_out, post, term_begin, term_count, pad0, pad1;
};
struct MpoTerm {  // int64[4]
    int64_t src_off, d_in, coeff_off, pad;
};

template <bool CPLX, int D, bool VEC>
__device__ __forceinline__ void mpo_apply_job(const MpoJob &J, const MpoTerm *__restrict__ T, const double *__restrict__ coeff,
                                              const double *__restrict__ src, double *__restrict__ dst) {
    constexpr int W = (CPLX || VEC) ? 2 : 1;           // doubles per item
    constexpr int EPI = (!CPLX && VEC) ? 2 : 1;        // elements per item
    constexpr int CW = CPLX ? 2 : 1;                   // doubles per coefficient
    const int d_out = (int)J.d_out, nt = (int)J.term_count;
    const int64_t post_items = J.post / EPI;
    const int64_t n_cols = J.pre * post_items;
    const int64_t row_d = post_items * W;              // doubles from (i, o, j) to (i, o + 1, j)
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n_cols; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / post_items, jj = e - i * post_items;
        double2 acc[D];
#pragma unroll
        for (int o = 0; o < D; ++o) acc[o] = double2{0., 0.};
        for (int t = 0; t < nt; ++t) {
            const int d_in = (int)T[t].d_in;
            const double *x = src + CW * T[t].src_off + (i * d_in * post_items + jj) * W;
            const double *m = coeff + CW * T[t].coeff_off;
            for (int c = 0; c < d_in; ++c) {
                double2 v;
                if (VEC) {
                    v = *reinterpret_cast<const double2 *>(x + c * row_d);
                } else {
                    v.x = x[c * row_d];
                    v.y = CPLX ? x[c * row_d + 1] : 0.;
                }
#pragma unroll
                for (int o = 0; o < D; ++o) {
                    if (o < d_out) {
                        const double *a = m + CW * (o * d_in + c);
                        if (CPLX) {
                            acc[o].x = fma(a[0], v.x, acc[o].x);
                            acc[o].x = fma(-a[1], v.y, acc[o].x);
                            acc[o].y = fma(a[0], v.y, acc[o].y);
                            acc[o].y = fma(a[1], v.x, acc[o].y);
                        } else {
                            acc[o].x = fma(a[0], v.x, acc[o].x);
                            if (VEC) acc[o].y = fma(a[0], v.y, acc[o].y);
                        }
                    }
                }
            }
        }
        double *y = dst + CW * J.dst_off + (i * d_out * post_items + jj) * W;
#pragma unroll
        for (int o = 0; o < D; ++o) {
            if (o < d_out) {
                if (VEC) {
                    *reinterpret_cast<double2 *>(y + o * row_d) = acc[o];
                } else {
                    y[o * row_d] = acc[o].x;
                    if (CPLX) y[o * row_d + 1] = acc[o].y;
                }
            }
        }
    }
}

template <bool CPLX, int D, bool VEC>
__global__ __launch_bounds__(NT) void mpo_apply_kernel(const MpoJob *__restrict__ jobs, const MpoTerm *__restrict__ terms,
                                                       const double *__restrict__ coeff, const double *__restrict__ src,
                                                       double *__restrict__ dst) {
    const MpoJob J = jobs[blockIdx.y];
    const MpoTerm *T = terms + J.term_begin;
    if (J.pre <= 0 || J.d_out <= 0 || J.post <= 0) return;
    if (VEC && !CPLX) {         // two real elements per item: the whole job has to keep the items on 16-byte boundaries
        bool even = ((J.post | J.dst_off) & 1) == 0;
        for (int t = 0; t < (int)J.term_count; ++t) even = even && (T[t].src_off & 1) == 0;
        if (!even) {
            mpo_apply_job<CPLX, D, false>(J, T, coeff, src, dst);
            return;
        }
    }
    mpo_apply_job<CPLX, D, VEC>(J, T, coeff, src, dst);
}

// ---- dst slab (pre, n_rows, post) = rows of src slabs, entry by entry: dst row o = sum_t alpha_t * (one middle row of src_t) -----------
// What it replaces: the same W0 / W1 tensordots as mpo_apply_kernel for MPO tensors that kernel does not serve -- MPO bond legs with
// blocks wider than 1 (sorted and bunched bond legs), physical sectors wider than TPA_MPO_APPLY_MAXD, no conserved charge: the MPO
// index then sits INSIDE the memory of a block, and a single entry of W takes one middle row c of a source block (pre, M_in, post) to
// one middle row o of a destination block (pre, M_out, post).  HBM-bound: a source row is read once per term, every destination
// element is written once.  The same tables fed to lincomb_kernel would be one job per destination row, 8-byte accesses and a 64-bit
// division per element; here:
//   item     = 16 bytes in the VEC form (one complex element, or two real elements j, j + 1 of one row); the scalar form (8-byte
//              accesses, item = one element) serves base addresses off a 16-byte boundary and, for real data, jobs with an odd post,
//              dst_off, dst_ld, src_off or src_ld (decided per job from its tables, uniform over the workgroup).
//   thread   = one column (i, item of j) of its job: it walks the rows o of the job, one accumulator, terms in table order, one chain
//              of fused multiply-adds per component; one division per column.  j is the fastest index: the loads and stores of a
//              wavefront are contiguous.  The loads of up to four terms are issued before their multiply-adds.
//   tables   : the addresses of the row and term entries do not depend on the lane -- uniform (scalar) loads, no LDS.
//   grid     = (min(512, ceil(max_job_cols / (EPI NT))), n_jobs), EPI = 2 for real data with aligned bases, else 1; grid-stride over
//              the columns of the job.
struct EntJob {   // int64[8]
    int64_t dst_off, pre, n_rows, post, row_begin, dst_ld, pad0, pad1;
};
struct EntRow {   // int64[2]
    int64_t term_begin, term_count;
};
struct ExpRow {   // int64[4]: a row of tpa_mpo_expand_batch
    int64_t term_begin, term_count, dst_row_off, src_sel;
};

// Where a row of a job lands and which source it reads: what tells the two entry points apart.  Everything else -- the walk over the
// rows, the order of the terms, the multiply-adds -- is the one mpo_entry_job below.
struct SlabRows {     // tpa_mpo_entry_apply_batch: row o of a job is o * post elements into the slab; one source
    using Row = EntRow;
    static __device__ __forceinline__ int64_t dst_ld(const EntJob &J) { return J.dst_ld ? J.dst_ld : J.n_rows * J.post; }
    static __device__ __forceinline__ int64_t row_off(const Row &, int o, int64_t post) { return o * post; }
    static __device__ __forceinline__ const double *source(const Row &, const double *src, const double *) { return src; }
    static __device__ __forceinline__ bool row_even(const Row &) { return true; }
};
struct ScatteredRows {  // tpa_mpo_expand_batch: every row has a destination offset of its own and selects one of two sources
    using Row = ExpRow;
    static __device__ __forceinline__ int64_t dst_ld(const EntJob &J) { return J.dst_ld; }
    static __device__ __forceinline__ int64_t row_off(const Row &r, int, int64_t) { return r.dst_row_off; }
    static __device__ __forceinline__ const double *source(const Row &r, const double *src, const double *src2) {
        return r.src_sel ? src2 : src;
    }
    static __device__ __forceinline__ bool row_even(const Row &r) { return (r.dst_row_off & 1) == 0; }
};

template <bool CPLX, bool VEC>
__device__ __forceinline__ double2 ent_load(const double *x) {
    if (VEC) return *reinterpret_cast<const double2 *>(x);
    return double2{x[0], CPLX ? x[1] : 0.};
}

template <bool CPLX, bool VEC>
__device__ __forceinline__ void ent_fma(double2 &acc, const LinTerm &t, const double2 v) {
    if (CPLX) {
        acc.x = fma(t.a_re, v.x, acc.x);
        acc.x = fma(-t.a_im, v.y, acc.x);
        acc.y = fma(t.a_re, v.y, acc.y);
        acc.y = fma(t.a_im, v.x, acc.y);
    } else {
        acc.x = fma(t.a_re, v.x, acc.x);
        if (VEC) acc.y = fma(t.a_re, v.y, acc.y);
    }
}

template <bool CPLX, bool VEC, class P>
__device__ __forceinline__ void mpo_entry_job(const EntJob &J, const typename P::Row *__restrict__ R, const LinTerm *__restrict__ terms,
                                              const double *__restrict__ src, const double *__restrict__ src2,
                                              double *__restrict__ dst) {
    constexpr int EPI = (!CPLX && VEC) ? 2 : 1;        // elements per item
    constexpr int CW = CPLX ? 2 : 1;                   // doubles per element
    const int n_rows = (int)J.n_rows;
    const int64_t post_items = J.post / EPI;
    const int64_t n_cols = J.pre * post_items;
    const int64_t dst_ld = P::dst_ld(J);
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n_cols; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / post_items, j = (e - i * post_items) * EPI;
        double *y = dst + CW * (J.dst_off + i * dst_ld + j);
        typename P::Row r = R[0];
        for (int o = 0; o < n_rows; ++o) {
            const LinTerm *T = terms + r.term_begin;
            const int nt = (int)r.term_count;
            const double *x0 = P::source(r, src, src2) + CW * j;
            double *yo = y + CW * P::row_off(r, o, J.post);
            if (o + 1 < n_rows) r = R[o + 1];          // the next row's entry is on its way while this row's terms are read
            double2 acc{0., 0.};
            int t = 0;
            for (; t + 4 <= nt; t += 4) {
                const double2 v0 = ent_load<CPLX, VEC>(x0 + CW * (T[t].src_off + i * T[t].src_ld));
                const double2 v1 = ent_load<CPLX, VEC>(x0 + CW * (T[t + 1].src_off + i * T[t + 1].src_ld));
                const double2 v2 = ent_load<CPLX, VEC>(x0 + CW * (T[t + 2].src_off + i * T[t + 2].src_ld));
                const double2 v3 = ent_load<CPLX, VEC>(x0 + CW * (T[t + 3].src_off + i * T[t + 3].src_ld));
                ent_fma<CPLX, VEC>(acc, T[t], v0);
                ent_fma<CPLX, VEC>(acc, T[t + 1], v1);
                ent_fma<CPLX, VEC>(acc, T[t + 2], v2);
                ent_fma<CPLX, VEC>(acc, T[t + 3], v3);
            }
            for (; t < nt; ++t) ent_fma<CPLX, VEC>(acc, T[t], ent_load<CPLX, VEC>(x0 + CW * (T[t].src_off + i * T[t].src_ld)));
            if (VEC) {
                *reinterpret_cast<double2 *>(yo) = acc;
            } else {
                yo[0] = acc.x;
                if (CPLX) yo[1] = acc.y;
            }
        }
    }
}

// One job = blockIdx.y, for both row-addressing policies.
template <bool CPLX, bool VEC, class P>
__device__ __forceinline__ void mpo_entry_block(const EntJob *__restrict__ jobs, const typename P::Row *__restrict__ rows,
                                                const LinTerm *__restrict__ terms, const double *__restrict__ src,
                                                const double *__restrict__ src2, double *__restrict__ dst) {
    const EntJob J = jobs[blockIdx.y];
    if (J.pre <= 0 || J.n_rows <= 0 || J.post <= 0) return;
    if ((int64_t)blockIdx.x * NT >= J.pre * J.post) return;      // the grid is sized by the largest job: nothing left for this workgroup
    const typename P::Row *R = rows + J.row_begin;
    if (VEC && !CPLX) {         // two real elements per item: every address of the job has to stay on a 16-byte boundary
        bool even = ((J.post | J.dst_off | J.dst_ld) & 1) == 0;
        // every wavefront scans the tables of the job, lane l the rows l, l + 64, ...: the same answer in all of them
        for (int64_t o = threadIdx.x & 63; o < J.n_rows; o += 64) {
            even = even && P::row_even(R[o]);
            const LinTerm *T = terms + R[o].term_begin;
            for (int64_t t = 0; t < R[o].term_count; ++t) even = even && ((T[t].src_off | T[t].src_ld) & 1) == 0;
        }
        if (!__all(even)) {
            mpo_entry_job<CPLX, false, P>(J, R, terms, src, src2, dst);
            return;
        }
    }
    mpo_entry_job<CPLX, VEC, P>(J, R, terms, src, src2, dst);
}

template <bool CPLX, bool VEC>
__global__ __launch_bounds__(NT) void mpo_entry_apply_kernel(const EntJob *__restrict__ jobs, const EntRow *__restrict__ rows,
                                                             const LinTerm *__restrict__ terms, const double *__restrict__ src,
                                                             double *__restrict__ dst) {
    mpo_entry_block<CPLX, VEC, SlabRows>(jobs, rows, terms, src, src, dst);
}

// ---- the fused matrix of the subspace expansion: mpo_entry_apply_kernel with a destination offset per row ---------------------------
// What it replaces: LHeff / RHeff, iscale_axis, the tensordot over the fused leg and combine_legs of SubspaceExpansion (reference
// mps_common.py:2140-2168, :2170-2199).  T1 = LP . theta (or theta . RP) is the source; a job is one cell (row slice x column slice) of
// a charge block of the fused [(vL.p0), (wR.vR)] matrix, whose rows (p0', wR') lie one leading dimension apart for p0' and in other
// column slices for wR' -- so every row carries its own offset from (dst_off + i dst_ld).  Rows of the stacked form read theta itself
// (src2).  Launch geometry, summation and access widths are those of mpo_entry_apply_kernel above.
template <bool CPLX, bool VEC>
__global__ __launch_bounds__(NT) void mpo_expand_kernel(const EntJob *__restrict__ jobs, const ExpRow *__restrict__ rows,
                                                        const LinTerm *__restrict__ terms, const double *__restrict__ src,
                                                        const double *__restrict__ src2, double *__restrict__ dst) {
    mpo_entry_block<CPLX, VEC, ScatteredRows>(jobs, rows, terms, src, src2, dst);
}

// ---- a cell of the fused matrix as ONE small dense product: dst rows (n_rows) = coeff (n_rows x n_src) . distinct source rows (n_src) ---
// What it replaces: tensordot(B, W) and combine_legs of the zip-up MPO application (reference mpo.py:1733-1757) for MPO tensors that are
// DENSE in the bond index (the time-evolution MPOs U_I / U_II fill nearly every (wL, wR) block).  mpo_entry_job above computes every
// destination row from its own term list: the N rows of a cell that draw on the same K source rows load each of them N times (N K
// loads per column item).  Here a thread loads each source item ONCE and updates the accumulators of all rows of the job: K loads and
// N stores per column item.
//   item, thread, grid, access widths: those of mpo_expand_kernel (a thread owns one column item (i, j) of its job, lanes along j; 16
//              bytes per item where the bases and, for real data, every offset and stride of the job allow it, decided per job).
//   rows     : R = 8, 16 or 32 accumulators (selected by max_rows) in an array indexed by fully unrolled constants only -- registers,
//              never scratch.  Accumulators o >= n_rows are not stored (cell_update).
//   coeff    : the address of coeff(o, k) does not depend on the lane and is contiguous in o for a fixed k: UNIFORM (scalar) loads
//              through the constant cache, no LDS; the job's matrix is shared by all wavefronts of the launch through that cache.
//              The scalar register file does not hold the coefficients of four sources for 16 or 32 rows: the compiler spills scalar
//              registers through vector lanes (counts with the register figures in DESIGN.md; cell_update says what was done about it).
//   sources  : k ascending, the loads of four k issued before their multiply-adds; one chain of fused multiply-adds per component in
//              table order, zero coefficients included, the complex pattern of ent_fma: on finite data the result equals what
//              mpo_expand_kernel gives for the nonzero coefficients in the same order.
struct CellJob {  // int64[10]
    int64_t dst_off, pre, n_rows, post, dst_ld, row_begin, src_begin, n_src, coeff_off, pad;
};
struct CellRow {  // int64[2]
    int64_t dst_row_off, pad;
};
struct CellSrc {  // int64[2]
    int64_t src_off, src_ld;
};

constexpr int CELL_CHUNK = 8;

// acc[o] += coeff(o, k) * v for the rows of the job.  Accumulators o >= n_rows are not stored.
//   real   : CELL_CHUNK rows at a time behind a uniform branch -- a chunk inside the job reads its coefficients as one contiguous run
//            from one base address, the chunk that holds the last row clamps the index, the chunks beyond it are skipped.  Without the
//            branches the clamped addresses of all R rows stay live next to the coefficients of four sources and spill through vector
//            lanes (R = 32: 1759 spilled scalar registers against 194 this way); measured at chi = 1024, 12- and 24-row cells: 0.086
//            against 0.106 ms and 0.28 against 0.53 ms.
//   complex: all R rows with the index clamped (the rows beyond the job repeat the last one), no branch: it spills less to begin with
//            (at most 265), and the chunked form needs more vector registers and was slower on 1- to 12-row cells (0.047 against 0.038
//            ms, 0.175 against 0.167 ms) and 6 % faster on 24-row cells only.
template <bool CPLX, bool VEC, int R>
__device__ __forceinline__ void cell_update(double2 (&acc)[R], const double *__restrict__ c, const int n_rows, const double2 v) {
    constexpr int CW = CPLX ? 2 : 1;
    const int last = n_rows - 1;
    if constexpr (CPLX) {
#pragma unroll
        for (int o = 0; o < R; ++o) {
            const int oc = o < last ? o : last;
            const LinTerm t{0, 0, c[CW * oc], c[CW * oc + 1]};
            ent_fma<CPLX, VEC>(acc[o], t, v);
        }
    } else {
#pragma unroll
        for (int o0 = 0; o0 < R; o0 += CELL_CHUNK) {
            if (o0 + CELL_CHUNK <= n_rows) {
#pragma unroll
                for (int o = o0; o < o0 + CELL_CHUNK; ++o) ent_fma<CPLX, VEC>(acc[o], LinTerm{0, 0, c[o], 0.}, v);
            } else if (o0 < n_rows) {
#pragma unroll
                for (int o = o0; o < o0 + CELL_CHUNK; ++o) ent_fma<CPLX, VEC>(acc[o], LinTerm{0, 0, c[o < last ? o : last], 0.}, v);
            }
        }
    }
}

template <bool CPLX, bool VEC, int R>
__device__ __forceinline__ void mpo_cell_job(const CellJob &J, const int n_store, const CellRow *__restrict__ rows,
                                             const CellSrc *__restrict__ S, const double *__restrict__ coeff,
                                             const double *__restrict__ src, double *__restrict__ dst) {
    constexpr int EPI = (!CPLX && VEC) ? 2 : 1;        // elements per item
    constexpr int CW = CPLX ? 2 : 1;                   // doubles per element
    const int n_rows = (int)J.n_rows, ns = (int)J.n_src;
    const int64_t post_items = J.post / EPI;
    const int64_t n_cols = J.pre * post_items;
    const double *C = coeff + CW * J.coeff_off;
    const int64_t cs = (int64_t)CW * n_rows;           // doubles from the coefficients of source k to those of source k + 1
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n_cols; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / post_items, j = (e - i * post_items) * EPI;
        const double *x0 = src + CW * j;
        double2 acc[R];
#pragma unroll
        for (int o = 0; o < R; ++o) acc[o] = double2{0., 0.};
        int k = 0;
        for (; k + 4 <= ns; k += 4) {
            const double2 v0 = ent_load<CPLX, VEC>(x0 + CW * (S[k].src_off + i * S[k].src_ld));
            const double2 v1 = ent_load<CPLX, VEC>(x0 + CW * (S[k + 1].src_off + i * S[k + 1].src_ld));
            const double2 v2 = ent_load<CPLX, VEC>(x0 + CW * (S[k + 2].src_off + i * S[k + 2].src_ld));
            const double2 v3 = ent_load<CPLX, VEC>(x0 + CW * (S[k + 3].src_off + i * S[k + 3].src_ld));
            cell_update<CPLX, VEC, R>(acc, C + k * cs, n_rows, v0);
            cell_update<CPLX, VEC, R>(acc, C + (k + 1) * cs, n_rows, v1);
            cell_update<CPLX, VEC, R>(acc, C + (k + 2) * cs, n_rows, v2);
            cell_update<CPLX, VEC, R>(acc, C + (k + 3) * cs, n_rows, v3);
        }
        for (; k < ns; ++k)
            cell_update<CPLX, VEC, R>(acc, C + k * cs, n_rows, ent_load<CPLX, VEC>(x0 + CW * (S[k].src_off + i * S[k].src_ld)));
        double *y = dst + CW * (J.dst_off + i * J.dst_ld + j);
#pragma unroll
        for (int o = 0; o < R; ++o) {
            if (o < n_store) {
                double *yo = y + CW * rows[o].dst_row_off;
                if (VEC) {
                    *reinterpret_cast<double2 *>(yo) = acc[o];
                } else {
                    yo[0] = acc[o].x;
                    if (CPLX) yo[1] = acc[o].y;
                }
            }
        }
    }
}

template <bool CPLX, bool VEC, int R>
__global__ __launch_bounds__(NT) void mpo_cell_kernel(const CellJob *__restrict__ jobs, const CellRow *__restrict__ rows,
                                                      const CellSrc *__restrict__ srcs, const double *__restrict__ coeff, const int max_rows,
                                                      const double *__restrict__ src, double *__restrict__ dst) {
    const CellJob J = jobs[blockIdx.y];
    if (J.pre <= 0 || J.n_rows <= 0 || J.post <= 0) return;
    if ((int64_t)blockIdx.x * NT >= J.pre * J.post) return;      // the grid is sized by the largest job: nothing left for this workgroup
    const CellRow *Rw = rows + J.row_begin;
    const CellSrc *S = srcs + J.src_begin;
    const int n_store = J.n_rows < max_rows ? (int)J.n_rows : max_rows;      // (max_rows <= R: rows beyond it are not written)
    if (VEC && !CPLX) {         // two real elements per item: every address of the job has to stay on a 16-byte boundary
        bool even = ((J.post | J.dst_off | J.dst_ld) & 1) == 0;
        // every wavefront scans the tables of the job, lane l the entries l, l + 64, ...: the same answer in all of them
        for (int64_t o = threadIdx.x & 63; o < n_store; o += 64) even = even && (Rw[o].dst_row_off & 1) == 0;
        for (int64_t k = threadIdx.x & 63; k < J.n_src; k += 64) even = even && ((S[k].src_off | S[k].src_ld) & 1) == 0;
        if (!__all(even)) {
            mpo_cell_job<CPLX, false, R>(J, n_store, Rw, S, coeff, src, dst);
            return;
        }
    }
    mpo_cell_job<CPLX, VEC, R>(J, n_store, Rw, S, coeff, src, dst);
}

struct ScaleJob {  // int64[6]
    int64_t x_off, pre, len, post, s_off, pad;
};

template <bool CPLX, bool SCPLX>
__global__ __launch_bounds__(NT) void scale_axis_kernel(const ScaleJob *__restrict__ jobs,
                                                        double *__restrict__ x,
                                                        const double *__restrict__ s) {
    const ScaleJob J = jobs[blockIdx.y];
    const int64_t total = J.pre * J.len * J.post;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t j = (e / J.post) % J.len;
        if (!CPLX) {
            x[J.x_off + e] *= s[J.s_off + j];
        } else {
            double2 v = reinterpret_cast<double2 *>(x)[J.x_off + e];
            if (SCPLX) {
                const double2 f = reinterpret_cast<const double2 *>(s)[J.s_off + j];
                v = double2{v.x * f.x - v.y * f.y, v.x * f.y + v.y * f.x};
            } else {
                const double f = s[J.s_off + j];
                v.x *= f;
                v.y *= f;
            }
            reinterpret_cast<double2 *>(x)[J.x_off + e] = v;
        }
    }
}

struct GatherJob {  // int64[8]
    int64_t dst_off, src_off, pre, len_src, len_dst, post, idx_off, pad;
};

template <bool CPLX>
__global__ __launch_bounds__(NT) void gather_axis_kernel(const GatherJob *__restrict__ jobs,
                                                         const int64_t *__restrict__ idx,
                                                         const double *__restrict__ src,
                                                         double *__restrict__ dst) {
    const GatherJob J = jobs[blockIdx.y];
    const int64_t total = J.pre * J.len_dst * J.post;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t l = e % J.post;
        const int64_t t = e / J.post;
        const int64_t j = t % J.len_dst;
        const int64_t i = t / J.len_dst;
        const int64_t so = J.src_off + (i * J.len_src + idx[J.idx_off + j]) * J.post + l;
        if (CPLX)
            reinterpret_cast<double2 *>(dst)[J.dst_off + e] = reinterpret_cast<const double2 *>(src)[so];
        else
            dst[J.dst_off + e] = src[so];
    }
}

// out[o_off + j] = sum_{i,l} |x[i, j, l]|^2 for blocks viewed as (pre, len, post): the per-slice norms that
// _qr_theta_Y0 takes with np.linalg.norm(block, axis=...) (truncation.py:452).  One wavefront per (job, j).
struct NormJob {  // int64[6]
    int64_t x_off, pre, len, post, o_off, pad;
};
template <bool CPLX>
__global__ __launch_bounds__(NT) void axis_sqnorm_kernel(const NormJob *__restrict__ jobs,
                                                         const int2 *__restrict__ rows,
                                                         const double *__restrict__ x, double *__restrict__ out) {
    const int gw = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int2 jr = rows[gw];
    if (jr.x < 0) return;
    const NormJob J = jobs[jr.x];
    const int64_t j = jr.y;
    double s = 0;
    const int64_t cnt = J.pre * J.post;
    for (int64_t e = lane; e < cnt; e += 64) {
        const int64_t i = e / J.post, l = e - i * J.post;
        const int64_t idx = J.x_off + (i * J.len + j) * J.post + l;
        if (CPLX) {
            const double2 v = reinterpret_cast<const double2 *>(x)[idx];
            s += v.x * v.x + v.y * v.y;
        } else {
            s = fma(x[idx], x[idx], s);
        }
    }
    s = wave_sum(s);
    if (lane == 0) out[J.o_off + j] = s;
}

// dtype conversion / conjugation over a flat arena.  MODE 0: f64->f64 copy, 1: f64->c128, 2: c128->f64 (real
// part), 3: c128->c128 (optionally conjugated)
template <int MODE>
__global__ __launch_bounds__(NT) void convert_kernel(int64_t n, const double *__restrict__ src,
                                                     double *__restrict__ dst, int conj) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        if (MODE == 0) {
            dst[i] = src[i];
        } else if (MODE == 1) {
            reinterpret_cast<double2 *>(dst)[i] = double2{src[i], 0.0};
        } else if (MODE == 2) {
            dst[i] = reinterpret_cast<const double2 *>(src)[i].x;
        } else {
            double2 v = reinterpret_cast<const double2 *>(src)[i];
            if (conj) v.y = -v.y;
            reinterpret_cast<double2 *>(dst)[i] = v;
        }
    }
}

inline int grid_x(int64_t max_elems) {
    int64_t g = (max_elems + NT * 4 - 1) / (NT * 4);
    if (g < 1) g = 1;
    if (g > 512) g = 512;
    return (int)g;
}
}  // namespace

extern "C" int tpa_copy_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int64_t max_job_elems,
                              const void *src_base, void *dst_base, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    dim3 grid(grid_x(max_job_elems), n_jobs);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        copy_batch_kernel<false><<<grid, NT, 0, st>>>((const CopyJob *)jobs_dev, (const double *)src_base, (double *)dst_base);
    else
        copy_batch_kernel<true><<<grid, NT, 0, st>>>((const CopyJob *)jobs_dev, (const double *)src_base, (double *)dst_base);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_lincomb_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *terms_dev,
                                 int64_t max_job_elems, const void *src_base, void *dst_base, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    dim3 grid(grid_x(max_job_elems), n_jobs);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        lincomb_kernel<false><<<grid, NT, 0, st>>>((const LinJob *)jobs_dev, (const LinTerm *)terms_dev, (const double *)src_base, (double *)dst_base);
    else
        lincomb_kernel<true><<<grid, NT, 0, st>>>((const LinJob *)jobs_dev, (const LinTerm *)terms_dev, (const double *)src_base, (double *)dst_base);
    TPA_LAUNCH_CHECK();
    return 0;
}

template <bool CPLX, bool VEC>
static void mpo_apply_launch(int max_d, dim3 grid, hipStream_t st, const int64_t *jobs_dev, const int64_t *terms_dev, const void *coeff_dev,
                             const void *src_base, void *dst_base) {
    const MpoJob *jobs = (const MpoJob *)jobs_dev;
    const MpoTerm *terms = (const MpoTerm *)terms_dev;
    const double *coeff = (const double *)coeff_dev, *src = (const double *)src_base;
    double *dst = (double *)dst_base;
    if (max_d <= 2)
        mpo_apply_kernel<CPLX, 2, VEC><<<grid, NT, 0, st>>>(jobs, terms, coeff, src, dst);
    else if (max_d <= 4)
        mpo_apply_kernel<CPLX, 4, VEC><<<grid, NT, 0, st>>>(jobs, terms, coeff, src, dst);
    else if (max_d <= 8)
        mpo_apply_kernel<CPLX, 8, VEC><<<grid, NT, 0, st>>>(jobs, terms, coeff, src, dst);
    else
        mpo_apply_kernel<CPLX, 16, VEC><<<grid, NT, 0, st>>>(jobs, terms, coeff, src, dst);
}

extern "C" int tpa_mpo_apply_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *terms_dev, const void *coeff_dev,
                                   int max_d, int64_t max_job_elems, const void *src_base, void *dst_base, void *stream) {
    static_assert(TPA_MPO_APPLY_MAXD == 16, "mpo_apply_launch dispatches up to 16 accumulators");
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(max_d >= 1 && max_d <= TPA_MPO_APPLY_MAXD);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    int64_t g = (max_job_elems / max_d + NT - 1) / NT;
    if (g < 1) g = 1;
    if (g > 512) g = 512;
    dim3 grid((int)g, n_jobs);
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = (((uintptr_t)src_base | (uintptr_t)dst_base) & 15) == 0;
    if (dtype == TPA_F64) {
        if (aligned)
            mpo_apply_launch<false, true>(max_d, grid, st, jobs_dev, terms_dev, coeff_dev, src_base, dst_base);
        else
            mpo_apply_launch<false, false>(max_d, grid, st, jobs_dev, terms_dev, coeff_dev, src_base, dst_base);
    } else {
        if (aligned)
            mpo_apply_launch<true, true>(max_d, grid, st, jobs_dev, terms_dev, coeff_dev, src_base, dst_base);
        else
            mpo_apply_launch<true, false>(max_d, grid, st, jobs_dev, terms_dev, coeff_dev, src_base, dst_base);
    }
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_mpo_entry_apply_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *rows_dev, const int64_t *terms_dev,
                                         int64_t max_job_cols, const void *src_base, void *dst_base, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    const bool aligned = (((uintptr_t)src_base | (uintptr_t)dst_base) & 15) == 0;
    const int64_t items = (dtype == TPA_F64 && aligned) ? (max_job_cols + 1) / 2 : max_job_cols;
    int64_t g = (items + NT - 1) / NT;
    if (g < 1) g = 1;
    if (g > 512) g = 512;
    dim3 grid((int)g, n_jobs);
    hipStream_t st = (hipStream_t)stream;
    const EntJob *jobs = (const EntJob *)jobs_dev;
    const EntRow *rows = (const EntRow *)rows_dev;
    const LinTerm *terms = (const LinTerm *)terms_dev;
    const double *src = (const double *)src_base;
    double *dst = (double *)dst_base;
    if (dtype == TPA_F64) {
        if (aligned)
            mpo_entry_apply_kernel<false, true><<<grid, NT, 0, st>>>(jobs, rows, terms, src, dst);
        else
            mpo_entry_apply_kernel<false, false><<<grid, NT, 0, st>>>(jobs, rows, terms, src, dst);
    } else {
        if (aligned)
            mpo_entry_apply_kernel<true, true><<<grid, NT, 0, st>>>(jobs, rows, terms, src, dst);
        else
            mpo_entry_apply_kernel<true, false><<<grid, NT, 0, st>>>(jobs, rows, terms, src, dst);
    }
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_mpo_expand_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *rows_dev, const int64_t *terms_dev,
                                    int64_t max_job_cols, const void *src_base, const void *src2_base, void *dst_base, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    const bool aligned = (((uintptr_t)src_base | (uintptr_t)src2_base | (uintptr_t)dst_base) & 15) == 0;
    const int64_t items = (dtype == TPA_F64 && aligned) ? (max_job_cols + 1) / 2 : max_job_cols;
    int64_t g = (items + NT - 1) / NT;
    if (g < 1) g = 1;
    if (g > 512) g = 512;
    dim3 grid((int)g, n_jobs);
    hipStream_t st = (hipStream_t)stream;
    const EntJob *jobs = (const EntJob *)jobs_dev;
    const ExpRow *rows = (const ExpRow *)rows_dev;
    const LinTerm *terms = (const LinTerm *)terms_dev;
    const double *src = (const double *)src_base, *src2 = (const double *)src2_base;
    double *dst = (double *)dst_base;
    if (dtype == TPA_F64) {
        if (aligned)
            mpo_expand_kernel<false, true><<<grid, NT, 0, st>>>(jobs, rows, terms, src, src2, dst);
        else
            mpo_expand_kernel<false, false><<<grid, NT, 0, st>>>(jobs, rows, terms, src, src2, dst);
    } else {
        if (aligned)
            mpo_expand_kernel<true, true><<<grid, NT, 0, st>>>(jobs, rows, terms, src, src2, dst);
        else
            mpo_expand_kernel<true, false><<<grid, NT, 0, st>>>(jobs, rows, terms, src, src2, dst);
    }
    TPA_LAUNCH_CHECK();
    return 0;
}

template <bool CPLX, bool VEC>
static void mpo_cell_launch(int max_rows, dim3 grid, hipStream_t st, const int64_t *jobs_dev, const int64_t *rows_dev, const int64_t *srcs_dev,
                            const void *coeff_dev, const void *src_base, void *dst_base) {
    const CellJob *jobs = (const CellJob *)jobs_dev;
    const CellRow *rows = (const CellRow *)rows_dev;
    const CellSrc *srcs = (const CellSrc *)srcs_dev;
    const double *coeff = (const double *)coeff_dev, *src = (const double *)src_base;
    double *dst = (double *)dst_base;
    if (max_rows <= 8)
        mpo_cell_kernel<CPLX, VEC, 8><<<grid, NT, 0, st>>>(jobs, rows, srcs, coeff, max_rows, src, dst);
    else if (max_rows <= 16)
        mpo_cell_kernel<CPLX, VEC, 16><<<grid, NT, 0, st>>>(jobs, rows, srcs, coeff, max_rows, src, dst);
    else
        mpo_cell_kernel<CPLX, VEC, 32><<<grid, NT, 0, st>>>(jobs, rows, srcs, coeff, max_rows, src, dst);
}

extern "C" int tpa_mpo_cell_apply_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *rows_dev, const int64_t *srcs_dev,
                                        const void *coeff_dev, int max_rows, int64_t max_job_cols, const void *src_base, void *dst_base,
                                        void *stream) {
    static_assert(TPA_MPO_CELL_MAXROWS == 32, "mpo_cell_launch dispatches up to 32 accumulators");
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(max_rows >= 1 && max_rows <= TPA_MPO_CELL_MAXROWS);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    const bool aligned = (((uintptr_t)src_base | (uintptr_t)dst_base) & 15) == 0;
    const int64_t items = (dtype == TPA_F64 && aligned) ? (max_job_cols + 1) / 2 : max_job_cols;
    int64_t g = (items + NT - 1) / NT;
    if (g < 1) g = 1;
    if (g > 512) g = 512;
    dim3 grid((int)g, n_jobs);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64) {
        if (aligned)
            mpo_cell_launch<false, true>(max_rows, grid, st, jobs_dev, rows_dev, srcs_dev, coeff_dev, src_base, dst_base);
        else
            mpo_cell_launch<false, false>(max_rows, grid, st, jobs_dev, rows_dev, srcs_dev, coeff_dev, src_base, dst_base);
    } else {
        if (aligned)
            mpo_cell_launch<true, true>(max_rows, grid, st, jobs_dev, rows_dev, srcs_dev, coeff_dev, src_base, dst_base);
        else
            mpo_cell_launch<true, false>(max_rows, grid, st, jobs_dev, rows_dev, srcs_dev, coeff_dev, src_base, dst_base);
    }
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_scale_axis_batch(int dtype, const int64_t *jobs_dev, int n_jobs,
                                    int64_t max_job_elems, void *x_base, const void *s_dev,
                                    int s_is_complex, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    TPA_ARG_CHECK(!(dtype == TPA_F64 && s_is_complex));
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    dim3 grid(grid_x(max_job_elems), n_jobs);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        scale_axis_kernel<false, false><<<grid, NT, 0, st>>>((const ScaleJob *)jobs_dev, (double *)x_base, (const double *)s_dev);
    else if (s_is_complex)
        scale_axis_kernel<true, true><<<grid, NT, 0, st>>>((const ScaleJob *)jobs_dev, (double *)x_base, (const double *)s_dev);
    else
        scale_axis_kernel<true, false><<<grid, NT, 0, st>>>((const ScaleJob *)jobs_dev, (double *)x_base, (const double *)s_dev);
    TPA_LAUNCH_CHECK();
    return 0;
}

// Ordered (Gram-Schmidt like) orthonormalisation step on the Gram matrix G = T T^H of row vectors sorted by DESCENDING weight:
// G <- strict lower triangle of G, diagonal (G_ii - 1) / 2, zero above.  Then T <- T - G T makes every vector orthogonal to the
// vectors BEFORE it (to second order in the defect) and moves no vector towards a later one: the clean-up of the small singular
// vectors of the block SVD (tenpy_amd/linalg/_svd_warm.py::ordered_rows).  jobs: int64[n][2] = {g_off, n}.
struct TriJob {
    int64_t g_off, n;
};

template <bool CPLX>
__global__ __launch_bounds__(NT) void tri_lower_kernel(const TriJob *__restrict__ jobs, double *__restrict__ g) {
    const TriJob J = jobs[blockIdx.y];
    const int64_t total = J.n * J.n;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / J.n, j = e - i * J.n;
        if (!CPLX) {
            double v = g[J.g_off + e];
            v = (i > j) ? v : (i == j) ? 0.5 * (v - 1.0) : 0.0;
            g[J.g_off + e] = v;
        } else {
            double2 v = reinterpret_cast<double2 *>(g)[J.g_off + e];
            v = (i > j) ? v : (i == j) ? double2{0.5 * (v.x - 1.0), 0.0} : double2{0.0, 0.0};
            reinterpret_cast<double2 *>(g)[J.g_off + e] = v;
        }
    }
}

extern "C" int tpa_tri_lower_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int64_t max_job_elems, void *g_base,
                                   void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    dim3 grid(grid_x(max_job_elems), n_jobs);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        tri_lower_kernel<false><<<grid, NT, 0, st>>>((const TriJob *)jobs_dev, (double *)g_base);
    else
        tri_lower_kernel<true><<<grid, NT, 0, st>>>((const TriJob *)jobs_dev, (double *)g_base);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_gather_axis_batch(int dtype, const int64_t *jobs_dev, int n_jobs,
                                     int64_t max_job_elems, const int64_t *idx_dev,
                                     const void *src_base, void *dst_base, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_jobs <= 0) return 0;
    TPA_ARG_CHECK(n_jobs <= 65535);
    dim3 grid(grid_x(max_job_elems), n_jobs);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        gather_axis_kernel<false><<<grid, NT, 0, st>>>((const GatherJob *)jobs_dev, idx_dev, (const double *)src_base, (double *)dst_base);
    else
        gather_axis_kernel<true><<<grid, NT, 0, st>>>((const GatherJob *)jobs_dev, idx_dev, (const double *)src_base, (double *)dst_base);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_convert(int from_dtype, int to_dtype, int64_t n, const void *src, void *dst, int conj,
                           void *stream) {
    TPA_ARG_CHECK((from_dtype == TPA_F64 || from_dtype == TPA_C128) && (to_dtype == TPA_F64 || to_dtype == TPA_C128));
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    int g = grid_x(n) * 4;
    if (g > 2048) g = 2048;
    if (from_dtype == TPA_F64 && to_dtype == TPA_F64)
        convert_kernel<0><<<g, NT, 0, st>>>(n, (const double *)src, (double *)dst, 0);
    else if (from_dtype == TPA_F64)
        convert_kernel<1><<<g, NT, 0, st>>>(n, (const double *)src, (double *)dst, 0);
    else if (to_dtype == TPA_F64)
        convert_kernel<2><<<g, NT, 0, st>>>(n, (const double *)src, (double *)dst, 0);
    else
        convert_kernel<3><<<g, NT, 0, st>>>(n, (const double *)src, (double *)dst, conj);
    TPA_LAUNCH_CHECK();
    return 0;
}

extern "C" int tpa_axis_sqnorm_batch(int dtype, const int64_t *jobs_dev, const int32_t *rows_dev, int n_rows,
                                     const void *x_base, double *out_dev, void *stream) {
    TPA_ARG_CHECK(dtype == TPA_F64 || dtype == TPA_C128);
    if (n_rows <= 0) return 0;
    TPA_ARG_CHECK(n_rows % (NT / 64) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TPA_F64)
        axis_sqnorm_kernel<false><<<n_rows / (NT / 64), NT, 0, st>>>((const NormJob *)jobs_dev, (const int2 *)rows_dev, (const double *)x_base, out_dev);
    else
        axis_sqnorm_kernel<true><<<n_rows / (NT / 64), NT, 0, st>>>((const NormJob *)jobs_dev, (const int2 *)rows_dev, (const double *)x_base, out_dev);
    TPA_LAUNCH_CHECK();
    return 0;
}
