/* tenpy_amd.h -- C-ABI of the MI355X (gfx950) backend for TeNPy's block-sparse hot path.
 *
 * Every entry point replaces one native call site of the reference
 * (tenpy/linalg/_npc_helper.pyx, tenpy/linalg/np_conserved.py; cited per function).
 * Conventions:
 *   - all pointers named *_dev / *base are DEVICE pointers (HBM); `stream` is a hipStream_t
 *     passed as void* (NULL = default stream); everything is asynchronous on that stream
 *     unless the doc says "synchronises".
 *   - dtype: TPA_F64 (real double) or TPA_C128 (interleaved complex double) -- the only two
 *     calculation dtypes of the reference (_npc_helper.pyx:410-424 `_find_calc_dtype`).
 *   - block data: an Array's blocks are packed back to back in ONE device arena; a block is
 *     addressed as (arena base, element offset).  Offsets / sizes are in ELEMENTS of dtype.
 *   - return value: 0 = ok, >0 = hipError_t of the failing runtime call,
 *     <0 = TPA_E_* argument/algorithm error (mapped to ValueError / RuntimeError /
 *     LinAlgError by the Python shim, SURVEY 8(b) "Errors").
 */
#ifndef TENPY_AMD_H
#define TENPY_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TPA_F64 0
#define TPA_C128 1

#define TPA_E_BADARG (-1)      /* -> ValueError  */
#define TPA_E_NOCONV (-2)      /* -> numpy.linalg.LinAlgError (Jacobi sweeps exhausted)  */
#define TPA_E_NAN (-3)         /* -> ValueError("NaN ...") like np_conserved.py:4978-4982 */
#define TPA_E_NOMEM (-4)
#define TPA_E_RANKCAP (-5)     /* tpa_svd_batch with a rank cap: a block is not of low rank (caller falls back) */

/* ---- library / device --------------------------------------------------------------- */
int tpa_version(void);
/* Fills name (<=255 chars), number of CUs, HBM bytes of the current device. */
int tpa_device_info(char *name, int name_len, int *n_cu, int64_t *hbm_bytes);
const char *tpa_last_error(void);

/* ---- K1: grouped, chained GEMM  (replaces CblasGemmBatch.run, _npc_helper.pyx:204-273;
 *          python twin `fast_dot_sum`, np_conserved.py:4807-4837) ----------------------
 * The reference queues (A,B,C,m,k,n) per accumulation *level* and runs level 0 with beta=0
 * and later levels with beta=1.  Here the levels of one C block form a *chain* that is
 * accumulated in MFMA registers (no beta=1 re-read of C):
 *        C_t (m x n, row stride ldc)  =  [C_t +]  sum_{l in chain(t)} A_l (m x k_l) * B_l (k_l x n)
 * links  : int64[n_links][8]  = {a_off, b_off, k, a_rs, a_ks, b_ks, b_ns, flags}
 *          A_l(i,kk) = Abase[a_off + i*a_rs + kk*a_ks], B_l(kk,j) = Bbase[b_off + kk*b_ks + j*b_ns]
 *          (one of a_rs/a_ks and one of b_ks/b_ns should be 1 for coalescing; any strides are legal)
 *          flags bit0: conj(A), bit1: conj(B)   (complex only)
 *          links with k <= 0 are skipped wherever they stand in a chain; a chain without a non-empty link gives C_t = 0
 *          (accumulate = 0) or leaves C_t as it is (accumulate = 1).  Real data ignores the flags.
 * tasks  : int64[n_tasks][8]  = {c_off, m, n, ldc, link_begin, link_count, accumulate, act}
 * tiles  : int32[n_tiles][4]  = {task, tile_row, tile_col, w}   (tile shape: tpa_gemm_tile_shape(dtype, cfg))
 *          Every task is covered by its tiles exactly once, in any order.  Only the m x n elements of a block are written: the
 *          ldc - n elements behind a row and everything between the blocks keep their contents.
 * Identity-row skip (act, w; every caller but the block SVD leaves both 0).  `act` is 0 or the address of int32 words in DEVICE
 *          memory; a tile with w > 0 of a task with act != 0 looks at ((const int32_t *)act)[w - 1].  A word of 0 is the caller's
 *          promise that the rows of A which this tile needs are unit vectors, A(i, kk) = (i == kk) for the rows i of the tile (the
 *          rows of the accumulated rotation Qtot of a block-Jacobi sweep that did not rotate: tpa_svd.hip, [W | G] <- Qtot [W | G]).
 *          The tile of C is then a COPY of the rows of B: C(i, j) = B_l(i, j) of the FIRST link l = link_begin of the chain --
 *          bit for bit what the product gives, because sums of exact zeros and one exact 1 * b do not round.  The copy does not
 *          look at `accumulate`, at flags bit1 or at further links: the skip is for tasks with accumulate = 0 whose chain is that
 *          one link (with k >= m; later links empty) without conj(B).  A non-zero word, w = 0 or act = 0 mean the ordinary product.
 * cfg    : 0 = large tiles (128 x 128 real), 1 = small tiles (64 x 64 real) -- chosen per plan by the host
 *          so that the launch has enough workgroups for 256 CUs.
 * All three tables live on the DEVICE (uploaded once per cached contraction plan).
 */
int tpa_gemm_chain(int dtype, int cfg, const int64_t *tasks_dev, const int64_t *links_dev,
                   const int32_t *tiles_dev, int n_tiles, const void *Abase, const void *Bbase,
                   void *Cbase, void *stream);
/* The same launch with EXTENDED LINKS (TPA_F64 only; TPA_E_BADARG for another dtype or when A2base or alphas_dev is NULL).  Tables as
 * above, and in link.flags:
 *   bit 2       second source: A_l is read from A2base instead of Abase (a chain may mix both);
 *   bits 16-31  scale: index i into alphas_dev, an array of (re, im) PAIRS of doubles (real data uses the first of a pair); i = 0 means
 *               no scale.  Every element of A_l is multiplied by alphas[2 i] on its way into LDS -- one rounding, the single-term
 *               product of tpa_lincomb_batch: a scaled link gives bit for bit what tpa_gemm_chain gives on a copy of the block
 *               that tpa_lincomb_batch scaled.  A chain without an extended link gives the bits of tpa_gemm_chain;
 *   bit 3       unit factor: B_l is the unit matrix and the link adds alpha * A_l(row, col) to C_t(row, col), read from global memory
 *               in the epilogue with the strides a_rs (row) and a_ks (column); A_l is m x n.  Store such links with k = 0.  Their
 *               terms are added to the sum of the products in chain order, before `accumulate`; a chain may consist of them alone.
 * A2base and alphas_dev are read only by links that ask for them. */
int tpa_gemm_chain_ex(int dtype, int cfg, const int64_t *tasks_dev, const int64_t *links_dev, const int32_t *tiles_dev, int n_tiles,
                      const void *Abase, const void *A2base, const void *Bbase, void *Cbase, const double *alphas_dev, void *stream);

/* Which of the two loops a launch of n_tiles tiles runs on: 0 = gemm_chain_kernel, 1 = gemm_chain2_kernel (host only; follows
 * tpa_gemm_set_variant).  Both give their own bits: a caller that drops tiles from a launch and wants the bits of the full launch keeps
 * the answer the same. */
int tpa_gemm_kernel_id(int dtype, int cfg, int n_tiles);

/* Largest |B(i, j) - delta_ij| over a list of square blocks, exact (a maximum, no sums): jobs int64[n_jobs][4] = {offset, n, row
 * stride, 0} in elements of `dtype` relative to src_base (DEVICE table).  out_dev[0] (one DEVICE double) receives the result, 0 for an
 * empty list, +inf if an entry is NaN.  Asynchronous on `stream`.  n_jobs <= 65535. */
int tpa_unit_defect_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const void *src_base, double *out_dev, void *stream);

/* ---- K1h: grouped, chained, weighted Hermitian rank-k update  (the contraction in the middle of
 *          DensityMatrixMixer.mix_rho, mps_common.py:2002-2026: rho = X diag(mix) X^dagger per charge sector, which the
 *          reference forms with conj(), iscale_axis and a general tensordot) -------------------------------------------
 *        C_t (m x n, row stride ldc)  =  [C_t +]  sum_{l in chain(t)} sum_kk  s_l(kk) * A_l(i,kk) * conj(B_l(j,kk))
 * links  : int64[n_links][12] = {a_off, b_off, k, a_rs, a_ks, b_rs, b_ks, w_off, w_len, w_inner, 0, 0}
 *          A_l(i,kk) = Abase[a_off + i*a_rs + kk*a_ks], B_l(j,kk) = Bbase[b_off + j*b_rs + kk*b_ks]; Abase and Bbase may coincide.
 *          (one of each pair of strides should be 1 for coalescing -- the left mixer has k fast, the right mixer the row; any
 *          strides are legal)
 *          s_l(kk) = wvec_dev[w_off + (kk / w_inner) % w_len], a REAL (double) weight whatever the dtype; w_off < 0: s_l = 1 and
 *          wvec_dev is not read.  w_len >= 1, w_inner >= 1.  A scalar weight per link is w_len = 1 (MPO bond blocks of width 1);
 *          the modulo form covers an MPO bond block of width w_len that sits anywhere among the contracted legs (w_inner = the
 *          product of the dimensions of the contracted legs behind it).  The weight is multiplied into A_l(i,kk) first (one
 *          rounding), the products are summed in MFMA registers.  Zero and negative weights are ordinary data.
 *          links with k <= 0 are skipped wherever they stand in a chain; a chain without a non-empty link gives C_t = 0
 *          (accumulate = 0) or leaves C_t as it is (accumulate = 1).  Real data: no conjugation.
 * tasks  : int64[n_tasks][10] = {c_off, m, n, ldc, link_begin, link_count, accumulate, herm, mirror_off, mirror_ldc}
 *          herm != 0 (Hermitian task): m == n and A_l == B_l (same base, offset and strides) for every link of the chain.  Only the
 *          tiles with tile_row >= tile_col are scheduled (a tile above the diagonal is ignored).  The kernel writes C[i,j] for
 *          i >= j and the mirror C[j,i] = conj(C[i,j]) from the same register, and Im C[i,i] = 0: after the call the m x m block is
 *          Hermitian bit for bit.  With accumulate = 1 the elements C[i,j], i >= j, are read (the imaginary part of an old diagonal
 *          element is dropped); the old upper triangle is not.  mirror_off / mirror_ldc are ignored.
 *          herm == 0 (general task: the rectangle between two different slices of one charge sector): the kernel writes the m x n
 *          rectangle at c_off and, if mirror_off >= 0, its conjugate transpose (n x m, row stride mirror_ldc) at mirror_off of the
 *          same arena: M[j,i] = conj(C[i,j]), the value stored at C (after accumulation).  The two rectangles must not overlap.
 * tiles  : int32[n_tiles][4]  = {task, tile_row, tile_col, 0}; square tiles of tpa_herk_tile_shape(dtype) rows, built on the
 *          host as for tpa_gemm_chain (longest chains first).  A general task is covered by all of its tiles exactly once, a
 *          Hermitian task by its tiles on and below the diagonal.  Only the elements of the blocks (and mirrors) are written.
 * Asynchronous on `stream`; TPA_E_BADARG for a dtype that is neither TPA_F64 nor TPA_C128; n_tiles <= 0 returns 0 without a
 * launch.  Two identical calls give identical bits.  All three tables and wvec live on the DEVICE.
 */
int tpa_herk_tile_shape(int dtype, int *bt);      /* TPA_E_BADARG for another dtype or bt == NULL */
int tpa_herk_chain(int dtype, const int64_t *tasks_dev, const int64_t *links_dev, const int32_t *tiles_dev, int n_tiles,
                   const void *Abase, const void *Bbase, const double *wvec_dev, void *Cbase, void *stream);

/* ---- K2-K4: vector kernels over packed arenas (replace ddot/zdotc/zdotu
 *      _npc_helper.pyx:1854-1871, daxpy/zaxpy :316-336, dscal/zscal :339-364,
 *      np.linalg.norm per block np_conserved.py:2252-2255) ------------------------------
 * `n` counts elements of dtype.  Scalars alpha are passed as (re, im); im ignored for F64.
 * Reductions are deterministic two-pass (per-workgroup partials, then one workgroup);
 * `scratch_dev` must hold >= TPA_RED_SCRATCH doubles; the result (2 doubles: re, im) is
 * written to out_dev[0..1] on the stream (no host sync); two identical calls give bit-identical results.
 * n <= 0: tpa_axpy and tpa_scal return 0 without a launch.  tpa_dot, tpa_nrm2sq and tpa_lanczos_update read and write no vector
 * element and post out_dev[0..1] = (0, 0); tpa_lanczos_step posts ab_out[0..1] = (0, 0) and leaves w alone (as for any bsq = 0: no
 * division).  tpa_krylov_combine / tpa_krylov_combine_z return TPA_E_BADARG.  tpa_project_out: see there.
 */
#define TPA_RED_SCRATCH 4096
int tpa_axpy(int dtype, int64_t n, double alpha_re, double alpha_im, const void *x_dev,
             void *y_dev, void *stream);
int tpa_scal(int dtype, int64_t n, double alpha_re, double alpha_im, void *x_dev, void *stream);
/* out = sum conj?(x_i) * y_i ;  do_conj as in _inner_worker(a, b, do_conj) */
int tpa_dot(int dtype, int64_t n, const void *x_dev, const void *y_dev, int do_conj,
            double *out_dev, double *scratch_dev, void *stream);
/* out[0] = sum |x_i|^2  (2-norm squared; host takes the sqrt) */
int tpa_nrm2sq(int dtype, int64_t n, const void *x_dev, double *out_dev, double *scratch_dev,
               void *stream);
/* Fused Lanczos recurrence step (krylov_based.py:660-672):
 *   w -= alpha * v1 ; w -= beta * v0 (v0 may be NULL) ; out[0] = sum |w_i|^2           */
int tpa_lanczos_update(int dtype, int64_t n, void *w_dev, double alpha_re, double alpha_im,
                       const void *v1_dev, double beta_re, double beta_im, const void *v0_dev,
                       double *out_dev, double *scratch_dev, void *stream);
/* The same step with the scalars kept on the device, so that the host never waits between a matvec and the next one
 * (LanczosGroundState._build_krylov, krylov_based.py:655-672; the host reads alpha / beta one step late for the tridiagonal
 * eigen-problem and the convergence test):
 *   alpha = Re <w|v1> ;  w -= alpha v1 ;  w -= sqrt(bsq_prev[0]) v0 (v0, bsq_prev may be NULL) ;  bsq = |w|^2 ;  w /= sqrt(bsq)
 *   ab_out[0] = alpha, ab_out[1] = bsq.  scratch_dev: TPA_RED_SCRATCH doubles. */
int tpa_lanczos_step(int dtype, int64_t n, void *w_dev, const void *v1_dev, const void *v0_dev,
                     const double *bsq_prev_dev, double *ab_out_dev, double *scratch_dev, void *stream);

/* dst = src - sum_{j < m} c_j b_j with c_j = sum_i conj(b_j[i]) src[i]: the projection on the orthogonal complement of m packed
 * vectors b_j = basis_dev + j * stride (elements of dtype, stride >= n) in ONE call, the coefficients never leaving the device.
 * Replaces the m (npc.inner, iadd_prefactor_other) pairs of OrthogonalNpcLinearOperator.matvec (linalg/sparse.py:243-255) and of the
 * re-orthogonalisation of a Lanczos step (krylov_based.py:667-669).  Classical Gram-Schmidt: every c_j is taken from the same src
 * (the reference's loops are the modified form; the two agree to rounding for orthonormal b_j).
 *   coeff_dev[2 j], coeff_dev[2 j + 1] = (re, im) of c_j, written on the stream (im = 0 for F64); m <= TPA_PROJECT_MAX.
 *   dst_dev == src_dev (in place) is allowed; dst must not overlap the basis (TPA_E_BADARG where it does).
 *   nrm2_out_dev: NULL, or nrm2_out_dev[0..1] = (sum |dst_i|^2, 0) out of the pass that writes dst (deterministic two-pass reduction).
 *   work_dev: TPA_PROJECT_WORK doubles (TPA_RED_SCRATCH holds the partials of two vectors only).  Nothing outside dst[0:n],
 *   coeff[0:2m], nrm2_out[0:2] and the work area is written; the basis is only read.  Two identical calls give identical bits.
 * Traffic: itemsize n (2 m + ceil(m / 8) + 2) bytes (src once per 8 basis vectors for the coefficients, every b_j twice, src and
 * dst once for the update) against 5 m itemsize n of the dot / axpy sequence.  16-byte loads where basis, src and dst are 16-byte
 * aligned and, for F64, n and (m > 1) stride are even; 8-byte loads otherwise.
 * m = 0: dst = src (a copy where the two differ; nothing at all in place without nrm2_out_dev), nrm2 as asked; coeff is not touched.
 * n <= 0: no kernel is launched, no vector element is read or written; coeff[0:2m] and nrm2_out[0:2] are posted as zeros.
 * TPA_E_BADARG: dtype, m < 0, m > TPA_PROJECT_MAX, and for m > 0: coeff_dev NULL, or (n > 0) basis_dev NULL or stride < n; for
 * n > 0: src_dev, dst_dev or work_dev NULL.  Argument errors are found before anything is launched. */
#define TPA_PROJECT_MAX 64
#define TPA_PROJECT_WORK (2 * 1024 * (TPA_PROJECT_MAX + 1))
int tpa_project_out(int dtype, int64_t n, const void *basis_dev, int m, int64_t stride, const void *src_dev, void *dst_dev,
                    double *coeff_dev, double *nrm2_out_dev, double *work_dev, void *stream);

/* Many inner products <b| op |x_s> with a small matrix on the physical index in ONE launch pair: the closing values of all started
 * rows of MPS.correlation_function at one site (reference networks/mps.py:1312-1316: tensordot(op2, C), inner(B.conj(), Cij) -- per
 * row i -- and the one-site MPS.expectation_value, :591-596), the rows stacked on a stride of x.  A job is one pair of charge blocks:
 * b block (pre, d_b, post), x block (pre, [stack,] d_x, post) with the stack index anywhere (x_sstride), coeff the (d_b, d_x) sector
 * block of the operator, out_col the operator.
 * jobs : int64[n_jobs][12] = {b_off, b_ld, d_b, x_off, x_ld, x_sstride, d_x, pre, post, coeff_off, out_col, 0}
 *   out[2*(s*n_out + k) + (0|1)] = (re | im) of
 *      sum_{jobs with out_col == k} sum_{i<pre} sum_{j<post} sum_{o<d_b} sum_{c<d_x}
 *          conj(b[b_off + i*b_ld + o*post + j]) * coeff[coeff_off + o*d_x + c] * x[x_off + i*x_ld + s*x_sstride + c*post + j]
 *   for s < n_stack, k < n_out        (im = 0 for F64)
 * Offsets and strides in elements of dtype; coeff_dev holds elements of dtype.  1 <= max_d <= TPA_MPO_APPLY_MAXD bounds every d_b and
 * d_x of the call (it selects the register budget of the kernel, the convention of tpa_mpo_apply_batch); of a job that breaks this,
 * the terms with o >= max_d or c >= max_d are left out (the coefficient rows stay d_x apart).  x_sstride and x_ld are free: the stack
 * index may be the slowest index of a block (x_sstride = pre * x_ld) or sit between i and c.  max_job_cols = max pre * post over the
 * jobs sizes the grid.  Every out[0 : 2*n_stack*n_out] is written exactly once (columns without a job, out_col outside [0, n_out) and
 * jobs with a zero extent: zeros / no contribution); nothing else is written apart from work_dev[0 : tpa_site_inner_work(n_jobs,
 * n_stack, n_out, max_job_cols)] (doubles).  b and x are only read and may alias.  Two passes, no atomics: per-workgroup partials in
 * work_dev, then one workgroup per output adds them in a fixed order -- two identical calls give identical bits.
 * dtype, max_d, n_stack >= 1, n_out >= 1 and out_dev are checked first; then n_jobs <= 0 posts zeros to out and returns 0; n_jobs >
 * 65535 (one job per blockIdx.y) and a NULL jobs, coeff, b, x or work pointer return TPA_E_BADARG; all argument errors are found
 * before anything is launched or written.
 * Traffic: itemsize sum_jobs pre post (n_stack d_x + ceil(n_stack / 8) d_b) bytes: a thread folds conj(b) coeff of its column into
 * d_x values once per group of 8 stack slots, then streams x.  16-byte loads where b_base and x_base are 16-byte aligned and, for F64,
 * post and every offset and stride of the job (b_off, b_ld, x_off, x_ld, x_sstride) are even, decided per job; 8-byte loads
 * otherwise. */
int64_t tpa_site_inner_work(int n_jobs, int n_stack, int n_out, int64_t max_job_cols);
int tpa_site_inner_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const void *coeff_dev, int max_d, int n_stack, int n_out,
                         int64_t max_job_cols, const void *b_base, const void *x_base, double *out_dev, double *work_dev, void *stream);

/* The closing step of a reduced density matrix with the physical index pair left open, for a whole stack of rows in ONE launch pair:
 * per pair (i, j) MPS.mutinf_two_site closes rho . B_j with tensordot(rho, B.conj(), [['vR*', 'vR'], ['vL*', 'vR*']]) (reference
 * networks/mps.py:4218-4232), a product that is d^2 rows tall, and reads the result on the host; the one-site density matrix of
 * get_rho_segment (:4004) is the same contraction with x = b = theta_i and n_stack = 1, out[p', p] = rho_i[p, p'].  A job is one pair
 * of charge blocks with equal row and column sectors: b block (pre, d_b, post), x block (pre, [stack,] d_x, post) with the stack index
 * anywhere (x_sstride), the conventions of tpa_site_inner_batch; its d_b x d_x tile lies at (out_off, out_ld) inside the out_size
 * entries of one slot (for a physical leg of d states: out_size = d * d, out_ld = d, out_off = first o * d + first c of the sectors).
 * jobs : int64[n_jobs][12] = {b_off, b_ld, d_b, x_off, x_ld, x_sstride, d_x, pre, post, out_off, out_ld, 0}
 *   out[2*(s*out_size + e) + (0|1)] = (re | im) of
 *      sum_{jobs, o<d_b, c<d_x with out_off + o*out_ld + c == e} sum_{i<pre} sum_{j<post}
 *          conj(b[b_off + i*b_ld + o*post + j]) * x[x_off + i*x_ld + s*x_sstride + c*post + j]
 *   for s < n_stack, e < out_size        (im = 0 for F64)
 * Offsets and strides in elements of dtype.  1 <= max_d <= TPA_SITE_RHO_MAXD bounds every d_b and d_x of the call (it selects the
 * register budget: D = 1, 2 or 4 and 8, 4 or 2 stack slots per pass over b); of a job that breaks this, the terms with o >= max_d or
 * c >= max_d are left out.  Wider sectors are not served.  Several jobs may write one tile; tile entries with out_off + o*out_ld + c
 * outside [0, out_size), or with o*d_x + c >= min(16, out_size), contribute nothing.  max_job_cols = max pre * post over the jobs
 * sizes the grid.  Every out[0 : 2*n_stack*out_size] is written exactly once (entries that no job covers, and jobs with a zero
 * extent: exact zeros / no contribution); nothing else is written apart from work_dev[0 : tpa_site_rho_work(n_jobs, n_stack,
 * out_size, max_job_cols)] (doubles).  b and x are only read and may alias.  Two passes, no atomics: per-workgroup partials in
 * work_dev, then one workgroup per output entry gathers and adds them in a fixed order -- two identical calls give identical bits.
 * (The gather costs n_stack * out_size * n_jobs * grid tile tests: cheap for tens of jobs, not for tens of thousands under a wide stack.)
 * dtype, max_d, n_stack >= 1, out_size >= 1, n_stack * out_size < 2^31 and out_dev are checked first; then n_jobs <= 0 posts zeros to
 * out and returns 0; n_jobs > 65535 (one job per blockIdx.y) and a NULL jobs, b, x or work pointer return TPA_E_BADARG; all argument
 * errors are found before anything is launched or written.
 * Traffic: itemsize sum_jobs pre post (n_stack d_x + ceil(n_stack / S) d_b) bytes, S = 8, 4, 2 for D = 1, 2, 4.  16-byte loads where
 * b_base and x_base are 16-byte aligned and, for F64, post and every offset and stride of the job (b_off, b_ld, x_off, x_ld,
 * x_sstride) are even, decided per job; 8-byte loads otherwise. */
#define TPA_SITE_RHO_MAXD 4
int64_t tpa_site_rho_work(int n_jobs, int n_stack, int out_size, int64_t max_job_cols);
int tpa_site_rho_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int max_d, int n_stack, int out_size, int64_t max_job_cols,
                       const void *b_base, const void *x_base, double *out_dev, double *work_dev, void *stream);

/* Projective sampling of a whole stack of rows at one site: MPS.sample_measurements (reference networks/mps.py:4403-4433) computes,
 * per sample, rho = tensordot(theta.conj(), theta), reads its diagonal on the host, draws rng.choice(dim, p = diag / sum), takes
 * theta.take_slice(sigma, 'p'), reads its norm on the host and divides by it.  Here X = V . B_i holds the theta of every sample as a
 * row of a charge block (rows, d, post): tpa_sample_select_batch turns every row into probabilities and an outcome,
 * tpa_sample_gather_batch writes the chosen slices, divided by their norms, into the next stack.
 * segs   : int64[n_segs][8]   = {x_off, x_ld, d, post, sigma0, 0, 0, 0}   one charge block of x; sigma0 = the index on the site's
 *          physical leg of its first state
 * groups : int64[n_groups][4] = {seg_first, seg_count, row_first, n_rows}  the rows [row_first, row_first + n_rows) of one sector of
 *          the stack leg and its segs [seg_first, seg_first + seg_count); these have disjoint [sigma0, sigma0 + d), ascending in sigma0
 * u      : double[n_rows_total], one uniform number in [0, 1) per row;   out : double[n_rows_total][4] = {sigma, w, total, 0}
 * For row r of group g, with i = r - row_first:
 *   p[sigma] = sum_{j < post} |x[x_off + i*x_ld + (sigma - sigma0)*post + j]|^2   for every sigma a seg of g covers (inside [0, dim)),
 *   p[sigma] = 0 exactly for every other sigma < dim;
 *   total = p[0] + p[1] + ... + p[dim-1], added sequentially in this order;  cdf_k = (p[0] + ... + p[k]) / total, the same sequential sums;
 *   sigma = min(#{k : cdf_k <= u[r]}, the last sigma with p > 0);   w = sqrt(p[sigma])
 * -- numpy's Generator.choice(dim, p = p / total) with its one random() replaced by u[r]: cdf.searchsorted(u, side = 'right'); an
 * outcome with p = 0 is never chosen, u = 0 included.  total == 0 or not finite: sigma = -1, w = 0 (total as computed).  A row that no
 * group holds gets {-1, 0, 0, 0}.  Offsets and strides in elements of dtype.  1 <= dim <= TPA_SAMPLE_MAX_DIM.
 * Written: out[0 : 4*n_rows_total], every entry exactly once; nothing else -- no work area.  x, u and the tables are only read.  The
 * sums of squares are reduced in a fixed order (lanes of a wavefront by shuffles, the four wavefronts of the row's workgroup through
 * LDS), no atomics: two identical calls give identical bits.
 * TPA_E_BADARG, found before anything is launched: dtype, dim outside [1, TPA_SAMPLE_MAX_DIM], n_segs < 0 or n_groups < 0, and (for
 * n_rows_total > 0) a NULL segs, groups, x, u or out pointer.  n_rows_total <= 0 is a no-op that returns 0.
 * Traffic: itemsize * sum_segs rows d post bytes, every element of x once, plus 40 bytes per row.  16-byte loads where x_base is 16-byte
 * aligned and, for F64, post, x_off and x_ld of the seg are even, decided per seg; 8-byte loads otherwise. */
#define TPA_SAMPLE_MAX_DIM 64
int tpa_sample_select_batch(int dtype, const int64_t *segs_dev, int n_segs, const int64_t *groups_dev, int n_groups, int dim,
                            int64_t n_rows_total, const void *x_base, const double *u_dev, double *out_dev, void *stream);
/* rows : int64[n_rows][4] = {src_off, len, dst_off, out_row}
 *   dst[dst_off + j] = src[src_off + j] / out[4*out_row + 1]      for j < len
 * (reference networks/mps.py:4426-4431: theta.take_slice(sigma, 'p') / npc.norm(theta)) -- a true division, component by component
 * for C128, so the result is bitwise what the w of tpa_sample_select_batch gives; w is read from the device, it is not checked (the
 * caller has looked at out before it builds the table).  Written: the len elements of every row of the table, nothing else; rows with
 * len <= 0 write nothing.  src and out are only read; src and dst are different buffers, the destinations are disjoint.
 * TPA_E_BADARG, found before anything is launched: dtype, and (for n_rows > 0) a NULL pointer or src_base == dst_base.  n_rows <= 0 is
 * a no-op that returns 0.  Traffic: 2 itemsize sum len bytes.  16-byte loads and stores for the rows whose source and destination
 * addresses are both 16-byte aligned, 8-byte ones otherwise. */
int tpa_sample_gather_batch(int dtype, const int64_t *rows_dev, int64_t n_rows, const void *src_base, const double *out_dev,
                            void *dst_base, void *stream);

/* LanczosGroundState.run as ONE host call (krylov_based.py:645-700 `_build_krylov`; the caller keeps the reference's host
 * logic -- tridiagonal eigh :702, `_converged` :713 -- in `cb`).  The matvec is a replayed "program" of cached launches:
 *   ops : HOST int64[n_ops][12] = {kind, cfg, p0, p1, p2, count, a_slot, b_slot, c_slot, max_elems, 0, 0}
 *         kind 0: tpa_gemm_chain(dtype, cfg, tasks = p0, links = p1, tiles = p2, n_tiles = count, A, B, C)
 *         kind 1: tpa_lincomb_batch(dtype, jobs = p0, n_jobs = count, terms = p1, max_elems, src = A, dst = C); cfg = 1 marks the
 *                 reduction of the split-K partial blocks of the kind-0 op before it (timed together with that GEMM)
 *         kind 2: tpa_copy_batch(dtype, jobs = p0, n_jobs = count, max_elems, src = A, dst = C)   (pack / unpack of row panels)
 *         kind 3: the caller's collective number `cfg` -- `tpa_lanczos_set_collective` -- is invoked on the host at this point of
 *                 the program; it enqueues an exchange (RCCL all-gather of the row panels of a sharded matvec) that is
 *                 ordered on the launch stream.  The recurrence, its scalars and the stopping test stay replicated and bit-identical
 *                 on every rank, so all ranks run the same number of steps.
 *         kind 4: tpa_project_out(dtype, n, basis = A, m = count, stride = p1 (elements), src = B, dst = C, coeff = p0, no norm,
 *                 work = p0 + 2 count + 2): p0 is a device area of 2 count + 2 + TPA_PROJECT_WORK doubles.  The projector of
 *                 OrthogonalNpcLinearOperator: in front of the operator's program from slot -1 into a temporary, behind it in place
 *                 on slot -2.
 *         kind 5: {5, 0, jobs, terms, coeff, n_jobs, a_slot, max_d, c_slot, max_elems, 0, 0} -- tpa_mpo_apply_batch(dtype, jobs = p0,
 *                 n_jobs = count, terms = p1, coeff = p2, max_d (in the place of b_slot), max_elems, src = A, dst = C): the MPO step of
 *                 a factored operator whose MPO blocks are small matrices.  Not counted as GEMM time.
 *         kind 6: {6, 0, jobs, rows, terms, n_jobs, a_slot, 0, c_slot, max_cols, 0, 0} -- tpa_mpo_entry_apply_batch(dtype, jobs = p0,
 *                 n_jobs = count, rows = p1, terms = p2, max_job_cols = max_elems, src = A, dst = C): the MPO step of a factored operator
 *                 whose MPO index sits inside the blocks (wide MPO bond blocks, wide sectors).  Not counted as GEMM time.
 *         kind 7: {7, cfg, tasks, links, tiles, n_tiles, a_slot, b_slot, c_slot, a2_slot, alphas, 0} -- kind 0 through
 *                 tpa_gemm_chain_ex: A2 = the slot in field 9, alphas_dev = the device pointer in field 10.  Counted as GEMM time.
 *         slots: >= 0 -> bufs[slot] (HOST array of n_bufs device pointers: fixed operands and temporaries), -1 -> the input
 *         vector v_k, -2 -> the output vector w of this matvec.  (p0..p2 are device pointers stored as integers.)
 *   krylov_dev : (N_max + 1) * n elements; on return vectors 0 .. N-1 are the orthonormal Krylov basis (v_0 = psi0 / |psi0|).
 *   scalars_dev: 2 * (N_max + 2) doubles.  Per step k:  w = matvec(v_k) [+ E_shift v_k];  tpa_lanczos_step;  (alpha_k, beta_k^2)
 *   are posted to mapped host memory and `cb(k, alpha_k, beta_k^2, user)` is called ONE STEP LATE, while step k + 1 already runs
 *   on the device; a nonzero return stops the iteration after step k (N = k + 1; the step in flight is discarded).
 *   info (HOST double[4]) = {N, number of matvecs launched, summed GEMM time in ms if time_gemms else 0, |psi0|};
 *   N = 0 <=> |psi0| < cutoff (nothing useful was computed).                                                          */
typedef int (*tpa_lanczos_callback)(int step, double alpha, double beta_sq, void *user);
/* Collective hook of op kind 3 (per host thread; NULL = none): returns 0 on success. */
typedef int (*tpa_collective_callback)(int which, void *user);
int tpa_lanczos_set_collective(tpa_collective_callback cb, void *user);
int tpa_lanczos_run(int dtype, int64_t n, const int64_t *ops, int n_ops, void *const *bufs, int n_bufs,
                    void *krylov_dev, const void *psi0_dev, int N_max, double cutoff, int has_shift, double E_shift,
                    double *scalars_dev, double *scratch_dev, tpa_lanczos_callback cb, void *user,
                    int time_gemms, double *info, void *stream);
/* tpa_lanczos_run with `flags` (tpa_lanczos_run is this call with flags = 0, project_work_dev = NULL).
 * flags bit 0: full re-orthogonalisation (`reortho` of the reference, krylov_based.py:667-669).  Step k >= 1 becomes
 *   alpha = Re <w|v_k> ;  w -= alpha v_k ;  tpa_project_out of w against v_0 .. v_{k-1} in place (basis = krylov_dev, stride = n; the
 *   beta v_{k-1} term of the recurrence is part of that projection) ;  bsq = |w|^2 out of the same pass ;  w /= sqrt(bsq);
 *   step 0 is the plain step.  Needs N_max <= TPA_PROJECT_MAX and project_work_dev: 2 TPA_PROJECT_MAX + 2 + TPA_PROJECT_WORK doubles
 *   (only read and written with bit 0).  Other bits: TPA_E_BADARG. */
int tpa_lanczos_run_ex(int dtype, int64_t n, const int64_t *ops, int n_ops, void *const *bufs, int n_bufs,
                       void *krylov_dev, const void *psi0_dev, int N_max, double cutoff, int has_shift, double E_shift,
                       double *scalars_dev, double *scratch_dev, tpa_lanczos_callback cb, void *user,
                       int time_gemms, double *info, int flags, double *project_work_dev, void *stream);
/* out = sum_{k < N} coeff[k] v_k over the Krylov basis of tpa_lanczos_run (N <= 64, real coefficients: the eigenvector of
 * the tridiagonal matrix), norm_host[0] = |out| (blocking): `_calc_result_full`, krylov_based.py:223-236, in one pass. */
int tpa_krylov_combine(int dtype, int64_t n, const void *krylov_dev, int N, const double *coeff, void *out_dev,
                       double *red_out_dev, double *scratch_dev, double *norm_host, void *stream);
/* The same with COMPLEX coefficients (coeff: N pairs re, im on the host; exp(delta h) e_0 of `LanczosEvolution.run`):
 * out = scale * sum_{k < N} c_k v_k.  The basis is F64 or C128 (`basis_dtype`), `out_dev` is ALWAYS C128 (n elements): a real
 * basis with complex c_k is the first time step of a real state.  norm_host[0] = |sum_k c_k v_k| BEFORE `scale` (blocking); the
 * caller normalises with tpa_scal.  red_out_dev: 2 doubles, scratch_dev: TPA_RED_SCRATCH doubles. */
int tpa_krylov_combine_z(int basis_dtype, int64_t n, const void *krylov_dev, int N, const double *coeff, double scale,
                         void *out_dev, double *red_out_dev, double *scratch_dev, double *norm_host, void *stream);

/* ---- K8/K9/K10: data movement ---------------------------------------------------------
 * Generic strided N-d block copy (N <= TPA_COPY_MAXDIM), batched.  Replaces
 * _sliced_strided_copy/_sliced_copy (_npc_helper.pyx:368, :754; combine/split legs :1112-1123,
 * :1235-1240) and the per-block PyArray_Transpose+copy of itranspose (:853).
 * jobs : int64[n_jobs][4 + 3*TPA_COPY_MAXDIM] =
 *        {dst_off, src_off, ndim, flags, shape[MAXDIM], dst_stride[MAXDIM], src_stride[MAXDIM]}
 *        flags bit0: conjugate while copying (complex only).
 * The last dim is the fastest-varying loop index; strides in elements.
 * All batched entry points of this section take one job per blockIdx.y: n_jobs <= 0 returns 0 without a launch, n_jobs > 65535
 * returns TPA_E_BADARG before anything is launched.  `max_job_elems` is the largest element count of a job; it sizes the grid, which
 * is capped at 512 workgroups per job (larger jobs loop).  Jobs with a zero extent are legal and do nothing.
 */
#define TPA_COPY_MAXDIM 6
int tpa_copy_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int64_t max_job_elems,
                   const void *src_base, void *dst_base, void *stream);
/* dst slab (rows x cols, row stride dst_ld) = sum_t alpha_t * src_t slab (row stride src_ld_t), batched.
 * Fuses tensordot(LP, W) + combine_legs of MPOEnvironment._contract_LHeff / _contract_RHeff (networks/mpo.py:3107,
 * :3118; TwoSiteH.combine_Heff, mps_common.py:1350) when every charge block of the MPO tensor W is a single number:
 * each (w', p, p*) slab of LHeff is a linear combination of the LP[:, w, :] blocks with the W entries as coefficients.
 * jobs : int64[n_jobs][8] = {dst_off, rows, cols, dst_ld, term_begin, term_count, 0, 0}
 * terms: int64[n_terms][4] = {src_off, src_ld, alpha_re, alpha_im}  (alpha_* are the IEEE-754 bit patterns of doubles) */
int tpa_lincomb_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *terms_dev, int64_t max_job_elems,
                      const void *src_base, void *dst_base, void *stream);
/* dst slab (pre, d_out, post) = sum_t M_t applied on the middle index of src_t slab (pre, d_in_t, post), batched: the MPO step of
 * the factored effective Hamiltonians for MPO tensors whose bond legs have 1-wide blocks while a physical charge sector holds
 * several states -- the W0 / W1 tensordots of TwoSiteH.matvec (mps_common.py:1321-1348) and the W0 tensordot of OneSiteH.matvec
 * (:1146-1149) as ONE pass; tpa_lincomb_batch is the d = 1 case with the coefficient stored in the term.
 * jobs : int64[n_jobs][8]  = {dst_off, pre, d_out, post, term_begin, term_count, 0, 0}
 * terms: int64[n_terms][4] = {src_off, d_in, coeff_off, 0}
 *   dst[dst_off + (i*d_out + o)*post + j] = sum_t sum_c coeff[coeff_off_t + o*d_in_t + c] * src[src_off_t + (i*d_in_t + c)*post + j]
 *                                           for i < pre, o < d_out, j < post
 * Offsets in elements of dtype; coeff_dev holds elements of dtype, row-major d_out x d_in_t per term.  max_d >= every d_in / d_out of
 * the call (it selects the register budget of the kernel; rows o >= max_d of a job that breaks this are not written); max_job_elems =
 * max pre * d_out * post sizes the grid, capped at 512 workgroups per job (larger jobs loop).  One job per blockIdx.y like the other
 * batched entry points of this section: n_jobs <= 0 returns 0 without a launch, n_jobs > 65535 returns TPA_E_BADARG; jobs with a zero
 * extent do nothing.  dtype and 1 <= max_d <= TPA_MPO_APPLY_MAXD are checked first (TPA_E_BADARG also for n_jobs <= 0), all argument
 * errors before anything is launched.  A job with term_count = 0 writes zeros.  Every element of a destination slab is written
 * exactly once, nothing else is written; src and dst must not overlap.  Summation order: terms in table order, c ascending, one chain
 * of fused multiply-adds per component (real: sum_t d_in_t, complex: twice that) -- two identical calls give identical bits.
 * Traffic: itemsize (sum_terms pre d_in post + sum_jobs pre d_out post) bytes.  16-byte loads and stores where src_base and dst_base
 * are 16-byte aligned and, for F64, post, dst_off and every src_off of the job are even; 8-byte ones otherwise. */
#define TPA_MPO_APPLY_MAXD 16
int tpa_mpo_apply_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *terms_dev, const void *coeff_dev, int max_d,
                        int64_t max_job_elems, const void *src_base, void *dst_base, void *stream);
/* dst slab (pre, n_rows, post): row o = sum_t alpha_t * (one middle row of a src slab), batched, one job per destination slab: the MPO
 * step of the factored effective Hamiltonians entry by entry, for the MPO tensors tpa_lincomb_batch and tpa_mpo_apply_batch do not
 * serve -- MPO bond legs with blocks wider than 1 (sorted bond legs), physical sectors wider than TPA_MPO_APPLY_MAXD, no conserved
 * charge.  A single entry of W (two sites: of sum_w'' W0[w, w''] W1[w'', w']) takes one middle row c of a block (pre, M_in, post) of the
 * source to one middle row o of a block (pre, M_out, post) of the destination.
 * jobs : int64[n_jobs][8] = {dst_off, pre, n_rows, post, row_begin, dst_ld, 0, 0}     dst_ld = 0 means n_rows * post
 * rows : int64[..][2]     = {term_begin, term_count}                                  row o of a job: rows[row_begin + o], o < n_rows
 * terms: int64[..][4]     = {src_off, src_ld, alpha_re, alpha_im}                     the terms of tpa_lincomb_batch (bit patterns)
 *   dst[dst_off + i*dst_ld + o*post + j] = sum_t alpha_t * src[src_off_t + i*src_ld_t + j]      for i < pre, o < n_rows, j < post
 * Offsets and strides in elements of dtype; src_off already contains c * post.  dst_ld > n_rows * post lets several jobs share one
 * block (each a range of its rows).  max_job_cols = max pre * post over the jobs sizes the grid, capped at 512 workgroups per job
 * (larger jobs loop).  One job per blockIdx.y like the other batched entry points of this section: dtype is checked first, then
 * n_jobs <= 0 returns 0 without a launch and n_jobs > 65535 returns TPA_E_BADARG; all argument errors before anything is launched; jobs
 * with a zero extent do nothing.  Every element of a destination slab is written exactly once -- a row with term_count = 0 writes zeros
 * --, nothing else is written; src and dst must not overlap.  Summation order: the terms of a row in table order, one chain of fused
 * multiply-adds per component (real: term_count, complex: twice that) -- two identical calls give identical bits.
 * Traffic: itemsize (sum_terms pre post + sum_jobs pre n_rows post) bytes.  16-byte loads and stores where src_base and dst_base are
 * 16-byte aligned and, for F64, post, dst_off, dst_ld and every src_off and src_ld of the job are even; 8-byte ones otherwise. */
int tpa_mpo_entry_apply_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *rows_dev, const int64_t *terms_dev,
                              int64_t max_job_cols, const void *src_base, void *dst_base, void *stream);
/* tpa_mpo_entry_apply_batch with a destination offset per row and a second source: the fused matrix of the subspace expansion of
 * single-site DMRG in ONE pass.  It replaces the build of LHeff / RHeff, iscale_axis with the mixing weights, the tensordot over the
 * fused leg and combine_legs of SubspaceExpansion (reference mps_common.py:2140-2168, right move, and :2170-2199, left move): the
 * source is T1 = LP . theta (theta . RP), a job is one cell (row slice x column slice) of a charge block of the fused matrix
 * [(vL.p0), (wR.vR)] ([(vL.wL), (p0.vR)]), and the rows (p0', wR') of a cell lie one leading dimension apart for p0' and in other
 * column slices for wR' -- no (pre, n_rows, post) slab holds them.  The mixing weight is multiplied into alpha on the host.
 * jobs : int64[n_jobs][8] = {dst_off, pre, n_rows, post, row_begin, dst_ld, 0, 0}     dst_ld is used as it is (no default)
 * rows : int64[..][4]     = {term_begin, term_count, dst_row_off, src_sel}            row o of a job: rows[row_begin + o], o < n_rows
 * terms: int64[..][4]     = {src_off, src_ld, alpha_re, alpha_im}                     the terms of tpa_lincomb_batch (bit patterns)
 *   dst[dst_off + i*dst_ld + dst_row_off_o + j] = sum_t alpha_t * SRC_o[src_off_t + i*src_ld_t + j]     for i < pre, o < n_rows, j < post
 *   SRC_o = src_base if src_sel_o == 0 else src2_base    (the stacked form, IdL / IdR = None: the rows of theta itself read src2)
 * Offsets and strides in elements of dtype.  max_job_cols = max pre * post over the jobs sizes the grid, capped at 512 workgroups per
 * job (larger jobs loop).  One job per blockIdx.y like the other batched entry points of this section: dtype is checked first, then
 * n_jobs <= 0 returns 0 without a launch and n_jobs > 65535 returns TPA_E_BADARG; all argument errors before anything is launched; jobs
 * with a zero extent do nothing.  Exactly the listed elements are written, each once -- the caller guarantees that the rows of a launch
 * do not overlap; a row with term_count = 0 writes zeros --, nothing else is written; src, src2 and dst must not overlap; src2_base is
 * read only by rows that select it (it may be NULL when none does).  Summation order: the terms of a row in table order, one chain of
 * fused multiply-adds per component (real: term_count, complex: twice that) -- two identical calls give identical bits.  A thread owns
 * one column item (i, j) of its job and walks the job's rows with one accumulator; row and term tables go through uniform loads.
 * Traffic: itemsize (sum_terms pre post + sum_rows pre post) bytes.  16-byte loads and stores where src_base, src2_base and dst_base
 * are 16-byte aligned and, for F64, post, dst_off, dst_ld and every dst_row_off, src_off and src_ld of the job are even (decided per
 * job); 8-byte ones otherwise. */
int tpa_mpo_expand_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *rows_dev, const int64_t *terms_dev,
                         int64_t max_job_cols, const void *src_base, const void *src2_base, void *dst_base, void *stream);
/* A cell of a fused [(vL.p), (wR.vR)] matrix as one small dense product: the rows of a job = coeff (n_rows x n_src) times the job's
 * DISTINCT source rows.  It serves the zip-up application of an MPO to an MPS (reference mpo.py:1733-1757: tensordot(B, W),
 * combine_legs) for MPO tensors that are dense in the bond index (U_I / U_II), where the N rows of a cell draw on the same K source
 * rows: tpa_mpo_expand_batch loads N K source items per column item of the cell, this entry point K (and stores N).
 * jobs : int64[n_jobs][10] = {dst_off, pre, n_rows, post, dst_ld, row_begin, src_begin, n_src, coeff_off, 0}
 * rows : int64[..][2]      = {dst_row_off, 0}                  row o of a job: rows[row_begin + o]
 * srcs : int64[..][2]      = {src_off, src_ld}                 source k of a job: srcs[src_begin + k]
 * coeff: elements of dtype; coefficient of (row o, source k) of a job at coeff[coeff_off + k*n_rows + o]
 *   dst[dst_off + i*dst_ld + dst_row_off_o + j] = sum_{k < n_src} coeff(o,k) * src[src_off_k + i*src_ld_k + j]
 *   for i < pre, o < n_rows, j < post
 * Offsets and strides in elements of dtype.  1 <= max_rows <= TPA_MPO_CELL_MAXROWS and max_rows >= n_rows of every job (it selects the
 * number of accumulators a thread keeps: 8, 16 or 32); rows o >= max_rows of a job that breaks this are not written (the max_d
 * convention of tpa_mpo_apply_batch).  Several jobs may share one source list and differ in coeff_off (a cell with more than
 * TPA_MPO_CELL_MAXROWS rows is split that way).  max_job_cols = max pre * post over the jobs sizes the grid, capped at 512 workgroups
 * per job (larger jobs loop).  One job per blockIdx.y like the other batched entry points of this section: dtype, then max_rows are
 * checked first, then n_jobs <= 0 returns 0 without a launch and n_jobs > 65535 returns TPA_E_BADARG; all argument errors before
 * anything is launched; jobs with a zero extent do nothing.  Exactly the listed elements are written, each once -- the caller
 * guarantees that the rows of a launch do not overlap; a job with n_src = 0 writes zeros --, nothing else is written; src and dst must
 * not overlap.  Summation order: k ascending, one chain of fused multiply-adds per component, zero coefficients included, the complex
 * pattern of tpa_mpo_expand_batch -- on finite data the result compares equal (==) to tpa_mpo_expand_batch fed the nonzero
 * coefficients in the same order, and two identical calls give identical bits.  A thread owns one column item (i, j) of its job,
 * loads every source item once and updates the accumulators of all rows; the coefficients go through uniform (scalar) loads.
 * Traffic: itemsize (sum_jobs pre post (n_src + n_rows)) bytes.  16-byte loads and stores where src_base and dst_base are 16-byte
 * aligned and, for F64, post, dst_off, dst_ld and every dst_row_off, src_off and src_ld of the job are even (decided per job); 8-byte
 * ones otherwise. */
#define TPA_MPO_CELL_MAXROWS 32
int tpa_mpo_cell_apply_batch(int dtype, const int64_t *jobs_dev, int n_jobs, const int64_t *rows_dev, const int64_t *srcs_dev,
                             const void *coeff_dev, int max_rows, int64_t max_job_cols, const void *src_base, void *dst_base,
                             void *stream);
/* x_b[i, j, l] *= s[s_off_b + j]  for each block b viewed as (pre, len, post).  Replaces
 * iscale_axis, np_conserved.py:2132-2140.  jobs: int64[n][6] = {x_off, pre, len, post, s_off, 0};
 * the scale vector s is real (F64) or of `dtype` when s_is_complex. */
int tpa_scale_axis_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int64_t max_job_elems,
                         void *x_base, const void *s_dev, int s_is_complex, void *stream);
int tpa_fill_zero(void *dst_dev, int64_t n_bytes, void *stream);
/* G_b <- strict lower triangle of G_b, diagonal (G_ii - 1) / 2, zeros above, for square blocks G_b (n x n row-major at g_off).
 * With G = T T^H the Gram matrix of row vectors sorted by descending singular value, T <- T - G T orthonormalises every vector
 * against the vectors before it (one ordered Gram-Schmidt step on the matrix cores, defect d -> O(d^2)): the post-processing of
 * the singular vectors below the absolute floor of the block SVD, where the reference gets LAPACK's orthonormal vectors
 * (np_conserved.py:4970 svd_flat).  jobs: int64[n][2] = {g_off, n}. */
int tpa_tri_lower_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int64_t max_job_elems, void *g_base, void *stream);
/* dst[b][i, j, l] = src[b][i, idx[idx_off + j], l] for blocks viewed as (pre, len, post): the np.compress
 * of iproject (np_conserved.py:1982).  jobs: int64[n][8] = {dst_off, src_off, pre, len_src, len_dst, post,
 * idx_off, 0}; idx_dev: int64 indices. */
int tpa_gather_axis_batch(int dtype, const int64_t *jobs_dev, int n_jobs, int64_t max_job_elems,
                          const int64_t *idx_dev, const void *src_base, void *dst_base, void *stream);
/* out[o_off + j] = sum_{i,l} |x[i, j, l]|^2 for blocks viewed as (pre, len, post): per-slice squared norms
 * (np.linalg.norm(block, axis) in _qr_theta_Y0, truncation.py:452).  jobs: int64[n][6] = {x_off, pre, len, post,
 * o_off, 0}; rows: int32[n_rows][2] = {job, j} (one wavefront each; n_rows padded to a multiple of 4 with job=-1). */
int tpa_axis_sqnorm_batch(int dtype, const int64_t *jobs_dev, const int32_t *rows_dev, int n_rows,
                          const void *x_base, double *out_dev, void *stream);
/* Flat dtype conversion / (complex) conjugation of an arena: astype (np_conserved.py:1865) and
 * iconj's complex_conj (np_conserved.py:2202-2235).  c128->f64 keeps the real part. */
int tpa_convert(int from_dtype, int to_dtype, int64_t n, const void *src_dev, void *dst_dev, int conj,
                void *stream);
/* Tile shape (rows, cols of C per workgroup) of GEMM configuration `cfg` for `dtype`. */
int tpa_gemm_tile_shape(int dtype, int cfg, int *bm, int *bn);
/* Tuning hook (also TPA_GEMM_VARIANT in the environment): bit 0 = the round-6 loop of the real kernel also for launches of <= 1024
 * tiles (default there: eight wavefronts per 64 x 64 tile on the round-4 loop; profiles/r06_gemm_v2.txt). */
int tpa_gemm_set_variant(int v);

/* ---- K5: batched block SVD, one-sided (Hestenes) Jacobi -- replaces svd_flat / LAPACK gesdd
 *      per charge block (np_conserved.py:4970-4980 via svd_robust.py:36-75) ---------------
 * jobs : int64[n_jobs][8] = {a_off, m, n, u_off, s_off, vh_off, flags, norm2_bits}  (HOST pointer)
 *   norm2_bits: 0, or the IEEE-754 bit pattern of a double that replaces |A_b|_F^2 as the scale of the numerical-rank
 *   decision and of the absolute floor (used for residual blocks E = A - P whose own norm is far below that of A).
 *   flags bit 0 (square blocks only): orthogonalise the rows of A instead of its columns (default 0).
 *   A_b is m x n row-major at a_off in a_base; on return
 *   U_b (m x k, row-major, k=min(m,n)) at u_off in u_base, S_b (k, descending) at s_off in s_dev
 *   (always real), VH_b (k x n, row-major) at vh_off in vh_base.  A is NOT overwritten.
 * work_dev: >= tpa_svd_worksize(...) bytes.  Synchronises the stream (sweep-convergence test).
 * min(m,n) >= 32 (complex: and max(m,n) <= 2048): the blocks are first reduced by a rank-revealing Householder QR with column
 *   pivoting (X P = Q [R;0], X = A or A^T); the Jacobi iteration then runs on the r x min(m,n) factor only
 *   (r = numerical rank: residual column norms <= 1e-15 ||A||_F).  Singular values below that threshold are
 *   returned as exact zeros with zero singular vectors (LAPACK returns rounding noise there).
 * tol: absolute floor rho of the stopping rule, |tol| <= 1 (0: the purely relative Hestenes criterion, every pair converged to a
 *   cosine of eps sqrt(L)).  tol > 0: pairs whose LARGER row is below rho |A|_F stop at |x.y| <= eps sqrt(L) |y| rho |A|_F (rounds
 *   1 - 5; exact after a SYMMETRIC re-orthonormalisation of the small vectors).  tol < 0 (round 6, what the engines pass): the floor
 *   |tol| acts on the SMALLER row, |x.y| <= eps sqrt(L) |x| max(|y|, rho |A|_F) with |x| >= |y| -- the same absolute accuracy of
 *   U S VH and of S provided the caller orthonormalises the normalised rows in DESCENDING order of S (every vector against the
 *   ones before it: tpa_tri_lower_batch), far fewer rotations on spectra graded down to rounding level.
 * Returns TPA_E_NOCONV if max_sweeps is exhausted, TPA_E_NAN if the input holds NaN/Inf.
 */
int64_t tpa_svd_worksize(int dtype, const int64_t *jobs_host, int n_jobs);
int tpa_svd_batch(int dtype, const int64_t *jobs_host, int n_jobs, const void *a_base,
                  void *u_base, double *s_dev, void *vh_base, void *work_dev, int64_t work_bytes,
                  int max_sweeps, double tol, int *sweeps_done, void *stream);

/* ---- the per-bond SVD section of a sweep as ONE call (round 6) -- replaces, for a two-site wave function whose bond has been
 *      decomposed before, the per-block LAPACK calls of npc.svd (np_conserved.py:3676-3760, worker :4950-5002) inside svd_theta
 *      (truncation.py:258): the WARM route (project on the singular vectors Bq of the bond's previous visit, residual test, one-sided
 *      Jacobi on W = Bq X^H without any QR, accumulated basis, results in the layout of tpa_svd_batch, singular values on the host,
 *      ordered clean-up of the vectors below the absolute floor).  All tables are built inside and uploaded in one copy per stage.
 * side   : 0 = 'R' (X = A: the basis spans the row space of theta; sweep moving right), 1 = 'L' (X = A^T).
 * blocks : HOST int64[n_blocks][8] = {a_off, m, n, u_off, s_off, v_off, b_off, b_k}: A_b (m x n row-major at a_off; the blocks lie back
 *          to back and fill a_numel elements), results U_b (m x kk) / S_b (kk) / VH_b (kk x n) at u_off / s_off / v_off (kk = min(m, n)),
 *          basis Bq_b (b_k x n (side 0) or b_k x m (side 1), row-major, orthonormal rows, 0 < b_k <= kk) at b_off in basis_arena.
 * u_arena / v_arena (u_numel / v_numel elements) are cleared here; s_host (HOST, sum of kk doubles) receives S (zero beyond b_k).
 * e_tol  : per block |X - (X Bq^H) Bq|_F <= e_tol |X|_F or the call returns 1 ("stale basis") with info[0] = the worst relative
 *          residual, info[1] = number of failing blocks, and the result arenas cleared -- the caller goes on with the sketch / cold route.
 * lowdin_basis: one first-order Loewdin step on the accumulated basis (every few warm generations of a bond).
 * clean_iterations, clean_floor: ordered re-orthonormalisation (tpa_tri_lower_batch) of the normalised Jacobi rows over the
 *          significant vectors when some lie below clean_floor |S_b|_2 (0 iterations: none) -- the counterpart of tol < 0 below.
 * alg_warm / alg_restore: tpa_svd_set_algorithm values for the Jacobi stage (bit 9: no pivoted QR) and afterwards.
 * max_sweeps, tol, sweeps_done: as for tpa_svd_batch.  info: HOST double[4].  f64 only.  Waits for the residual test and for the
 * singular values; the result copies and the clean-up may still be queued on the stream when it returns.
 * Returns 0 (done), 1 (stale), or a TPA_E_* code of the Jacobi stage. */
int tpa_svd_theta(int dtype, int side, const int64_t *blocks, int n_blocks, int64_t a_numel, const void *a_arena,
                  const void *basis_arena, void *u_arena, int64_t u_numel, void *v_arena, int64_t v_numel, double *s_host,
                  double e_tol, int lowdin_basis, int clean_iterations, double clean_floor, int alg_warm, int alg_restore,
                  int max_sweeps, double tol, int *sweeps_done, double *info, void *stream);
/* The warm-start bases of the bond's next visit out of a finished decomposition: rows [0, ksig_b) of VH_b -> basis_r (ksig x n,
 * back to back), columns [0, ksig_b) of U_b transposed -> basis_l (ksig x m).  blocks as above (m, n, u_off, v_off are read). */
int tpa_svd_theta_store(int dtype, const int64_t *blocks, const int64_t *ksig, int n_blocks, const void *u_arena, const void *v_arena,
                        void *basis_r, void *basis_l, void *stream);

/* Algorithm switch (test / benchmark hook): 0 (default) = pivoted-QR preconditioner + block Jacobi (16-row MFMA
 * Gram + in-LDS eigen-solve); bit 0 = one wavefront per row pair; bit 1 = two-kernel Jacobi rounds instead of the fused one; bit 2 = full local
 * sweep in every round; bits 4-7 = local sweeps; bit 9 (512) = no pivoted-QR preconditioner; bit 10 (1024) = NO predicted
 * convergence; bit 11 (2048) = no one-workgroup-per-pair round (real data, blocks with rank + columns <= 2048; the fused round with
 * column parts is used instead); bit 12 (4096) = no 32-row-block rounds (real data; the 8-row-block kernels run instead); bit 13 (8192) = no
 * look-ahead round (the host drains the stream after every sweep before it enqueues the next one).  Predicted convergence (default since round 2, validated on the MI355X on chi = 2048 blocks: same singular values
 * to 1.4e-15 sigma_max, same orthogonality, one to two sweeps fewer): a sweep in which no rotated pair had a scaled cosine
 * above 1e-7 ends the iteration without the verification sweep (quadratic convergence leaves cosines <= 1e-14).
 * Round 4 -- Gram-only sweeps (csrc/tpa_svd_b32.inc, real data; csrc/tpa_svd_b32c.inc, complex data -- there they are the only
 * 32-row-block path; calls whose largest block has >= 96 rows; default): a sweep starts
 * from ONE exact Gram matrix W W^T per block (grouped GEMM), its rounds rotate that matrix alone (solve per pair + 64^3 MFMA
 * updates of the Gram tiles and of the accumulated transform) and end with one product [W | G] <- Qtot [W | G]; bit 20
 * (1048576) = off (gram / solve / apply on the data in every round, the round-3 path; complex data: the 8-row-block rounds).
 * Bit 14 (16384): complex Gram-only rounds with the tiles the next solve does not read on a second stream (measured slower; off).
 * Bit 23 (8388608): two launches per Gram-only round (round-4 A/B switch; bit 22 selected the round-3 solve kernel, removed in round 5).
 * Round 5: the "big rotation" test of the predicted convergence judges a pair below the floor against its own stopping rule
 * (scale sqrt(max(alpha, beta)) rho |A|_F instead of rho^2 |A|_F^2: with the old scale such pairs never counted and the iteration
 * could end on cosines of O(0.1) among them).  (Bits 15 - 19 and 21 switched the round-4 end game by simultaneous rotations +
 * Newton-Schulz steps: measured slower over a whole sweep, never on by default, removed in round 5 with its counters.) */
int tpa_svd_set_algorithm(int pairwise);
/* Round 6 -- activity-driven rounds of the Gram-only sweeps (real data; bit 24 (16777216) of tpa_svd_set_algorithm = off): at the start
 * of a sweep a kernel tests, on the exact Gram matrix, which pairs of 32-row blocks contain a row pair that needs a rotation; the host
 * packs only those block pairs into perfect matchings (the rounds of that sweep) and ends the iteration after a sweep that started
 * without "big" pairs.  tpa_svd_dyn_stats: out = {rounds launched, rounds the round-robin schedule would have run, sweeps}. */
int tpa_svd_dyn_stats(int64_t *out, int reset);
/* Diagnostic ring of the most recent tpa_svd_batch calls (host): rows of out = {min(m, n) of the largest block, its max(m, n),
 * blocks, sweeps, pivoted QR used, algorithm switches, wall microseconds inside the call, return code}; returns the rows written. */
int64_t tpa_svd_call_log(int64_t *out, int64_t max_rows, int reset);
/* Rank cap of the pivoted-QR stage (0 = none, default): with cap > 0 tpa_svd_batch returns TPA_E_RANKCAP as soon as some
 * block turns out to have numerical rank above ~cap (checked every 64 columns).  Used by the warm-started SVD for the residual
 * blocks E = A - P, which are decomposed only if they are of low rank (tenpy_amd/linalg/_svd_warm.py). */
int tpa_svd_set_rank_cap(int cap);

/* ---- K6: batched Householder QR (np.linalg.qr per block, np_conserved.py:4190) ----------
 * jobs : int64[n_jobs][8] = {a_off, m, n, q_off, r_off, 0,0,0} (HOST); reduced mode:
 *   Q_b m x k row-major, R_b k x n row-major, k = min(m,n).  A not overwritten.
 *   a_off is a signed element offset from a_base: the blocks of SEVERAL arenas may be factorised in one call by taking the
 *   lowest arena address as a_base (np_conserved.qr_batched: the bonds of one half-step of the QR-based TEBD, reference
 *   algorithms/tebd.py:374-414 / truncation.py:611-640).
 * Pinned by tests/test_conformance_qr.py on every dispatch path:
 *   - Q_b and R_b are written COMPLETELY, the zeros below the diagonal of R_b (+0.0) included: q_base / r_base may be
 *     uninitialised memory (every caller passes such).  Nothing outside of the Q_b / R_b of the jobs is written, a_base is only read.
 *   - LAPACK's reflector convention (d/zlarfg): R_jj = -sign(Re x_0) |x| for the column x that is reduced, the diagonal of R_b is
 *     real (Im R_jj == 0 exactly), and H_j = I (R_jj = x_0, either sign) where x is already reduced (nothing below x_0, x_0 real).
 *     Q_b has orthonormal columns also for rank-deficient blocks (zero or equal columns).
 *   - the same call on the same data gives bit-identical Q_b and R_b.
 *   - n_jobs <= 0: returns 0, nothing is touched.  A job with m <= 0 or n <= 0: TPA_E_BADARG.  m <= 19200 (f64) / 9600 (c128) for
 *     every job, otherwise TPA_E_BADARG: blocks beyond the row limit of the blocked path go to the one-workgroup kernel, which
 *     holds a reflector in 150 KB of LDS.  An argument error is found before anything is launched: the outputs are untouched. */
int tpa_qr_batch(int dtype, const int64_t *jobs_host, int n_jobs, const void *a_base, void *q_base,
                 void *r_base, void *stream);
/* Test hook: bit 0 = always use the one-workgroup Householder kernel (default: blocked compact-WY QR on the matrix
 * cores when min(m,n) >= 32 and m <= 8192 (real) / 2048 (complex)); bit 1 = two launches per 8-column panel (factorisation, then
 * trailing update: rounds 2-4) also where the default is ONE launch per panel (round 5, csrc/tpa_qr_la.inc: real data, every block
 * tall with <= 2048 rows -- workgroup 0 of a block brings panel k + 1 up to date and factorises it while the other workgroups apply
 * panel k behind it).  Since round 5 tpa_qr_batch also orthogonalises the sketch Y = X Omega^H of the warm-started block SVD
 * (linalg/_svd_warm.py::svd_blocks_sketch). */
int tpa_qr_set_algorithm(int v);

/* ---- K7: batched Hermitian eigendecomposition (np.linalg.eigh per block, np_conserved.py:5059-5061; `_eig_worker` :5041)
 * jobs : int64[n_jobs][8] = {a_off, n, w_off, v_off, 0,0,0,0} (HOST);  A_b n x n row-major, eigenvalues at w_off in w_dev,
 *   eigenvectors as COLUMNS of V_b (n x n row-major at v_off in v_base).  The three offsets are independent of each other.
 * Route, chosen PER CALL: if the largest block of the call, padded to an even number of rows, has >= 96 rows, ALL blocks of the call
 * (1-row blocks included) run the TWO-SIDED block Jacobi on A_b + mu (mu = 2 |A_b|_F) itself -- 32-row blocks, per round one cyclic
 * Jacobi solve of every 64 x 64 diagonal pair block and the two-sided MFMA update S[P, P'] <- Q_P S[P, P'] Q_P'^H,
 * Qtot[P, :] <- Q_P Qtot[P, :]; no GEMM over the data, no squared spectrum; it stops when no |S_ij| > 2^-52 sqrt(n) sqrt(S_ii S_jj)
 * is left.  Otherwise (and with tpa_eigh_set_direct(0), and for real data when the activity-driven rounds are switched off, bit 24 of
 * tpa_svd_set_algorithm): the one-sided iteration on the rows of A_b + mu.  All blocks of the call share the launches: callers
 * batch independent matrices (np_conserved.eigh_batched: the bond matrices of a TEBD half-step).
 * Pinned by tests/test_conformance_eigh.py on every route (two-sided, one-sided below 96 rows, one-sided on the Gram tables):
 *   - only the LOWER triangle of A_b is read (UPLO = 'L'), and of its diagonal only the real part: what stands above the diagonal
 *     (NaN, Inf, any finite data) and in Im A_ii has no influence on the result, mu = 2 |A_b|_F of the matrix so defined included.
 *   - W_b and V_b are written COMPLETELY (w_dev / v_base may be uninitialised memory), nothing outside of them is written, a_base is
 *     only read.
 *   - the eigenvalues ascend exactly (w[i + 1] >= w[i]).  Accuracy, in units u = eps sqrt(n) |A_b|_F (eps = 2^-53, f = 4 for complex
 *     data, |A_b|_F of the matrix defined by the lower triangle).  Every route iterates on A_b + mu, a matrix of norm up to
 *     (1 + 2 sqrt(n)) |A_b|_F with its spectrum in [|A_b|_F, 3 |A_b|_F]: the absolute accuracy is that of LAPACK's class ON THE SHIFTED
 *     MATRIX plus what the stopping rule leaves, NOT eps sqrt(n) |A_b|_F (rounds 1 - 6 said so; measured: 30 - 300 u at n = 64 ... 161
 *     where LAPACK reaches 1 - 2 u):  |w_i - lambda_i| <= (6 n + 16 f (1 + 2 sqrt(n))) u,  |A_b v_i - w_i v_i|_2 <=
 *     (6 sqrt(n) + 16 f (1 + 2 sqrt(n))) u per vector.  Column norms of V_b^H V_b - I <= 64 f eps sqrt(n) (LAPACK's class, 8 times what
 *     LAPACK itself reaches).  A diagonal block comes out exactly: w the sorted diagonal, V_b a signed permutation matrix of exact
 *     0 / +-1.  The iteration runs on the data scaled by a power of two (1 <= 2^-k mu < 2): |A_b|_F from 1e-150 to 1e+150 is fine.
 *   - the same call on the same data gives bit-identical W and V.
 *   - n_jobs <= 0: returns 0, nothing is touched.  dtype other than TPA_F64 / TPA_C128, a job with n <= 0, work_bytes <
 *     tpa_eigh_worksize: TPA_E_BADARG, found before anything is launched.  tpa_eigh_worksize does not depend on the test hooks and is
 *     > 0 for n_jobs = 0.
 *   - NaN / Inf in the triangle that is read (or |A_b|_F^2 beyond the range of a double): TPA_E_NAN (-> ValueError, like K5), decided by
 *     the norm before the iteration starts; max_sweeps exhausted: TPA_E_NOCONV.  In both cases W and V are untouched.
 * work_dev >= tpa_eigh_worksize bytes.  Synchronises the stream. */
int64_t tpa_eigh_worksize(int dtype, const int64_t *jobs_host, int n_jobs);
int tpa_eigh_batch(int dtype, const int64_t *jobs_host, int n_jobs, const void *a_base,
                   double *w_dev, void *v_base, void *work_dev, int64_t work_bytes, int max_sweeps,
                   double tol, int *sweeps_done, void *stream);
/* Test hook: 0 = tpa_eigh_batch always takes the shift + one-sided route (rounds 1 - 5), 1 = default. */
int tpa_eigh_set_direct(int on);
/* Test hook (read-only): 1 if the last tpa_eigh_batch on this host thread ran the direct two-sided iteration, 0 if it ran the
 * one-sided route (or returned before the iteration). */
int tpa_eigh_last_direct(void);
/* Eigenpairs of Hermitian blocks out of their SVDs A_b = U_b S_b VH_b (tpa_svd_batch), WITH the check that this is legitimate: where |lambda|
 * is not shared by a positive and a negative eigenvalue, v_i = d_i u_i (d_i = +/-1), lambda_i = d_i S_i and u_i is the eigenvector.
 * np_conserved.eigh_batched takes this route for real data (the graded, rank-deficient density matrices of the mixer, mps_common.py:1972-2079:
 * ~7 Jacobi sweeps on the rank-r factor instead of 35 - 40 on the matrix) and falls back to tpa_eigh_batch if err is not at rounding level.
 * jobs : int64[n_jobs][8] = {u_off, n, s_off, vh_off, lam_off, 0,0,0} (HOST);  U_b n x n row-major (vectors = columns u_i), VH_b n x n
 * row-major (rows = v_i^H); all four offsets are independent.  Jobs of different n share the call.
 * Pinned by tests/test_conformance_eigh.py:
 *   - d_i = -1 if Re u_i^H v_i < 0, else +1 (a zero or NaN product gives +1);  lam_dev[lam_off + i] = d_i S_i EXACTLY (order of S:
 *     descending |lambda|); nothing else of lam_dev is written.
 *   - err_dev[job] = max_i S_i |v_i - d_i u_i|_2 (= max_i |A u_i - lambda_i u_i|), >= 0.  err_dev[0 .. n_jobs) is CLEARED by the call
 *     (whatever it held: the maximum is taken on bit patterns, which needs the +0.0 start); v_i = d_i u_i bit for bit gives exactly
 *     0.0, vectors with S_i = 0 contribute 0.  A NaN in u_i, v_i or S_i makes err_dev[job] >= 1e300 (never a value that passes a
 *     gate), other jobs are unaffected.
 *   - the same call on the same data gives bit-identical lam and err.
 *   - n_jobs <= 0: returns 0, nothing is touched.  A bad dtype or a job with n <= 0: TPA_E_BADARG, nothing is launched.
 * Asynchronous on `stream`. */
int tpa_eigh_from_svd(int dtype, const int64_t *jobs_host, int n_jobs, const void *u_base, const double *s_dev,
                      const void *vh_base, double *lam_dev, double *err_dev, void *stream);

/* ---- host planner: integer bookkeeping of _tensordot_worker (_npc_helper.pyx:1498-1786) ---
 * Inputs describe operand a with its contracted legs LAST and b with its contracted legs FIRST
 * (i.e. after _tensordot_transpose_axes, :1260-1295), block lists in any order.
 *   a_qdata : int64[na][ra]  qindices,  a_keep = ra - ncontr ;  likewise b.
 *   *_block_size: for each leg, `nblk` block sizes are looked up through leg_sizes/leg_ptr:
 *       size of qindex q on leg L of a = a_leg_sizes[a_leg_ptr[L] + q].
 * Outputs (caller-allocated, capacities given; counts returned through n_*):
 *   res_qdata   : int64[n_res][a_keep + b_keep]   lex-sorted like the reference (:1777)
 *   res_a_first, res_b_first: representative a / b block of each result block
 *   gemm        : int64[n_gemm][3] = {res_index, a_block, b_block}  ordered by (res_index, level)
 * Returns 0, or TPA_E_BADARG if a capacity is too small (n_* then hold the needed sizes).
 */
int tpa_plan_tensordot(const int64_t *a_qdata, int64_t na, int ra, const int64_t *b_qdata,
                       int64_t nb, int rb, int ncontr, const int64_t *contr_nblocks,
                       int64_t *res_qdata, int64_t *res_a_first, int64_t *res_b_first,
                       int64_t cap_res, int64_t *n_res, int64_t *gemm, int64_t cap_gemm,
                       int64_t *n_gemm);

#ifdef __cplusplus
}
#endif
#endif
