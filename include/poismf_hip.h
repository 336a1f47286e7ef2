/*
 * poismf_hip.h -- C-ABI of the MI355X (gfx950) implementation of poismf's alternating factor-update
 * hot path.  Two shared libraries export exactly these symbols, as the reference builds its core
 * twice (ref: setup.py:225-243, src/poismf.h:91-109):
 *
 *     libpoismf_hip_d.so   real_t = double
 *     libpoismf_hip_f.so   real_t = float      (compile this header with -DUSE_FLOAT)
 *     libpoismf_hip_r.so   real_t = double, sparse_ix = int: the reference's R ABI (compile with -D_FOR_R,
 *                          ref: src/poismf.h:75-89; same row kernels as libpoismf_hip_d.so)
 *
 * sparse_ix is size_t otherwise (the reference's C/Python ABI, ref: src/poismf.h:76).  No torch / HIP types
 * appear in any signature: pointers and sizes only.  All "ref:" citations are relative to the
 * reference tree (david-cortes/poismf).
 *
 * There is NO CPU fallback: every entry point fails (non-zero return) if no HIP device is usable.
 */
#ifndef POISMF_HIP_H
#define POISMF_HIP_H

#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ref: src/poismf.h:75-109.  -D_FOR_R selects the R ABI: int indices, double only (libpoismf_hip_r.so). */
#ifdef _FOR_R
  #undef USE_FLOAT
#endif
#ifndef real_t
  #ifdef USE_FLOAT
    #define real_t float
  #else
    #define real_t double
  #endif
#endif
#ifndef sparse_ix
  #ifdef _FOR_R
    #define sparse_ix int
  #else
    #define sparse_ix size_t
  #endif
#endif
#if defined(__GNUC__) || defined(__clang__)
  #define POISMF_HIP_API __attribute__((visibility("default")))
#else
  #define POISMF_HIP_API
#endif

/* ref: src/poismf.h:225  typedef enum Method {tncg = 1, cg = 2, pg = 3} Method; */
typedef enum poismf_hip_method { POISMF_TNCG = 1, POISMF_CG = 2, POISMF_PG = 3 } poismf_hip_method;

/* ---------------------------------------------------------------------------------------------
 * 1. Drop-in entry point.
 *
 * Replaces: run_poismf, ref: src/poismf.h:226-233 (prototype), src/poismf.c:435-632 (body).
 * Same name, same argument order (NOTE indptr before indices), same in-place A/B semantics, same
 * return codes: 0 ok, 1 out of memory (host or device; also printed to stderr as the reference
 * does, ref: src/poismf.c:501), 2 interrupted by SIGINT (ref: src/poismf.c:618-630).
 * `method` is the reference's enum passed as int (1 tncg, 2 cg, 3 pg).
 * `nthreads` is accepted and ignored (the row loop runs on the GPU).
 * A, B, X* are HOST pointers owned by the caller; A and B are overwritten with the result.
 * The device used is HIP device $POISMF_HIP_DEVICE (default 0).
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int run_poismf(
    real_t *A, real_t *Xr, sparse_ix *Xr_indptr, sparse_ix *Xr_indices,
    real_t *B, real_t *Xc, sparse_ix *Xc_indptr, sparse_ix *Xc_indices,
    const size_t dimA, const size_t dimB, const size_t k,
    const real_t l2_reg, const real_t l1_reg, const real_t w_mult, real_t step_size,
    const int method, const bool limit_step, const size_t numiter, const size_t maxupd,
    const bool early_stop, const bool reuse_prev,
    const bool handle_interrupt, const int nthreads);

/* ---------------------------------------------------------------------------------------------
 * 1b. Factors for new rows with B fixed.
 *
 * Replaces: factors_multiple, ref: src/poismf.h:270-280 (prototype), src/pred.c:66-199 (body); called by the
 * Python transform() through poismf_c_wrapper.pxi:147-199.  Same name, argument order and meaning: A [dimA x k]
 * is output only (host), B / Bsum (with l1 already added) / Amean come from the fitted model, Xr* is the CSR of
 * the new rows.  It is one half-sweep of the same row kernels with the column sums supplied by the caller.
 * Returns 0, or 1 when out of memory / no device.
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int factors_multiple(
    real_t *A, real_t *B, real_t *Bsum, real_t *Amean,
    real_t *Xr, sparse_ix *Xr_indptr, sparse_ix *Xr_indices,
    int k, size_t dimA,
    real_t l2_reg, real_t w_mult,
    real_t step_size, size_t niter, size_t maxupd,
    int method, bool limit_step, bool reuse_mean,
    int nthreads);

/* ---------------------------------------------------------------------------------------------
 * 1c. COO -> CSR + CSC on the device.
 *
 * Replaces: the SciPy conversions of PoisMF._process_data, ref: poismf/__init__.py:404-414 (coo.tocsr() and
 * coo.tocsc(): duplicate (i,j) entries summed, indices sorted within each row / column, then cast to real_t /
 * size_t).  There is no C function for this in the reference; the entry point takes what _process_data holds
 * (host triplets) and fills what run_poismf takes.  Output arrays are caller-allocated with capacity n
 * (values, indices) and dim + 1 (indptr); *nnz_out receives the number of distinct (i,j).  Requires n < 2^32.
 *
 * The summation rule.  The stored value of a cell is a function of that cell's own triplet values, in the order the
 * caller gave them, and of nothing else: with the cell's triplets t1, t2, ... in input order it is
 *     s = t1;  s = s + t2;  s = s + t3;  ...        every addition rounded in real_t
 * (what SciPy's csr_sum_duplicates does on a row once its duplicates are adjacent; d triplets cost d - 1 dependent
 * additions and |s - exact sum| <= (d - 1) u sum|t|, u = half an ulp of 1).  So the CSR and the CSC hold the same bits
 * for a cell, a row shard holds the unsharded rows' bits, a cell's bits do not depend on the other triplets of the
 * call or on their number, and repeated calls agree.  Every conversion in this library follows the rule: this entry
 * point, poismf_hip_session_create_coo (shards included), eval_llk and the duplicates inside an update (section 2b).
 * Where the values are small integers every order gives the same sum, and the results are SciPy's bit for bit; for
 * other values SciPy's own order of equal columns is not defined (tocsr() sorts a row by column with an unstable sort).
 *
 * Returns 0; 1 when out of memory / no device; 3 when a row index is >= dimA or a column index >= dimB (a negative
 * index of the R flavour included): checked before any device work, nothing is written.
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int poismf_hip_coo_to_csr_csc(
    const sparse_ix *row, const sparse_ix *col, const real_t *val, size_t n, size_t dimA, size_t dimB,
    real_t *csr_val, sparse_ix *csr_indices, sparse_ix *csr_indptr,
    real_t *csc_val, sparse_ix *csc_indices, sparse_ix *csc_indptr, size_t *nnz_out);

/* ---------------------------------------------------------------------------------------------
 * 1d. Serving-side helpers.
 *
 * Replaces: predict_multiple, ref: src/poismf.h:250-257 (prototype), src/pred.c:42-64;
 *           topN,             ref: src/poismf.h:240-247 (prototype), src/topN.c:112-284.
 * Same names, argument order and return codes (topN: 0 ok, 1 out of memory / no device, 2 invalid combination of
 * include / exclude / n_top as at ref src/topN.c:126-130).  Among equal scores topN returns ascending indices (the
 * reference leaves that order to qsort).  An item whose score is -inf (finite factors whose chain overflows) still comes
 * before every excluded item.  Host pointers in and out; the factors are copied to the device per call.
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API void predict_multiple(
    real_t *out, real_t *A, real_t *B, sparse_ix *ixA, sparse_ix *ixB, size_t n, int k, int nthreads);
POISMF_HIP_API int topN(
    real_t *a_vec, real_t *B, int k,
    sparse_ix *include_ix, size_t n_include,
    sparse_ix *exclude_ix, size_t n_exclude,
    sparse_ix *outp_ix, real_t *outp_score,
    size_t n_top, size_t n, int nthreads);

/* ---------------------------------------------------------------------------------------------
 * 1e. Poisson log-likelihood of fitted factors (the reference declares eval_llk, ref: src/poismf.h:258-269, and
 *     defines it nowhere -- SURVEY quirk Q12; this is the definition).
 *
 * For factors A [dimA x k], B [dimB x k] and cells (i, j, x) -- duplicate (i, j) summed first by the rule of section 1c, as for a fit --
 * with yhat_ij = sum_c A[i,c] B[j,c] (products and sums in double, in both precisions):
 *
 *     llk = sum_cells [ x log(yhat) - lgamma(x + 1) * full_llk ] - M
 *     M   = sum_cells yhat                                 include_missing = false
 *     M   = sum_c (sum_i A[i,c]) (sum_j B[j,c])             include_missing = true (every cell of the dimA x dimB
 *                                                           matrix, a missing cell counting as x = 0)
 *
 * A cell with x = 0 contributes only -yhat (no log is taken); yhat = 0 with x > 0 gives -inf; NaN factors give NaN.
 * The log is the row kernels' own (the one the solvers take).  This is a likelihood, not the solvers' objective: the
 * l1 / l2 terms and w_mult play no part.  The result is deterministic (fp64 partials over fixed ranges of nonzeros,
 * summed in a fixed order) and does not depend on the device's size.
 *
 * eval_llk: same name and arguments as the reference's declaration.  Host arrays; the triplets are converted to a CSR
 * on the device as in section 1c (requires nnz < 2^32, dimA and dimB < 2^31, 1 <= k <= 512).  `nthreads` is accepted and
 * ignored.  On an invalid index or argument, or a device error, it prints to stderr and returns NaN.
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API long double eval_llk(
    real_t *A, real_t *B, sparse_ix ixA[], sparse_ix ixB[], real_t *X,
    size_t nnz, int k, bool full_llk, bool include_missing,
    size_t dimA, size_t dimB, int nthreads);

/* ---------------------------------------------------------------------------------------------
 * 1f. Batched top-N: the best items of many users in one fused pass (no counterpart in the reference, whose topN serves
 *     one user per call, ref: src/topN.c:112-284).
 *
 * For a batch of users u_0 .. u_{m-1} (any order, repeats allowed), n_top, and per user an exclusion set E(u):
 *
 *   score(u, j)  the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t -- bit for bit what
 *                predict_multiple / poismf_hip_session_predict return.  It is NOT the summation order of topN /
 *                poismf_hip_session_topn (sixteen strided partial chains and a butterfly): the last bit of a batched score
 *                may differ from theirs.  Factors are assumed finite; the result for a user with a NaN score is unspecified.
 *                Everything else a finite chain can give is a score like any other, here and in sections 1g - 1n: negative
 *                scores, exact zeros in any number, subnormal operands, products and sums (nothing is flushed: the bits are
 *                predict_multiple's, measured on the MI355X for the f32-MFMA tile and the scalar chains alike), and the +inf or
 *                -inf of a chain that overflows.  An infinite score takes its place in the total order: +inf items first,
 *                -inf items last, each by ascending index, and a real item at -inf comes before every empty entry of a padded
 *                row.  (Sections 1o and 1p multiply a score and keep their own clause on denormal products.)
 *   answer(u)    the first n_top of {0..dimB-1} \ E(u) under the total order "score descending, then item index ascending".
 *                It is a function of (A[u], B, E(u), n_top) alone: not of the other users in the batch, their order, or how
 *                the library tiles users and items.
 *   E(u)         the union of (a) with exclude_seen (session only): the items of row u of the session's resident CSR -- nothing
 *                is uploaded; rows are binary-searched only when a check on the device (once per session) found every resident
 *                row strictly ascending, as the COO conversion leaves them; rows in the caller's own order are scanned -- and
 *                (b) an optional CSR-shaped list for the batch: excl_indptr [m + 1], excl_indices, host arrays, row i belonging
 *                to u_i, indices strictly ascending within a row.  excl_indptr = NULL: no list.
 *   output       out_ix [m x n_top] (row-major) and, unless NULL, out_score [m x n_top]; host arrays.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, when: a user index
 * >= dimA; an item index >= dimB; an exclusion row not strictly ascending; n_top == 0; n_top > dimB - |E(u)| for some user;
 * n_top > POISMF_HIP_TOPN_BATCH_MAX_N_TOP; k outside what a session supports (1..512 float, 1..256 double); exclude_seen on a
 * session whose rows of A (rowA_begin..rowA_end) do not contain every requested user; one exclusion row longer than
 * POISMF_HIP_TOPN_BATCH_BUDGET_MB / 8 Mi entries.  n_users == 0 is not an error (returns 0).  With exclude_seen the sizes of the
 * resident rows are known on the device only: the row pointers are fetched once per session, and a user whose two lists
 * together could leave fewer than n_top items has its resident row fetched and the union counted, before anything is written.
 *
 * Memory: the users x items scores are never materialised.  The batch is cut into chunks of users inside the call, and ONE
 * scratch allocation per call (session: kept and reused) of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB holds a chunk's user list,
 * exclusion lists, partial results and results, for any n_users; poismf_hip_topn_batch_scratch_bytes (testing aid, no HIP call)
 * is the size both entry points allocate.  poismf_hip_topn_batch's own copies of B and of A (all of A, or only the batch's
 * rows when n_users < dimA) come on top of that.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_BATCH_MAX_N_TOP 128   /* largest n_top of the batched entry points */
#define POISMF_HIP_TOPN_BATCH_BUDGET_MB 256   /* upper bound of their scratch allocation, MiB */
/* host factors, copied up once per call (what a fitted PoisMF holds); users' rows of A only if that is less */
POISMF_HIP_API int poismf_hip_topn_batch(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);
POISMF_HIP_API size_t poismf_hip_topn_batch_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1g. Batched exact ranks: where each held-out item of many users stands in the user's COMPLETE ranked list, in one fused pass
 *     (no counterpart in the reference, whose notebook gets ranking metrics from a CPU package that scores every user against
 *     every item on the host).  poismf_amd/metrics.py turns the ranks into P@K, AP@K, NDCG@K, Hit@K, RR@K and AUC.
 *
 * For a batch of users u_0 .. u_{m-1} (any order, repeats allowed), per user an exclusion set E(u) defined exactly as in
 * section 1f (exclude_seen on a session and / or the CSR-shaped host list excl_indptr / excl_indices), and per user a held-out
 * list T(u): CSR-shaped host arrays test_indptr [m + 1], test_indices, item indices strictly ascending within a row.  Only
 * indices: every listed cell is a positive.
 *
 *   score(u, j)  section 1f's score, bit for bit what predict_multiple / poismf_hip_session_predict return.
 *   C(u), N(u)   C(u) = {0..dimB-1} \ E(u), N(u) = |C(u)|.
 *   rank(u, t)   for t in T(u) and not in E(u): the number of j in C(u) that come before t under the total order of section 1f
 *                (score(u,j) > score(u,t), or equal and j < t): t's 0-based position in the user's complete ranked list.  The
 *                batched top-N with the same E(u) and n_top > rank lists t at index rank.  Other held-out items count like any
 *                other item.  A rank is a function of (A[u], B, E(u), t) alone: not of the other users, the other held-out
 *                items, the batch order, or how the library tiles users and items.  All counting is in integers.
 *   excluded     a cell whose item is in E(u) gets POISMF_HIP_RANK_EXCLUDED; it is not an error (train / test overlaps are
 *                common in real splits).
 *   output       out_rank: one unsigned int per entry of test_indices, in the caller's order; out_n_adm [m]: N(u) (with
 *                exclude_seen and a list together, |E(u)| is the size of the union).  Host arrays.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, when: a user index
 * >= dimA; an item index >= dimB; a test or exclusion row not strictly ascending; row pointers that decrease; k outside what a
 * session supports (1..512 float, 1..256 double); exclude_seen on a session whose rows of A do not contain every requested
 * user; one exclusion row longer than POISMF_HIP_RANK_BATCH_BUDGET_MB / 8 Mi entries; one held-out row longer than
 * POISMF_HIP_RANK_BATCH_MAX_ROW entries (a user's held-out scores are put in order on the device by counting, which is quadratic
 * in the row's length).  n_users == 0 is not an error (returns 0); a user with an empty T(u) is valid.  Factors are assumed finite.
 *
 * Memory: the users x items scores are never materialised.  The batch is cut into chunks of users inside the call, and ONE
 * scratch allocation per call (session: kept and reused) of at most POISMF_HIP_RANK_BATCH_BUDGET_MB MiB holds a chunk's users,
 * lists, thresholds, counts and results, for any n_users and any total number of held-out cells;
 * poismf_hip_rank_batch_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate.  poismf_hip_rank_batch's
 * own copies of B and of A (all of A, or only the batch's rows when n_users < dimA) come on top of that.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_RANK_EXCLUDED 0xffffffffu   /* out_rank of a held-out cell whose item is in E(u) */
#define POISMF_HIP_RANK_BATCH_BUDGET_MB 256    /* upper bound of the scratch allocation, MiB */
#define POISMF_HIP_RANK_BATCH_MAX_ROW 65536    /* most held-out items of one user */
POISMF_HIP_API int poismf_hip_rank_batch(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users,
        const sparse_ix *test_indptr, const sparse_ix *test_indices,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        unsigned int *out_rank, unsigned int *out_n_adm);
POISMF_HIP_API size_t poismf_hip_rank_batch_scratch_bytes(size_t n_users, size_t n_cells, size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1h. Batched top-N over per-user candidate lists: the best items of many users, each among a list of its own, in one fused
 *     pass (the batched form of the reference's topN(..., include_ix), ref: src/topN.c:112-284, which serves one user per call).
 *     Only the listed rows of B are read: the cost follows the lists' lengths, not dimB.
 *
 * For a batch of users u_0 .. u_{m-1} (any order, repeats allowed), n_top, and per user
 *
 *   I(u)         an include list: CSR-shaped host arrays incl_indptr [m + 1], incl_indices; row i belongs to u_i, indices are
 *                < dimB and strictly ascending within a row.  Rows may be empty.
 *   E(u)         an exclusion set exactly as in section 1f: exclude_seen on a session and / or the CSR-shaped host list
 *                excl_indptr / excl_indices (excl_indptr = NULL: no list).
 *   score(u, j)  section 1f's score,  s = +0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t: bit for bit what
 *                predict_multiple / poismf_hip_session_predict and the batched top-N of section 1f return.
 *   answer(u)    the first n_top of I(u) \ E(u) under section 1f's total order (score descending, then item index ascending).
 *                It is a function of (A[u], B, I(u), E(u), n_top) alone: not of the other users, the batch order, how a list
 *                is cut into slices or how the batch is cut into chunks.  Where |I(u) \ E(u)| >= n_top it therefore equals
 *                section 1f's answer for the exclusion set E(u) united with {0..dimB-1} \ I(u).
 *   short rows   are not an error: when only c < n_top items are admissible, entries c .. n_top-1 of the row are
 *                POISMF_HIP_TOPN_NONE in out_ix (all bits of sparse_ix set) and -inf in out_score.  With exclude_seen the
 *                admissible count is known on the device only, and candidate slates that lose items to "already seen" are
 *                the normal case: no per-user pre-check as in section 1f is made.
 *   output       out_ix [m x n_top] (row-major) and, unless NULL, out_score [m x n_top]; host arrays.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, when: a user index
 * >= dimA; an item index >= dimB; an include or exclusion row not strictly ascending, or row pointers that decrease;
 * incl_indptr == NULL; n_top == 0 or n_top > POISMF_HIP_TOPN_BATCH_MAX_N_TOP; k outside 1..512 float / 1..256 double;
 * exclude_seen for a user outside the session's rows of A; an exclusion row over section 1f's limit; an include row longer than
 * POISMF_HIP_TOPN_INCLUDE_MAX_ROW (the 32-bit indices a quarter of the scratch budget holds; a list near catalogue size belongs
 * on the dense path of section 1f with its complement).  n_users == 0 is not an error (returns 0).  Factors are assumed finite.
 *
 * Memory: ONE scratch allocation per call (session: the one the calls of sections 1f and 1g share) of at most
 * POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB, for any number of users and candidates; the batch is cut into chunks of users whose
 * lists fit.  poismf_hip_topn_include_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate for a
 * batch whose lists hold n_cells indices in all.  poismf_hip_topn_include_slice (testing aid, no HIP call) is the number of
 * candidates per slice the host plan gives a list of `len` candidates: one wave scores one slice, a fixed minimum grown only so
 * that no user has more slices than the merge step ranks at once.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_NONE (~(sparse_ix)0)             /* out_ix of an entry past a short row's last admissible item */
#define POISMF_HIP_TOPN_INCLUDE_MAX_ROW 16777216         /* longest include row: 2^24 */
POISMF_HIP_API int poismf_hip_topn_include(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *incl_indptr, const sparse_ix *incl_indices,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);
POISMF_HIP_API size_t poismf_hip_topn_include_scratch_bytes(size_t n_users, size_t n_cells, size_t n_top, size_t dimB, size_t k);
POISMF_HIP_API size_t poismf_hip_topn_include_slice(size_t len, size_t n_top);

/* ---------------------------------------------------------------------------------------------
 * 1i. Batched top-N over candidate lists SHARED between users: a few lists (the items in stock in a region, a category page,
 *     a campaign slate), each referred to by many users, in one fused pass.  Section 1h serves a list per user: the host reads
 *     every user's copy of its list and every user gathers its own rows of B.  Here the host reads each list once, and on the
 *     device 64 users that refer to one list share every row of B they gather (the f32-MFMA tile of section 1f).  Use 1h when
 *     the lists really differ from user to user -- a batch in which every user has a list of its own is valid here but
 *     degenerates to one user per tile, and the library does not re-route -- and this section when few lists serve many users.
 *
 * For a batch of users u_0 .. u_{m-1} (any order, repeats allowed), n_top, and
 *
 *   L_0..L_{G-1} a table of candidate lists: CSR-shaped host arrays list_indptr [G + 1], list_indices; indices are < dimB and
 *                strictly ascending within a row.  Rows may be empty.  A list no user refers to is valid and costs nothing on
 *                the device.
 *   list_of [m]  the list of user u_i, values < G.
 *   E(u)         an exclusion set exactly as in section 1f: exclude_seen on a session and / or the CSR-shaped host list
 *                excl_indptr / excl_indices with one row per entry of `users` (excl_indptr = NULL: no list).
 *   score(u, j)  section 1f's score,  s = +0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t: bit for bit what
 *                predict_multiple / poismf_hip_session_predict return.
 *   answer(u)    the first n_top of L_{list_of(u)} \ E(u) under section 1f's total order (score descending, then item index
 *                ascending).  It is a function of (A[u], B, L_{list_of(u)}, E(u), n_top) alone: not of the other users, how
 *                users are grouped into tiles, the order of the batch or of the list table, how a list is cut into slices or
 *                how the batch is cut into chunks.  It therefore equals section 1h's answer with I(u) = L_{list_of(u)}, bit
 *                for bit in items and scores.
 *   short rows   are not an error: a row with fewer than n_top admissible items is padded as in section 1h with
 *                POISMF_HIP_TOPN_NONE and -inf.  No per-user pre-check is made.
 *   output       out_ix [m x n_top] (row-major) and, unless NULL, out_score [m x n_top]; host arrays, in the caller's order.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, when: a user index
 * >= dimA; an item index >= dimB; a list or exclusion row not strictly ascending, or row pointers that decrease;
 * list_indptr == NULL or list_of == NULL; n_lists == 0 with n_users > 0; an entry of list_of >= n_lists; n_top == 0 or
 * n_top > POISMF_HIP_TOPN_BATCH_MAX_N_TOP; k outside 1..512 float / 1..256 double; exclude_seen for a user outside the
 * session's rows of A; an exclusion row over section 1f's limit; a list table whose rows hold more than
 * POISMF_HIP_TOPN_SHARED_MAX_CELLS indices in all (the 32-bit indices a quarter of the scratch budget holds: the table is
 * uploaded once per call and stays beside every chunk's other parts).  n_users == 0 is not an error (returns 0).  Factors are
 * assumed finite.
 *
 * Memory: ONE scratch allocation per call (session: the one the calls of sections 1f - 1h share) of at most
 * POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB, for any number of users, lists and cells; the batch is cut into chunks of consecutive
 * users.  poismf_hip_topn_shared_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate for a table
 * of n_lists lists that hold n_cells indices in all.  Host work is proportional to n_cells + n_users (+ the exclusion lists).
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_SHARED_MAX_CELLS 16777216        /* most indices of a list table, all rows together: 2^24 */
POISMF_HIP_API int poismf_hip_topn_shared(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *list_indptr, const sparse_ix *list_indices, size_t n_lists, const sparse_ix *list_of,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);
POISMF_HIP_API size_t poismf_hip_topn_shared_scratch_bytes(size_t n_users, size_t n_lists, size_t n_cells, size_t n_top,
        size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1j. Batched exact ranks among per-user candidate lists (sampled evaluation): where each held-out item of many users stands
 *     among a candidate list of the user's own -- sampled negatives plus the positives, the output of a retrieval stage, the
 *     items in stock -- in one fused pass.  Section 1g ranks against the whole catalogue; here only the listed rows of B are
 *     read, so the cost follows the lists' lengths, not dimB.  poismf_amd/metrics.py applies unchanged.
 *
 * For a batch of users u_0 .. u_{m-1} (any order, repeats allowed), per user
 *
 *   T(u)         a held-out list exactly as in section 1g: test_indptr [m + 1], test_indices, strictly ascending rows.
 *   I(u)         an include list exactly as in section 1h: incl_indptr [m + 1], incl_indices, indices < dimB and strictly
 *                ascending within a row; rows may be empty and hold at most POISMF_HIP_TOPN_INCLUDE_MAX_ROW indices.
 *   E(u)         an exclusion set exactly as in section 1f: exclude_seen on a session and / or the CSR-shaped host list
 *                excl_indptr / excl_indices (excl_indptr = NULL: no list).
 *   C(u), N(u)   C(u) = I(u) \ E(u), N(u) = |C(u)|.  N(u) = 0 is valid (an empty list, or one wholly excluded).
 *   rank(u, t)   for t in T(u) and in C(u): the number of j in C(u) that come before t under section 1f's total order with
 *                section 1f's score (bit for bit what predict_multiple / poismf_hip_session_predict return).  The answer is
 *                by definition section 1g's for the exclusion set E(u) united with {0..dimB-1} \ I(u), in out_rank and in
 *                out_n_adm alike, as section 1h states for the top-N; the batched top-N of section 1h with the same lists
 *                and n_top > rank lists t at index rank.  A rank is a function of (A[u], B, I(u), E(u), t) alone: not of
 *                the other users or cells, the batch order, how a list is cut into slices or how the batch is cut into
 *                chunks.  All counting is in integers; there are no float atomics.
 *   excluded     a held-out cell whose item is not in C(u) -- in E(u), or not listed in I(u) -- gets
 *                POISMF_HIP_RANK_EXCLUDED; it is not an error.  (A caller that passes sampled negatives alone unites each
 *                user's held-out row into its list first; poismf_amd.api.eval_ranking(include=) does.)
 *   output       out_rank: one unsigned int per entry of test_indices, in the caller's order; out_n_adm [m]: N(u).  Host arrays.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, in the cases of sections
 * 1g and 1h together: a user index >= dimA; an item index >= dimB; a test, include or exclusion row not strictly ascending, or
 * row pointers that decrease; test_indptr == NULL or incl_indptr == NULL; k outside 1..512 float / 1..256 double; exclude_seen
 * for a user outside the session's rows of A; an exclusion row over section 1f's limit; a held-out row longer than
 * POISMF_HIP_RANK_BATCH_MAX_ROW; an include row longer than POISMF_HIP_TOPN_INCLUDE_MAX_ROW.  n_users == 0 is not an error
 * (returns 0).  Factors are assumed finite.
 *
 * Memory: ONE scratch allocation per call (session: the one the calls of sections 1f - 1i share) of at most
 * POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB, for any number of users, held-out cells and candidates; the batch is cut into chunks of
 * users whose lists fit.  poismf_hip_rank_include_scratch_bytes (testing aid, no HIP call) is the size both entry points
 * allocate for a batch with n_test_cells held-out cells and n_incl_cells candidates in all.  A list is cut into slices of
 * POISMF_HIP_RANK_INCLUDE_SLICE candidates, one wave each; a wave keeps up to POISMF_HIP_RANK_INCLUDE_GROUP of the user's
 * held-out scores in LDS, and a user with more has them searched in device memory instead (slower per candidate, same answer).
 * poismf_hip_rank_include's own copies of B and of A (all of A, or only the batch's rows when n_users < dimA) come on top.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_RANK_INCLUDE_SLICE 1024   /* candidates of a list that one wave scores */
#define POISMF_HIP_RANK_INCLUDE_GROUP 128    /* held-out items of a user whose scores a wave keeps in LDS */
POISMF_HIP_API int poismf_hip_rank_include(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users,
        const sparse_ix *test_indptr, const sparse_ix *test_indices,
        const sparse_ix *incl_indptr, const sparse_ix *incl_indices,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        unsigned int *out_rank, unsigned int *out_n_adm);
POISMF_HIP_API size_t poismf_hip_rank_include_scratch_bytes(size_t n_users, size_t n_test_cells, size_t n_incl_cells,
        size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1k. Batched exact ranks among candidate lists SHARED between users (sampled evaluation against one pool): section 1j's ranks
 *     when few lists serve many users -- 1000 negatives sampled once for everybody, a popularity-stratified pool, the items in
 *     stock in a region.  Section 1j takes every user's copy of its list and every user gathers its own rows of B.  Here the
 *     host reads each list once, and on the device 64 rows of held-out items that refer to one list share every row of B they
 *     gather (the f32-MFMA tile of section 1f with section 1g's counting).  It is to section 1j what section 1i is to 1h.
 *
 * For a batch of users u_0 .. u_{m-1} (any order, repeats allowed), and
 *
 *   T(u)         a held-out list exactly as in section 1g: test_indptr [m + 1], test_indices, strictly ascending rows.
 *   L_0..L_{G-1} a table of candidate lists and list_of [m] exactly as in section 1i: list_indptr [G + 1], list_indices,
 *                indices < dimB and strictly ascending within a row; list_of[i] < G.  Rows may be empty.  A list no user
 *                refers to is valid and costs nothing on the device.  At most POISMF_HIP_TOPN_SHARED_MAX_CELLS indices in all.
 *   E(u)         an exclusion set exactly as in section 1f: exclude_seen on a session and / or the CSR-shaped host list
 *                excl_indptr / excl_indices (excl_indptr = NULL: no list).
 *   unite_test   == 0: C(u) = L_{list_of(u)} \ E(u).  A held-out cell whose item is not in C(u) -- in E(u), or not listed --
 *                gets POISMF_HIP_RANK_EXCLUDED.  By definition this is section 1j's answer with I(u) = L_{list_of(u)}, in
 *                out_rank and in out_n_adm alike.
 *                != 0: C(u) = (L_{list_of(u)} united with T(u)) \ E(u); only the cells in E(u) are marked.  By definition this is
 *                section 1j's answer with I(u) the union of the list and the user's held-out row.  It is the mode a shared
 *                pool of negatives needs: a shared list cannot have each user's positives written into it.
 *   N(u)         |C(u)|.  N(u) = 0 is valid (an empty list, or one wholly excluded).
 *   rank(u, t)   for t in T(u) and in C(u): the number of j in C(u) that come before t under section 1f's total order with
 *                section 1f's score (bit for bit what predict_multiple / poismf_hip_session_predict return).  The batched
 *                top-N of section 1i with the same table and n_top > rank lists a listed t at index rank when unite_test == 0.
 *                A rank is a function of (A[u], B, L_{list_of(u)}, T(u) when united, E(u), t) alone: not of the other users,
 *                how users or held-out items are grouped into tiles, the order of the batch or of the table, how a list is
 *                cut into slices or how the batch is cut into chunks.  All counting is in integers; there are no float atomics.
 *   output       out_rank: one unsigned int per entry of test_indices, in the caller's order; out_n_adm [m]: N(u).  Host arrays.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, in the cases of sections
 * 1g and 1i together: a user index >= dimA; an item index >= dimB; a test, list or exclusion row not strictly ascending, or row
 * pointers that decrease; test_indptr == NULL, list_indptr == NULL or list_of == NULL; n_lists == 0 with n_users > 0; an entry
 * of list_of >= n_lists; k outside 1..512 float / 1..256 double; exclude_seen for a user outside the session's rows of A; an
 * exclusion row over section 1f's limit; a held-out row longer than POISMF_HIP_RANK_BATCH_MAX_ROW; a list table whose rows hold
 * more than POISMF_HIP_TOPN_SHARED_MAX_CELLS indices in all.  n_users == 0 is not an error (returns 0).  Factors are assumed
 * finite.
 *
 * Memory: ONE scratch allocation per call (session: the one the calls of sections 1f - 1j share) of at most
 * POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB, for any number of users, held-out cells, lists and list indices.  The table goes up once
 * per call, narrowed to 32 bits, and a chunk's parts lie beside it; the batch is cut into chunks of consecutive users that
 * carry at most POISMF_HIP_RANK_SHARED_CHUNK_CELLS held-out cells together (one row of the longest kind always fits).
 * poismf_hip_rank_shared_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate; it never decreases
 * when one of its arguments grows.  Host work is proportional to n_list_cells + n_users + n_test_cells (+ the exclusion lists),
 * never to users x list length.  poismf_hip_rank_shared's own copies of B and of A (all of A, or only the batch's rows when
 * n_users < dimA) come on top.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_RANK_SHARED_CHUNK_CELLS 524288   /* most held-out cells of one chunk of users: 2^19 */
POISMF_HIP_API int poismf_hip_rank_shared(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users,
        const sparse_ix *test_indptr, const sparse_ix *test_indices,
        const sparse_ix *list_indptr, const sparse_ix *list_indices, size_t n_lists, const sparse_ix *list_of,
        int unite_test,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        unsigned int *out_rank, unsigned int *out_n_adm);
POISMF_HIP_API size_t poismf_hip_rank_shared_scratch_bytes(size_t n_users, size_t n_test_cells, size_t n_lists,
        size_t n_list_cells, size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1l. Deep batched top-N: section 1f's answer for n_top up to POISMF_HIP_TOPN_DEEP_MAX_N_TOP = 1024 -- candidate generation for a
 *     re-ranker, the stage whose output sections 1h and 1i consume.  (The reference's topN has no cap on n_top but serves one user
 *     per call, ref: src/topN.c:112-284.)
 *
 * Arguments, E(u), score(u, j), the total order, the output arrays and the return codes are section 1f's, except:
 *
 *   range        n_top is 1 .. POISMF_HIP_TOPN_DEEP_MAX_N_TOP.  Where n_top <= POISMF_HIP_TOPN_BATCH_MAX_N_TOP and every user keeps
 *                n_top admissible items, items and score bits are those of poismf_hip_topn_batch.
 *   answer(u)    the first n_top of {0..dimB-1} \ E(u) under "score descending, then item index ascending": a function of
 *                (A[u], B, E(u), n_top) alone -- not of the other users, their order, how the items are cut into slices or how the
 *                batch is cut into chunks.
 *   short rows   are not an error (section 1h's rule, not 1f's): when only c < n_top items are admissible, entries c .. n_top-1
 *                of the row are POISMF_HIP_TOPN_NONE in out_ix and -inf in out_score.  n_top > dimB is therefore valid.  No
 *                per-user pre-check is made and nothing of a resident row is downloaded to count a union.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, for n_top == 0,
 * n_top > POISMF_HIP_TOPN_DEEP_MAX_N_TOP and everything that is 2 in section 1f except "too few items left" (an exclusion row may
 * hold up to min(dimB, POISMF_HIP_TOPN_BATCH_BUDGET_MB / 8 Mi) entries, as there).  n_users == 0 returns 0.
 *
 * Memory: a user's candidate list cannot live in LDS at this depth (section 1f keeps n_top + 48 entries for each of a
 * workgroup's 64 users there).  It lives in the call's scratch: per (user, slice of the items) `cap` entries of (score, item),
 * cap = the power of two at or above n_top + max(n_top / 2, 64) (2048 at n_top = 1024), sorted down to the best n_top by the
 * list's own wave whenever fewer than 64 slots are free.  ONE allocation per call (session: the one sections 1f - 1k share; it grows
 * and never shrinks under them) of at most POISMF_HIP_TOPN_DEEP_BUDGET_MB MiB for any n_users;
 * poismf_hip_topn_deep_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate, and it never decreases
 * when n_users grows.  The budget's arithmetic, for the largest case (float, n_top = 1024, cap = 2048, 8 B per entry):
 *   - the lists are sized for items cut into slices until a chunk of users has 512 workgroups = two on each of the 256 CUs; 64
 *     lists each: 64 x 512 x 2048 x 8 B = 512 MiB.  A chunk of u users adds at most one more list per user: u x 2048 x 8 B;
 *   - exclusion indices of a chunk: 128 MiB at most (section 1f's area);  results: u x 1024 x 8 B;  users and row pointers: u x 8 B.
 *   1024 MiB leave 384 MiB for the parts that grow with u: chunks of 16 320 users = 255 tiles of 64, two workgroups per CU before
 *   the items are cut at all.  In double an entry is 12 B: 768 MiB of lists for 512 workgroups, chunks of 3 584 users.  The chunk
 *   grows as n_top shrinks (262 144 users at most, section 1f's bound).  (Where a CU's LDS holds only one workgroup, as at this
 *   depth, the planner stops cutting at 256 workgroups: more would add lists to fill and merge, and no parallelism.)
 * poismf_hip_topn_deep's own copies of B and of A (all of A, or only the batch's rows) come on top.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_DEEP_MAX_N_TOP 1024    /* largest n_top of the deep entry points */
#define POISMF_HIP_TOPN_DEEP_BUDGET_MB 1024    /* upper bound of their scratch allocation, MiB */
POISMF_HIP_API int poismf_hip_topn_deep(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);
POISMF_HIP_API size_t poismf_hip_topn_deep_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1n. Batched top-N with per-group quotas: section 1f's ranked list with "at most q items of one brand / seller / category on a
 *     page" applied on the device, in the same fused pass (no counterpart in the reference).
 *
 * Inputs are section 1f's -- users u_0 .. u_{m-1} (any order, repeats allowed), n_top, E(u), score(u, j) and the total order
 * "score descending, then item index ascending" -- and two host arrays of sparse_ix:
 *
 *   group_of     [dimB]: the group g(j) in 0 .. n_groups-1 of every item.  A group with no items is fine.
 *   quota        [n_groups]: q(g) >= 0.  q(g) = 0: no item of the group is ever returned.  q(g) >= n_top: the group is
 *                unconstrained (quotas above n_top are clipped to n_top on the host when they are narrowed to 32 bits).
 *
 * With Adm(u) = {0..dimB-1} \ E(u):
 *
 *   r(u, j)      #{ i in Adm(u) : g(i) = g(j), i before j in the total order }   -- the in-group rank among ADMISSIBLE items
 *   Q(u)         { j in Adm(u) : r(u, j) < q(g(j)) }
 *   answer(u)    the first n_top of Q(u) under the total order.  This is exactly the result of walking u's complete ranked list
 *                and taking an item iff fewer than q(g) items of its group were taken, until n_top are taken.  It is a function
 *                of (A[u], B, E(u), group_of, quota, n_top) alone: not of the other users, the order of the batch, how the items
 *                are cut into slices or how the users are cut into chunks.
 *   scores       bit for bit predict_multiple's, as in section 1f.  No float atomics.
 *   short rows   follow section 1h / 1l's rule, not 1f's: if |Q(u)| = c < n_top, entries c .. n_top-1 of the row are
 *                POISMF_HIP_TOPN_NONE in out_ix and -inf in out_score.  No per-user pre-check is made and nothing of a resident
 *                row is downloaded to count a union.
 *   range        n_top is 1 .. POISMF_HIP_TOPN_BATCH_MAX_N_TOP.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, for: everything that is 2 in
 * section 1f except "too few items left"; group_of == NULL or quota == NULL with n_users > 0; n_groups == 0 (or above 2^31 - 1: a
 * group id is narrowed to 32 bits); an entry of group_of that is >= n_groups, or negative in the R flavour; a negative quota in the
 * R flavour; dimB > POISMF_HIP_TOPN_QUOTA_MAX_ITEMS.  n_users == 0 returns 0.
 *
 * Slow path: where the quotas of the groups that have admissible items sum to less than n_top, the selection threshold never
 * rises, every admissible item becomes a candidate and the call is slow.  Its answer is correct and padded.
 *
 * Memory: ONE scratch allocation per call (session: the one sections 1f - 1l share) of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB for
 * any n_users.  The two maps go up once per call, per item and narrowed to 32 bits (the group, and its quota): 2 x 4 B x dimB,
 * together at most 128 MiB at the item limit.  They lie in front of the chunk's parts; the chunk of users is sized from what the
 * budget leaves beside maps of that largest size and an exclusion area of min(dimB x chunk, 2^24) indices, so every valid exclusion
 * row fits.  poismf_hip_topn_quota_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate; it never
 * decreases when n_users grows.  poismf_hip_topn_quota's own copies of B and of A (all of A, or only the batch's rows) come on top.
 * The session flavour, poismf_hip_session_topn_quota, is declared in section 2.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_QUOTA_MAX_ITEMS 16777216   /* largest dimB of the quota entry points (2^24) */
POISMF_HIP_API int poismf_hip_topn_quota(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *group_of, size_t n_groups, const sparse_ix *quota,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);
POISMF_HIP_API size_t poismf_hip_topn_quota_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t n_groups, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1o. Batched top-N with per-item score weights: section 1f's ranked list of "score times a value of the item" -- expected revenue
 *     (rate x price), a popularity discount, a freshness decay, a boost or a penalty -- with the multiplication made on the device,
 *     in the same fused pass, before anything is pruned (no counterpart in the reference).
 *
 * Inputs are section 1f's -- users u_0 .. u_{m-1} (any order, repeats allowed), n_top, E(u), score(u, j) -- and one host array:
 *
 *   item_weight  [dimB] of real_t: finite and >= 0.  A weight of 0 does NOT bar an item: the item scores 0 (-0 is taken as 0) and
 *                ties with its like by index; barring an item is what the exclusion lists are for.
 *
 *   wscore(u, j) score(u, j) * item_weight[j]: ONE multiplication rounded to real_t, made after the k-ordered fused chain and never
 *                contracted into it.
 *   answer(u)    the first n_top of {0..dimB-1} \ E(u) under "wscore descending, then item index ascending".  It is a function of
 *                (A[u], B, item_weight, E(u), n_top) alone: not of the other users, the order of the batch, how the items are cut
 *                into slices or how the users are cut into chunks.
 *   scores       out_score is wscore: bit for bit predict_multiple's score multiplied by item_weight[j] in real_t.  With every
 *                weight 1 the rows are section 1f's, bit for bit.  No float atomics.  Where a product is denormal the result is
 *                unspecified (the score or the order of such items may differ from the host's product).
 *   short rows   follow section 1h / 1l / 1n's rule, not 1f's: if fewer than n_top items are admissible, the rest of the row is
 *                POISMF_HIP_TOPN_NONE in out_ix and -inf in out_score.  No per-user pre-check is made and nothing of a resident row
 *                is downloaded to count a union.
 *   range        n_top is 1 .. POISMF_HIP_TOPN_BATCH_MAX_N_TOP.
 *
 * A caller of poismf_hip_topn_weighted who wants the items most similar to some items passes B as A too (users then index rows of
 * B and dimA = dimB); the session call has query_B for that.  With item_weight[j] = 1 / |B_j| the order is the order by cosine
 * similarity, and exclusion row i = { the query item } leaves the item itself out.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, for: everything that is 2 in
 * section 1f except "too few items left"; item_weight == NULL with n_users > 0; a weight that is NaN, infinite or negative;
 * dimB > POISMF_HIP_TOPN_WEIGHTED_MAX_ITEMS.  n_users == 0 returns 0.
 *
 * Memory: ONE scratch allocation per call (session: the one sections 1f - 1n share) of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB for
 * any n_users.  The weights go up once per call, sizeof(real_t) x dimB, at most 128 MiB in double at the item limit.  They lie in
 * front of the chunk's parts; the chunk of users is sized from what the budget leaves beside weights of that largest size and an
 * exclusion area of min(dimB x chunk, 2^24) indices, so every valid exclusion row fits.  poismf_hip_topn_weighted_scratch_bytes
 * (testing aid, no HIP call) is the size both entry points allocate; it does not depend on k.  poismf_hip_topn_weighted's own copies
 * of B and of A (all of A, or only the batch's rows) come on top.  The session flavour, poismf_hip_session_topn_weighted, is declared
 * in section 2.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_WEIGHTED_MAX_ITEMS 16777216   /* largest dimB of the weighted entry points (2^24) */
POISMF_HIP_API int poismf_hip_topn_weighted(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top,
        const real_t *item_weight,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);
POISMF_HIP_API size_t poismf_hip_topn_weighted_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1p. Diversified batched top-N: greedy maximal marginal relevance (MMR) over a pool of every user's best items, picked on the
 *     device from the factors themselves -- no group label per item is needed, as section 1n needs one (no counterpart in the
 *     reference).
 *
 * Inputs are section 1l's -- users u_0 .. u_{m-1} (any order, repeats allowed), E(u), score(u, j) and the total order "score
 * descending, then item index ascending" -- and:
 *
 *   n_top          1 .. POISMF_HIP_TOPN_BATCH_MAX_N_TOP (128): the picks per user.
 *   pool           n_top .. POISMF_HIP_TOPN_DEEP_MAX_N_TOP (1024): the candidates the picks are made among.
 *   lambda         a double in [0, 1]: 1 is pure relevance, 0 pure diversity.
 *   item_inv_norm  [dimB], a host array of real_t, finite and >= 0: 1 / sqrt(chain(B_j, B_j)), and 0 for a zero row of B.
 *
 * All arithmetic is in real_t; every operation below is rounded once and never contracted into a fused multiply-add.
 *
 *   P(u)         the first `pool` entries of section 1l's answer for (u, pool), at positions 0 .. c(u)-1, c(u) <= pool.  rel_i is the
 *                score of position i, with predict_multiple's bits; j_i is its item.
 *   r_i          rel_i / rel_0 (IEEE division) when rel_0 > 0, otherwise rel_i.
 *   lam, oml     (real_t)lambda and (real_t)(1 - lambda), the difference taken in double; both rounded on the host.
 *   chain(x, y)  the fused chain s = +0; for c in 0..k-1: s = fma(x_c, y_c, s): predict_multiple(B, B, j_i, j_q)'s, symmetric in
 *                its arguments.
 *   cos(i, q)    ((chain(B[j_i], B[j_q]) * inv[j_i]) * inv[j_q]), two rounded multiplications in this order.  Not clipped.
 *   m_i          0 for every position before any pick; after picking position q, m_i = (cos(i, q) > m_i ? cos(i, q) : m_i) for
 *                every unpicked i.
 *   v_i          (lam * r_i) - (oml * m_i): two rounded products, one rounded difference.
 *   picks        at each step the unpicked position with the largest v_i; ties (v equal, -0 = +0) go to the lowest position.  The
 *                first pick is therefore always position 0.  Picking stops after n_top picks or when the pool is used up.
 *
 * Outputs, [n_users x n_top] in pick order: out_ix the picked items; out_score (may be NULL) the picked item's RELEVANCE rel, with
 * predict_multiple's bits; out_value (may be NULL) v at the moment of the pick.  Short rows follow section 1l's rule: entries a row
 * does not reach are POISMF_HIP_TOPN_NONE, -inf and -inf.  The answer is a function of (A[u], B, E(u), item_inv_norm, n_top, pool,
 * lambda) alone: not of the other users, the order of the batch, how the items are cut into slices or how the users are cut into
 * chunks.  No float atomics.  Where a product or a quotient is denormal the result is unspecified, as in section 1o.  Consequences:
 *   - lambda = 1 gives the first n_top entries of section 1l's answer (and section 1f's, where every user keeps n_top items), items
 *     and scores bit for bit: v_i = r_i, which does not increase with i;
 *   - pool = n_top gives the SET of the plain top-N, in MMR order.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, for everything that is 2 in
 * section 1l (with `pool` as its n_top), and for: n_top == 0 or n_top > POISMF_HIP_TOPN_BATCH_MAX_N_TOP; pool < n_top or
 * pool > POISMF_HIP_TOPN_DEEP_MAX_N_TOP; lambda NaN or outside [0, 1]; item_inv_norm == NULL with n_users > 0; an entry of
 * item_inv_norm that is NaN, infinite or negative; dimB > POISMF_HIP_TOPN_DIVERSE_MAX_ITEMS.  n_users == 0 returns 0.
 *
 * Memory: ONE scratch allocation per call (session: the one sections 1f - 1o share) of at most POISMF_HIP_TOPN_DIVERSE_BUDGET_MB MiB
 * for any n_users; poismf_hip_topn_diverse_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate, it does
 * not depend on k and never decreases when n_users grows.  The budget's arithmetic:
 *   - the inverse norms go up once per call and lie in front of the chunk's parts: sizeof(real_t) x dimB, at most 8 B x 2^24 =
 *     128 MiB in double at the item limit;
 *   - behind them lies section 1l's layout for n_top = pool, inside section 1l's budget of 1024 MiB, with the chunk of users cut so
 *     that the picked rows fit the same budget: n_top x (4 B + 2 x sizeof(real_t)) per user, at most 128 x 20 B = 2.5 KiB against
 *     the 36 KiB a user's lists and results take at pool = 1024 in double (chunks of 3 328 users there instead of 3 584).
 *   1024 + 128 = 1152 MiB.
 * The MMR stage keeps no pool in LDS: it reads the pool's rows of B again for every pick, (n_top - 1) x c(u) x k x sizeof(real_t)
 * bytes per user out of the caches.  poismf_hip_topn_diverse's own copies of B and of A (all of A, or only the
 * batch's rows) come on top.  The session flavour, poismf_hip_session_topn_diverse, is declared in section 2.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_DIVERSE_MAX_ITEMS 16777216   /* largest dimB of the diversified entry points (2^24) */
#define POISMF_HIP_TOPN_DIVERSE_BUDGET_MB 1152       /* upper bound of their scratch allocation, MiB: section 1l's and the norms */
POISMF_HIP_API int poismf_hip_topn_diverse(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top, size_t pool, double lambda,
        const real_t *item_inv_norm,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score, real_t *out_value);
POISMF_HIP_API size_t poismf_hip_topn_diverse_scratch_bytes(size_t n_users, size_t n_top, size_t pool, size_t dimB, size_t k);

/* ---------------------------------------------------------------------------------------------
 * 1q. List-wise evaluation: where held-out items sit in given top-N lists, how similar the listed items are to each other and how
 *     often each item is shown -- for lists from any source, in the form sections 1f - 1p return them (no counterpart in the
 *     reference).  No user index and no A enter the call: the lists are the input.
 *
 *   B              [dimB x k] row-major.
 *   lists          [n_users x n_list] item indices, 1 <= n_list <= POISMF_HIP_TOPN_BATCH_MAX_N_TOP (128).  Row u holds c(u) <= n_list
 *                  real entries followed only by POISMF_HIP_TOPN_NONE; the real entries are distinct and below dimB.  Rows may repeat.
 *   item_inv_norm  optional (NULL: none).  [dimB], a host array of real_t, finite and >= 0: section 1p's.
 *   test_indptr    optional (NULL: none).  [n_users + 1] row pointers into test_indices, from any non-negative start; every row strictly
 *   test_indices   ascending, below dimB and at most POISMF_HIP_RANK_BATCH_MAX_ROW long.  `cells` below is their number,
 *                  test_indptr[n_users] - test_indptr[0], and cell p - test_indptr[0] stands for test_indices[p].
 *
 * Outputs, all integers, so that no result depends on the order of any sum:
 *
 *   out_pos    [cells] unsigned int, written only with a held-out CSR (then it must not be NULL): the 0-based position of the cell's
 *              item in its row of `lists`, or POISMF_HIP_LIST_ABSENT when the row does not list it.
 *   out_cos    [n_users] long long, written only with item_inv_norm (then it must not be NULL).  For the positions p < q < c(u) of a
 *              row, with items jp and jq:
 *                cs = ((chain(B[jq], B[jp]) * inv[jq]) * inv[jp])    section 1p's chain (s = +0; s = fma(x_c, y_c, s), c ascending,
 *                                                                    predict_multiple's bits) and its two multiplications, each
 *                                                                    rounded once in real_t and never contracted: the later position
 *                                                                    is the candidate and the earlier the picked one, exactly as
 *                                                                    section 1p multiplies;
 *                t  = (double)cs, 0 when cs is NaN, clamped to [-2, 2];
 *                Q  = llrint(t * 2^POISMF_HIP_LIST_COS_SHIFT), round half to even (the product is exact);
 *              out_cos[u] is the sum of Q over the row's c (c - 1) / 2 pairs: at most 8128 x 2^41 in magnitude.
 *   out_len    [n_users] unsigned int: c(u).
 *   exposure   [dimB] unsigned int: how many rows list item j (a repeated row counts each time).  Zeroed by the call.
 *
 * Every output of a row is a function of that row, B and item_inv_norm alone -- not of the other rows, their order or how the rows are
 * cut into chunks -- and exposure is the sum over the rows.  The only atomics are unsigned integer adds on `exposure`.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, for: B, lists, out_len or
 * exposure NULL; n_list == 0 or n_list > POISMF_HIP_TOPN_BATCH_MAX_N_TOP; k outside 1..512 float / 1..256 double;
 * dimB > POISMF_HIP_LIST_EVAL_MAX_ITEMS; a row of `lists` with a real entry behind a POISMF_HIP_TOPN_NONE, a repeated real entry or
 * an entry >= dimB; an entry of item_inv_norm that is NaN, infinite or negative; out_cos NULL with item_inv_norm; out_pos NULL or
 * test_indices NULL with cells; a held-out CSR whose row pointers decrease or start below 0, a held-out row that is not strictly
 * ascending, holds an index >= dimB or is longer than POISMF_HIP_RANK_BATCH_MAX_ROW; a budget_bytes below what one user needs (see
 * below).  n_users == 0 returns 0 and touches nothing.
 *
 * Memory: ONE scratch allocation per call (session: the one sections 1f - 1p share) of at most POISMF_HIP_LIST_EVAL_BUDGET_MB MiB
 * whatever n_users and cells.  It holds, once per call, the inverse norms (sizeof(real_t) x dimB) and the exposure counts (4 B x dimB) --
 * 12 B x 2^24 = 192 MiB in double at the item limit -- and behind them a chunk of users: 4 n_list + 16 B per user (its row, its first
 * cell, its sum and its length) and 8 B per cell (item and position).  budget_bytes = 0 means the default,
 * POISMF_HIP_LIST_EVAL_BUDGET_MB MiB, and so does any larger value; a smaller one cuts the users into more chunks, and one too small for
 * the norms, the counts, one user and min(cells, POISMF_HIP_RANK_BATCH_MAX_ROW) cells returns 2.
 * poismf_hip_list_eval_scratch_bytes (testing aid, no HIP call) is the size both entry points allocate -- 0 where they would return 2
 * for the budget; it never exceeds the budget, and with the other arguments fixed it grows with n_users until a chunk is full and
 * stays there, so the n_users from which it no longer grows is the most users one chunk takes (a chunk also ends where the next
 * user's cells would not fit).  poismf_hip_list_eval's own copy of B comes on top.  The session flavour, poismf_hip_session_list_eval, is declared in section 2.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_LIST_ABSENT 0xFFFFFFFEu           /* out_pos of a held-out item its row does not list */
#define POISMF_HIP_LIST_COS_SHIFT 40                 /* out_cos counts cosines in units of 2^-40 */
#define POISMF_HIP_LIST_EVAL_MAX_ITEMS 16777216      /* largest dimB of the list evaluation (2^24) */
#define POISMF_HIP_LIST_EVAL_BUDGET_MB 256           /* upper bound of its scratch allocation, MiB */
POISMF_HIP_API int poismf_hip_list_eval(const real_t *B, int k, size_t dimB,
        const sparse_ix *lists, size_t n_users, size_t n_list,
        const real_t *item_inv_norm,
        const sparse_ix *test_indptr, const sparse_ix *test_indices, size_t budget_bytes,
        unsigned int *out_pos, long long *out_cos, unsigned int *out_len, unsigned int *exposure);
POISMF_HIP_API size_t poismf_hip_list_eval_scratch_bytes(size_t n_users, size_t n_list, size_t n_cells, size_t dimB, size_t budget_bytes);

/* ---------------------------------------------------------------------------------------------
 * 1r. Batched top-N with per-(user, item) score factors: section 1f's ranked list where single cells of the score matrix are
 *     multiplied by a factor of their own -- an impression discount, a repeat-consumption discount on the user's seen items, a
 *     per-user boost -- on the device, exactly, in one call (no counterpart in the reference).
 *
 * Inputs are section 1f's -- users u_0 .. u_{m-1} (any order, repeats allowed), n_top, E(u), score(u, j) -- and a CSR-shaped host
 * list with one row per user of the batch:
 *
 *   adj_indptr   [n_users + 1] row pointers into adj_indices / adj_factor, from any non-negative start, never decreasing.  An
 *                all-empty list is passed as row pointers of zeros.
 *   adj_indices  items, below dimB and strictly ascending within a row; a row holds at most POISMF_HIP_TOPN_ADJUSTED_MAX_ROW cells.
 *   adj_factor   real_t, parallel to adj_indices: finite and >= 0.  A factor of 0 does NOT bar a cell: the cell scores 0 (-0 is
 *                taken as 0) and ties with its like by index; barring a cell is what the exclusion lists are for.
 *
 *   ascore(u, j) score(u, j) * f(u, j) where (u, j) is listed -- ONE multiplication rounded to real_t, made after the k-ordered fused
 *                chain and never contracted into it -- and score(u, j) untouched otherwise.
 *   answer(u)    the first n_top of {0..dimB-1} \ E(u) under "ascore descending, then item index ascending".  It is a function of
 *                (A[u], B, the user's adjust row, E(u), n_top) alone: not of the other users, the order of the batch, how the items
 *                or a long adjust row are cut into slices or how the users are cut into chunks.  A cell that is listed and in E(u)
 *                is excluded.
 *   scores       out_score is ascore: bit for bit predict_multiple's score, multiplied by the factor in real_t where the cell is
 *                listed.  With no cell listed, or every factor 1, the rows are section 1f's, bit for bit.  No float atomics.  Where
 *                a product is denormal or NaN (a factor of 0 on an infinite score) the result is unspecified, as in section 1o.
 *   short rows   follow section 1h's rule: if fewer than n_top items are admissible, the rest of the row is POISMF_HIP_TOPN_NONE in
 *                out_ix and -inf in out_score.
 *   range        n_top is 1 .. POISMF_HIP_TOPN_BATCH_MAX_N_TOP; dimB <= POISMF_HIP_TOPN_ADJUSTED_MAX_ITEMS.
 *
 * Returns 0; 1 on a device error / out of memory; 2, with nothing written and before any device work, for: everything that is 2 in
 * section 1o apart from its weight clauses; adj_indptr == NULL with n_users > 0; row pointers that decrease, start below 0 or leave
 * the list (adj_indices or adj_factor NULL with cells); an index >= dimB; a row that is not strictly ascending or is longer than
 * POISMF_HIP_TOPN_ADJUSTED_MAX_ROW; a factor that is NaN, infinite or negative.  n_users == 0 returns 0.
 *
 * Two stages and a merge: the dense pass of section 1f over all items with the user's listed cells treated
 * as excluded, a gather of the listed rows of B only (section 1h's) whose scores are multiplied by their factors, and one merge per
 * user of the sorted partial lists of both.
 *
 * Memory: ONE scratch allocation per call (session: the one sections 1f - 1q share) of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB MiB for
 * any n_users and any number of listed cells: an exclusion area of at most 2^24 indices (64 MiB; a user's exclusion row united with
 * its adjust row is no longer than dimB, so every valid row fits), an adjust area of at most POISMF_HIP_TOPN_ADJUSTED_MAX_ROW cells
 * (index and factor: 48 MiB in double), and in the rest the chunk's users, work items, partial lists and results; the chunk of
 * users is cut where one of the areas is full.  A user's partial lists are its own: the item slices of the dense stage and, behind
 * them, one per work item of its adjust row; a long row costs the other users of its chunk nothing.  An adjust row of len cells is
 * cut into poismf_hip_topn_adjusted_slices(len, n_top, 0) work items (testing aid, no HIP call).  That count is not monotone in len
 * (the cells per work item are rounded up to 64), and the row may lose cells to the exclusion list after the chunk was cut, so the
 * cut charges the row poismf_hip_topn_adjusted_slices(len, n_top, 1) lists: a bound that never decreases with len and is no less
 * than the work items of any row of at most len cells.  poismf_hip_topn_adjusted_scratch_bytes (testing aid, no HIP call; n_cells is
 * adj_indptr[n_users] - adj_indptr[0]) is the size both entry points allocate; it does not depend on k.  poismf_hip_topn_adjusted's
 * own copies of B and of A (all of A, or only the batch's rows) come on top.  The session flavour,
 * poismf_hip_session_topn_adjusted, is declared in section 2.
 * ------------------------------------------------------------------------------------------- */
#define POISMF_HIP_TOPN_ADJUSTED_MAX_ITEMS 16777216   /* largest dimB of the adjusted entry points (2^24) */
#define POISMF_HIP_TOPN_ADJUSTED_MAX_ROW 4194304      /* longest adjust row: 2^22 cells */
POISMF_HIP_API int poismf_hip_topn_adjusted(const real_t *A, const real_t *B, int k, size_t dimA, size_t dimB,
        const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *adj_indptr, const sparse_ix *adj_indices, const real_t *adj_factor,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);
POISMF_HIP_API size_t poismf_hip_topn_adjusted_scratch_bytes(size_t n_users, size_t n_cells, size_t n_top, size_t dimB, size_t k);
POISMF_HIP_API size_t poismf_hip_topn_adjusted_slices(size_t len, size_t n_top, int bound);

/* ---------------------------------------------------------------------------------------------
 * 2. Device-resident session: the same path with X, A and B kept in HBM between calls, one
 *    half-sweep per call.  This is what bench.py times (inputs already resident) and what the
 *    one-process-per-GPU driver uses: each rank owns a contiguous range of A rows and of B rows,
 *    both factors are replicated, and the caller all-gathers the updated shard between halves.
 *
 * Replaces, per call: sum_by_cols + l1 + PG pre-scaling (ref: src/poismf.c:77-83, :512-526,
 * :562-577) and pg_iteration / cg_iteration / tncg_iteration (ref: src/poismf.c:139-188, :275-322,
 * :324-404) for the rows of the shard.
 * ------------------------------------------------------------------------------------------- */
typedef struct poismf_hip_session poismf_hip_session;

/* Creates a session on HIP device `device`.  Xr* / Xc* are HOST CSR / CSC arrays of the WHOLE matrix
 * (size_t indices, as in run_poismf); only rows [rowA_begin,rowA_end) of the CSR and rows
 * [rowB_begin,rowB_end) of the CSC (= columns of X) are uploaded.  Pass 0,dimA / 0,dimB for a
 * single-GPU session.  `stream` is a hipStream_t passed as void*; all work of this session is enqueued on it.
 * NULL does NOT mean the legacy default stream: the session then creates and owns a non-blocking stream of its
 * own, which is not ordered against work the caller enqueues elsewhere -- a caller that touches the factors
 * through the device pointers below must either pass its own stream here or order its work against
 * poismf_hip_session_stream().  Returns 0, or 1 when out of memory / no device. */
POISMF_HIP_API int poismf_hip_session_create(
    poismf_hip_session **out, int device, void *stream,
    const real_t *Xr, const sparse_ix *Xr_indptr, const sparse_ix *Xr_indices,
    const real_t *Xc, const sparse_ix *Xc_indptr, const sparse_ix *Xc_indices,
    size_t dimA, size_t dimB, size_t k,
    size_t rowA_begin, size_t rowA_end, size_t rowB_begin, size_t rowB_end);

/* The same session built from HOST COO triplets (what PoisMF._process_data holds, ref: poismf/__init__.py:404-414):
 * both orientations are converted on the device (duplicates summed, indices sorted, section 1c) and stay there -- the
 * CSR / CSC never exist in host memory.  Only triplets whose row lies in [rowA_begin,rowA_end) enter the CSR shard and
 * only those whose column lies in [rowB_begin,rowB_end) the CSC shard.  Requires n < 2^32.  Returns 0; 1 out of memory / no
 * device; 3 when a row or column index lies outside the matrix (it would become a gather offset into the factors). */
POISMF_HIP_API int poismf_hip_session_create_coo(
    poismf_hip_session **out, int device, void *stream,
    const sparse_ix *row, const sparse_ix *col, const real_t *val, size_t n,
    size_t dimA, size_t dimB, size_t k,
    size_t rowA_begin, size_t rowA_end, size_t rowB_begin, size_t rowB_end);

POISMF_HIP_API void poismf_hip_session_destroy(poismf_hip_session *s);

/* The stream this session enqueues its work on (the one given at creation, or the one it created), as void*. */
POISMF_HIP_API void *poismf_hip_session_stream(poismf_hip_session *s);

/* Device pointers to the session-owned, replicated factors: A is [dimA x k], B is [dimB x k],
 * row-major real_t (allocations carry 16 bytes of slack because rows are gathered in 16-byte
 * slots).  The caller may wrap them (e.g. as torch tensors) to run collectives on them.
 * For small k the session also keeps a line-padded copy of each factor for its gathers; a
 * session whose shard is the whole factor refreshes that copy from its own row kernels and
 * must be told about outside writes: call poismf_hip_session_factors_dirty(s, which) (which = 0: B was
 * written, 1: A) after every write through a pointer obtained earlier (calling the getter again or
 * set_factors has the same effect).  Sessions with partial shards re-derive the copy from the compact
 * factor before every half-sweep in any case.
 * A pointer obtained here is DEAD after poismf_hip_session_append_rows / _adopt_new (section 2d) has grown that factor:
 * the grown factor lives in a new allocation.  Call the getter again. */
POISMF_HIP_API real_t *poismf_hip_session_A(poismf_hip_session *s);
POISMF_HIP_API real_t *poismf_hip_session_B(poismf_hip_session *s);
POISMF_HIP_API void poismf_hip_session_factors_dirty(poismf_hip_session *s, int which);

/* Host <-> device copies of the full factors (synchronous with respect to the session stream).
 * get_factors (like run_poismf and poismf_hip_session_run) also returns 1 when a half-sweep since the last check lost a
 * row launch that shares rows between CUs (fp64 CG, 385-2048 nonzeros; the kernels give up after ~1 s without an answer
 * from a team member instead of hanging the device): the factors are then not to be used. */
POISMF_HIP_API int poismf_hip_session_set_factors(poismf_hip_session *s, const real_t *A_host, const real_t *B_host);
POISMF_HIP_API int poismf_hip_session_get_factors(poismf_hip_session *s, real_t *A_host, real_t *B_host);

/* Hyper-parameters of the alternation; same meaning as the run_poismf arguments. */
typedef struct poismf_hip_params {
    real_t l2_reg, l1_reg, w_mult, step_size;
    int method;          /* 1 tncg, 2 cg, 3 pg */
    int limit_step;
    size_t maxupd;
    int early_stop, reuse_prev;
} poismf_hip_params;

/* One half-sweep over this session's shard.  which = 0: update B rows [rowB_begin,rowB_end) against
 * the full A (the reference's first half, ref: src/poismf.c:512-556); which = 1: update A rows against
 * the full B (ref: src/poismf.c:562-603).  The column sums of the opposing factor are recomputed on
 * the device from the replicated copy, so no k-vector collective is needed.  `step_size` is the step
 * of THIS half and `cnst_div` the PG divisor (the caller keeps the reference's step schedule: cnst_div from
 * the step before halving, A half run with the halved step -- quirk Q6; the double scaling of the column
 * sums on the A half -- quirk Q1 -- is applied inside).  If n_unchanged != NULL (TNCG early stop) it receives
 * the number of shard rows whose update moved by <= 1e-4 in squared norm (ref: src/poismf.c:393-396);
 * reading it synchronises the stream.  Asynchronous otherwise.  Returns 0 or 1. */
POISMF_HIP_API int poismf_hip_half_sweep(poismf_hip_session *s, int which, const poismf_hip_params *p,
                          real_t step_size, real_t cnst_div, size_t *n_unchanged);

/* Segments (multi-GPU overlap of the shard exchange with compute).  set_segments cuts the
 * session's shard of half `which` into `nseg` contiguous row ranges of equal row counts (rows begin + n j / nseg ..
 * begin + n (j + 1) / nseg), each sorted and binned on its own, and returns the number of segments (< 0 on error);
 * segment_rows reports a segment's global row range; half_sweep_segment runs ONE segment: segment 0 also computes the
 * column sums and resets the early-stop counter, the call that passes n_unchanged (the last segment) reads it.  Running
 * segments 0 .. nseg-1 in order is bit-identical to one poismf_hip_half_sweep (a row's arithmetic depends on its
 * length class only).  The caller orders its exchange of segment j's rows after that call on the session stream. */
POISMF_HIP_API int poismf_hip_session_set_segments(poismf_hip_session *s, int which, int nseg);
POISMF_HIP_API int poismf_hip_session_segment_rows(poismf_hip_session *s, int which, int seg, size_t *row_begin, size_t *row_end);
POISMF_HIP_API int poismf_hip_half_sweep_segment(poismf_hip_session *s, int which, const poismf_hip_params *p,
                          real_t step_size, real_t cnst_div, int seg, size_t *n_unchanged);

/* ---------------------------------------------------------------------------------------------
 * 2b. Session updates: a user the model knows interacts again.  New counts are merged into the resident CSR and CSC
 *     on the device and the rows they touch are refit, without rebuilding the session.  No counterpart in the reference.
 *
 * poismf_hip_session_add_coo: X += D.  D is HOST COO of the session's shape with n < 2^32 triplets.  Duplicates inside D
 * are summed first (section 1c's conversion and its summation rule); a cell the session already stores then gets ONE rounded
 * addition, a new cell is inserted at its place in the ascending row.  Both orientations are updated, so both halves of
 * the next sweep see the same matrix.  *n_new_cells (may be NULL) receives the number of cells that were not stored
 * before.  n == 0 is a no-op that returns 0.  No resident array comes to the host and nothing is sorted again: per
 * orientation one lane per cell of D finds its place in the resident row (binary search), an exclusive scan over D's
 * cells gives the new row pointers, one pass over the resident entries moves each to its new place (ranges between two
 * touched rows shift by a constant), and one lane per cell of D writes the new cell or adds to the moved entry.
 * Returns 0; 1 out of memory / no device; 3 an index lies outside the matrix; 4 a value is not finite or not > 0 (checked
 * on the host: deletions and decrements are section 2c's); 5 the session is not eligible: either shard is not the whole
 * matrix (or the session has no CSC), or some resident row of either orientation is not strictly ascending
 * (poismf_hip_session_create_coo sessions always qualify, a poismf_hip_session_create session built from unsorted host
 * arrays does not).  3, 4 and 5 are found before anything is written: the session is exactly as it was.
 * Memory: one orientation is merged after the other -- the CSR first -- and each one's new arrays are built beside its
 * resident ones, which are freed when the new ones are complete.  Peak extra device memory is therefore ONE half's arrays,
 * (nnz + new cells) x (4 + sizeof(real_t)) + 8 (dim + 1) bytes, plus O(n + dim) bytes of scratch for D -- not two halves'.
 * A failure (rc 1) while the CSR is merged leaves the session as it was; the price of the bound is that a failure while
 * the CSC is merged, after the CSR has been swapped, cannot be undone: the two orientations then disagree and the session
 * is only good for poismf_hip_session_destroy.
 * Afterwards: poismf_hip_session_nnz is updated, each half is sorted and binned again with the segments it had, "all values
 * positive" is re-derived, and exclude_seen of the batched calls sees the new cells.  The factors, the profiling counters,
 * the guest of the new-rows calls (section 1m) and every scratch area are untouched.
 *
 * poismf_hip_session_get_matrix: half `which`'s matrix to the host (1: the CSR shard, 0: the CSC shard): indptr [rows of the
 * shard + 1] local to the shard (from 0), indices widened to sparse_ix and values, each poismf_hip_session_nnz(s, which)
 * long; a NULL output is skipped.  The only way to see the CSR of a poismf_hip_session_create_coo session.  0 or 1.
 *
 * poismf_hip_half_sweep_rows: poismf_hip_half_sweep over the listed rows of half `which` only.  Every listed row is solved
 * exactly as poismf_hip_half_sweep would solve it from the session's current factors -- the same bits, column sums of the
 * WHOLE fixed factor and PG pre-scaling included (a row's arithmetic depends on its length class only) -- and every
 * unlisted row of the moving factor keeps its bits, in the compact and in the line-padded copy.  `rows` are global row
 * numbers, distinct and inside the shard, in any order: otherwise 3 is returned before any launch (two workgroups updating
 * one row in place would race).  n_rows == 0 returns 0 and launches nothing.  n_unchanged (TNCG early stop) counts the
 * listed rows only.  poismf_hip_session_plan then names this call's launches.  Synchronises the stream.  Returns 0, 1 or 3.
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int poismf_hip_session_add_coo(poismf_hip_session *s, const sparse_ix *row, const sparse_ix *col,
                          const real_t *val, size_t n, size_t *n_new_cells);
POISMF_HIP_API int poismf_hip_session_get_matrix(poismf_hip_session *s, int which,
                          sparse_ix *indptr, sparse_ix *indices, real_t *values);
POISMF_HIP_API int poismf_hip_half_sweep_rows(poismf_hip_session *s, int which, const sparse_ix *rows, size_t n_rows,
                          const poismf_hip_params *p, real_t step_size, real_t cnst_div, size_t *n_unchanged);

/* ---------------------------------------------------------------------------------------------
 * 2c. Session updates: counts are taken back.  An order is cancelled, a like withdrawn, a user asks to be forgotten, an
 *     item is delisted: counts leave the resident CSR and CSC on the device, without rebuilding the session.  The inverse
 *     of section 2b; no counterpart in the reference.
 *
 * poismf_hip_session_sub_coo: X -= D.  D is HOST COO of the session's shape with n < 2^32 triplets.  Triplets repeated
 * inside D are summed first (section 1c's conversion and its summation rule: in input order, so both orientations see the
 * same bits); a cell the session stores then gets ONE rounded subtraction nv = x - d in the model's precision.  The cell
 * is kept with value nv if and only if nv > 0; otherwise it is REMOVED: its entry leaves the row and the row gets shorter.
 * No stored zero or negative value ever results.  val == NULL removes every listed stored cell outright, whatever it
 * holds (a repeated triplet is then harmless).  A listed cell the session does not store is ABSENT: with strict != 0 any
 * absent cell makes the call return 6 before anything is written, with strict == 0 absent cells are skipped and counted
 * in *n_absent.  *n_removed receives the number of cells that left the matrix (either may be NULL).  Both orientations
 * are updated and end with identical cell sets and identical value bits: "removed" is decided from the same x and d bits
 * in both.  n == 0 returns 0 and launches nothing.
 * Per orientation: one lane per cell of D finds its place in the resident row (2b's search) and decides gone = !(nv > 0);
 * an exclusive scan of `gone` over D's cells gives the new row pointers; ONE pass over the resident entries moves each
 * survivor left to its new place and drops the gone ones (ranges between two touched rows shift by a constant; inside
 * a touched row an entry moves by the gone positions before it, a binary search); then one lane per surviving hit writes
 * nv over the moved entry.  No resident array comes to the host and nothing is sorted again.
 *
 * poismf_hip_session_remove_rows: every stored cell of the listed rows of half `which` (1: users, rows of the CSR; 0: items)
 * is removed -- from that orientation AND from the other one.  `rows` are global, distinct, inside the matrix, in any order.
 * The cell list is built on the device from the resident rows themselves (the listed rows' ranges expanded into (major,
 * minor) triplets; only their total count comes to the host) and goes through the core of sub_coo(val = NULL).  The rows
 * stay in the matrix with length 0: the dimensions never change and the factor rows are untouched.  n_rows == 0 returns 0
 * and launches nothing.  *n_removed (may be NULL) receives the number of cells removed.
 *
 * Returns 0; 1 out of memory / no device / n >= 2^32; 3 an index lies outside the matrix (remove_rows: or a row is listed
 * twice); 4 val is given and some value is not finite or not > 0; 5 the session is not eligible (2b's rule: either shard
 * is not the whole matrix, no CSC, or a resident row that is not strictly ascending); 6 strict was set and a cell is
 * absent.  3, 4, 5 and 6 are found before anything is written: the session is exactly as it was.
 * Memory and failure are 2b's: the CSR is done first, then the CSC; each orientation's new arrays are built beside the
 * resident ones and swapped in when complete, so peak extra device memory is one half's arrays plus O(n + dim) scratch;
 * a failure (rc 1) after the CSR has been swapped leaves the orientations in disagreement and the session only good for
 * poismf_hip_session_destroy.
 * Afterwards: poismf_hip_session_nnz is updated, each half is sorted and binned again with the segments it had, and
 * exclude_seen of the batched calls, poismf_hip_session_llk, the new-rows calls and the half-sweeps no longer see the
 * cells.  A matrix emptied to nnz == 0 is legal and a later poismf_hip_session_add_coo works on it.  The factors are
 * untouched (refit the touched rows with poismf_hip_half_sweep_rows).
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int poismf_hip_session_sub_coo(poismf_hip_session *s, const sparse_ix *row, const sparse_ix *col,
                          const real_t *val, size_t n, int strict, size_t *n_removed, size_t *n_absent);
POISMF_HIP_API int poismf_hip_session_remove_rows(poismf_hip_session *s, int which, const sparse_ix *rows, size_t n_rows,
                          size_t *n_removed);

/* ---------------------------------------------------------------------------------------------
 * 2d. Session updates: the matrix grows.  A user signs up, an item is listed: new rows join the resident CSR / CSC and
 *     the resident factors on the device, without rebuilding the session.  No counterpart in the reference.
 *
 * poismf_hip_session_append_rows: which = 1 appends n_new users (rows of A and of the CSR; dimA becomes dimA + n_new),
 * which = 0 appends n_new items (rows of B and of the CSC; dimB grows).  The new rows take the numbers old dim .. old dim
 * + n_new - 1; *first_row (may be NULL) receives old dim.  F is HOST [n_new x k], the new rows of the grown factor, or NULL:
 * zero rows.  The new rows' cells are HOST CS rows over the OTHER dimension: indptr [n_new + 1] (from any start, never
 * decreasing), indices below the other dimension and strictly ascending within a row, values finite and > 0 -- neither
 * is repaired; indptr == NULL: the rows are empty.  Both orientations receive the cells: the grown one as new rows at
 * its end, the other one as entries at the end of each touched row (their index exceeds every stored one).  Afterwards
 * the session is bit for bit the one poismf_hip_session_create_coo builds from the grown matrix at the grown dimensions
 * followed by set_factors([old; F], other): both matrices, poismf_hip_session_nnz, "all values positive", the segments each
 * half had, the plan and the results of every later half-sweep, likelihood, serving and new-rows call.  n_new == 0 returns 0
 * and does nothing.
 * The growth: ONE kernel builds the grown factor -- its compact copy and, where the session keeps one, its line-padded copy,
 * pad columns, the all-zero row and the slack behind it included -- in one pass over the old compact factor; the grown
 * orientation's row pointers are the old ones followed by nnz; its permutation and descriptors are sized anew; the per-row
 * counters of a profiling session keep the old rows' values and are zero for the new rows.  The other orientation's
 * arrays are untouched by the growth.  The cells then go through section 2b's merge as device triplets, the CSR first, and
 * each half is sorted and binned again with the segments it had.  exclude_seen of the batched calls sees the new rows; column-sum
 * partials of the grown factor (poismf_hip_session_partials_ready) are dropped; the guest of the new-rows calls (section
 * 1m) follows a grown B and keeps its own rows and factors.  The scratch of the likelihood, of the batched calls and the
 * team launches' row backup are sized by the call that uses them and need nothing.
 * Returns 0; 1 out of memory, a device error, a grown dimension > 0x7fffffff or n >= 2^32 cells; 3 an index outside the
 * other dimension, a row that is not strictly ascending, or decreasing pointers; 4 a value that is not finite or not > 0;
 * 5 the session is not eligible (2b's rule).  3, 4 and 5 are found on the host before anything is written: the session is
 * exactly as it was.
 * Memory and failure: the growth allocates all its new arrays beside the old ones -- the grown factor (and its padded copy)
 * and the grown half's row pointers, so peak extra device memory is one factor in both copies plus 8 (dim + 1) bytes -- and
 * swaps them in only when all exist: a failure (rc 1) of the growth leaves the session as it was.  The cell merge behind it
 * is 2b's, with 2b's bound (one half's arrays) and 2b's price: a failure while the CSR is merged leaves the grown session
 * with its new rows empty, a failure while the CSC is merged leaves the orientations in disagreement and the session
 * only good for poismf_hip_session_destroy.
 * Pointers obtained earlier from poismf_hip_session_A (which = 1) / poismf_hip_session_B (which = 0) are DEAD after the call.
 *
 * poismf_hip_session_adopt_new: the rows the session's guest holds from the last section 1m call (factors_new, topn_new,
 * rank_new) become resident users -- their CSR and their solved factors: append_rows(1, ...) with everything taken from
 * the device.  The factor rows are read from the guest's factor, the cells are expanded from the guest's CSR into triplets;
 * nothing crosses PCIe except the rows' counts.  *first_row / *n_rows (may be NULL) receive the first new user and how many
 * there are.  Returns as append_rows, and 5 when there is no guest or a guest row is not strictly ascending, 4 when the
 * guest's rows hold a value that is not > 0.  The guest is left as it was.  The result is bit for bit append_rows(1, the
 * same rows, F = what poismf_hip_session_factors_new returned).
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int poismf_hip_session_append_rows(poismf_hip_session *s, int which, size_t n_new,
                          const real_t *F, const real_t *val, const sparse_ix *indptr, const sparse_ix *indices,
                          size_t *first_row);
POISMF_HIP_API int poismf_hip_session_adopt_new(poismf_hip_session *s, size_t *first_row, size_t *n_rows);

/* ---------------------------------------------------------------------------------------------
 * 2e. Session updates: counts fade.  Time decay makes last month's plays count for less than last week's: every stored
 *     count is scaled on the device, in both orientations, and what fades below a floor leaves the matrix, without
 *     rebuilding the session.  Unlike 2b-2d it is not driven by a cell list: it touches every entry.  No counterpart in
 *     the reference.
 *
 * poismf_hip_session_scale: for every stored cell (u, i) with value x, nv = ((x * gamma) * row_scale[u]) * col_scale[i]:
 * three multiplications in the model's precision, in this order, each rounded once.  row_scale is HOST [dimA], col_scale
 * HOST [dimB]; either may be NULL: all ones (multiplying a finite value by 1 is exact, so an absent operand may be skipped:
 * the bits are those of the formula).  Both orientations compute the same nv bits from the same operands.  The cell stays
 * with value nv if and only if nv > floor; otherwise it is REMOVED: its entry leaves the row and the row gets shorter
 * (section 2c's rule is the case floor == 0).  No zero, negative or non-finite value is ever stored; a subnormal nv is a
 * value like any other and is not flushed.  *n_removed (may be NULL) receives the number of cells that left.  Rows stay,
 * possibly with length 0: the dimensions never change and the factors are untouched (every row has changed: refit with
 * poismf_hip_half_sweep).  A scale of 0 on a row or column is poismf_hip_session_remove_rows on it.  A matrix emptied to
 * nnz == 0 is legal and a later poismf_hip_session_add_coo works on it.  nnz == 0 returns 0 and launches nothing; so does
 * gamma == 1 with both vectors NULL and floor == 0.
 * Per orientation, over chunks of consecutive resident entries, a workgroup per chunk, so that a row of millions of entries
 * is cut over many workgroups like any other range: a DECIDE pass reads the values (the indices only when the vector over
 * them is given; the row of an entry, when the vector over the rows is given, is found from the chunk's slice of the row
 * pointers: one search per chunk, none over the whole dimension per entry) and writes a keep bit per entry, a kept count
 * per chunk and the number of results that are not finite; an exclusive scan over the chunk counts and one lane per row
 * (the chunk's base plus the keep bits of the chunk before the row's first entry) give the new row pointers; a COMPACT pass
 * computes every survivor's nv again from the same operands and stores it with its index at its new place, survivors in
 * their order, so rows stay strictly ascending.  When NO cell leaves -- the common case, floor == 0 and scales in (0, 1] --
 * an IN-PLACE pass rewrites the values only: row pointers, indices, the sort permutation, the bins, the segments and the
 * row pointers exclude_seen keeps are untouched.  No resident array comes to the host; only the two vectors go up and only
 * counts come down.
 * Returns 0; 1 out of memory / a device error; 4 gamma, floor or an entry of a vector is not finite or is < 0 (checked on
 * the host); 5 the session is not eligible (2b's rule: either shard is not the whole matrix, no CSC, or a resident row
 * that is not strictly ascending); 7 some nv is not finite (a scale above 1 overflowed): found by the CSR's decide pass
 * before anything resident is written.  After 4, 5 and 7 the session is exactly as it was.
 * Memory and failure are 2b's and 2c's: the CSR is done first, then the CSC; when cells leave, each orientation's new
 * arrays are built beside the resident ones and swapped in when complete, so peak extra device memory is one half's
 * arrays plus O(nnz / 8 + dim) bytes of scratch; a failure (rc 1) after the CSR has been written leaves the orientations in
 * disagreement and the session only good for poismf_hip_session_destroy.  The count of leaving cells and of non-finite
 * results is the CSR's; a CSC pass that finds another returns 1.
 * Afterwards, when cells left: poismf_hip_session_nnz is updated, each half is sorted and binned again with the segments
 * it had, and exclude_seen of the batched calls, poismf_hip_session_llk, the new-rows calls and the half-sweeps no longer
 * see the cells.  Either way "all values positive" holds.
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int poismf_hip_session_scale(poismf_hip_session *s, real_t gamma,
                          const real_t *row_scale, const real_t *col_scale, real_t floor, size_t *n_removed);

/* run_poismf's outer loop (ref: src/poismf.c:506-608: B half, PG step halving, A half, TNCG early stop, SIGINT
 * handling and return codes 0 / 1 / 2 exactly as in section 1) on a session that already holds X and the starting
 * factors; `p->step_size` is the initial step.  PoisMF.fit uses it with poismf_hip_session_create_coo so that the
 * converted CSR / CSC never leave the device. */
POISMF_HIP_API int poismf_hip_session_run(poismf_hip_session *s, const poismf_hip_params *p, size_t numiter, int handle_interrupt);

/* Wall-clock (HIP events on the session stream) of the row-update kernels launched by half-sweeps
 * since profiling was switched on: total milliseconds and number of kernel launches, per half.
 * Synchronises the stream. */
POISMF_HIP_API void poismf_hip_session_profile(poismf_hip_session *s, int enable);
POISMF_HIP_API int poismf_hip_session_kernel_time(poismf_hip_session *s, int which, double *total_ms, size_t *launches);

/* While profiling is enabled the row kernels also count, per half (which = 0: B, 1: A) and since the last
 * poismf_hip_session_profile() call, the passes they made over rows' gathered tiles (one per gradient / function
 * evaluation of the inner solver, ref src/poismf.c:126-133, :194-273) and the sum over rows of passes x nonzeros --
 * SURVEY.md 8(d)'s pass-weighted effective traffic is nnz_passes * k * sizeof(real_t). */
POISMF_HIP_API int poismf_hip_session_eval_stats(poismf_hip_session *s, int which, unsigned long long *tile_passes, unsigned long long *nnz_passes);

/* Diagnostic: the kernels take log() of the predictions in double (as the reference's C does even in its float build,
 * ref src/poismf.c:199, :268) with their own implementation of the fdlibm algorithm instead of the device library's.
 * This runs both on n sample arguments on the current device and reports the largest distance in ulps and the number
 * of special arguments (+-0, -1, +-inf, NaN) on which they disagree.  Returns 0 on success. */
POISMF_HIP_API int poismf_hip_selftest_log(size_t n, unsigned long long *worst_ulp, unsigned *mismatched_specials);

/* Serving from the session's resident factors: the same results as predict_multiple
 * (ref: src/pred.c:42-64) and as topN with a_vec = row `user` of A (ref: src/topN.c:112-284), without the per-call copy
 * of the factors that the host-pointer drop-ins of section 1d make.  Index arrays are host arrays.  Return 0, 1 (device
 * error / out of memory) or 2 (an index out of range, or topN's invalid combinations, ref src/topN.c:126-130). */
POISMF_HIP_API int poismf_hip_session_predict(poismf_hip_session *s, const sparse_ix *ixA, const sparse_ix *ixB, size_t n, real_t *out);
POISMF_HIP_API int poismf_hip_session_topn(poismf_hip_session *s, size_t user,
                          const sparse_ix *include_ix, size_t n_include, const sparse_ix *exclude_ix, size_t n_exclude,
                          sparse_ix *outp_ix, real_t *outp_score, size_t n_top);

/* Section 1f from the session-resident factors (and, with exclude_seen, the session's own CSR rows).  Ordered after the work already
 * enqueued on the session stream; reads the compact factors, as poismf_hip_session_llk does. */
POISMF_HIP_API int poismf_hip_session_topn_batch(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        int exclude_seen, const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);

/* Section 1l from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_topn_deep(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        int exclude_seen, const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);

/* Section 1n from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_topn_quota(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *group_of, size_t n_groups, const sparse_ix *quota,
        int exclude_seen, const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);

/* Section 1o from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above.
 * query_B != 0: `users` index rows of the resident B (checked against dimB) -- those rows are the queries and B is also the corpus,
 * the item-to-item call.  exclude_seen together with query_B returns 2. */
POISMF_HIP_API int poismf_hip_session_topn_weighted(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        const real_t *item_weight, int query_B, int exclude_seen,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);

/* Section 1r from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_topn_adjusted(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *adj_indptr, const sparse_ix *adj_indices, const real_t *adj_factor,
        int exclude_seen, const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);

/* Section 1p from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_topn_diverse(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        size_t pool, double lambda, const real_t *item_inv_norm, int exclude_seen,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score, real_t *out_value);

/* Section 1q against the session-resident B, ordered as the call above and in the same scratch: no factor is uploaded. */
POISMF_HIP_API int poismf_hip_session_list_eval(poismf_hip_session *s, const sparse_ix *lists, size_t n_users, size_t n_list,
        const real_t *item_inv_norm,
        const sparse_ix *test_indptr, const sparse_ix *test_indices, size_t budget_bytes,
        unsigned int *out_pos, long long *out_cos, unsigned int *out_len, unsigned int *exposure);

/* Section 1h from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_topn_include(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *incl_indptr, const sparse_ix *incl_indices,
        int exclude_seen, const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);

/* Section 1i from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_topn_shared(poismf_hip_session *s, const sparse_ix *users, size_t n_users, size_t n_top,
        const sparse_ix *list_indptr, const sparse_ix *list_indices, size_t n_lists, const sparse_ix *list_of,
        int exclude_seen, const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score);

/* Section 1g from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_rank_batch(poismf_hip_session *s, const sparse_ix *users, size_t n_users,
        const sparse_ix *test_indptr, const sparse_ix *test_indices, int exclude_seen,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        unsigned int *out_rank, unsigned int *out_n_adm);

/* Section 1j from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_rank_include(poismf_hip_session *s, const sparse_ix *users, size_t n_users,
        const sparse_ix *test_indptr, const sparse_ix *test_indices,
        const sparse_ix *incl_indptr, const sparse_ix *incl_indices, int exclude_seen,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        unsigned int *out_rank, unsigned int *out_n_adm);

/* Section 1k from the session-resident factors (and, with exclude_seen, the session's own CSR rows), ordered as the call above. */
POISMF_HIP_API int poismf_hip_session_rank_shared(poismf_hip_session *s, const sparse_ix *users, size_t n_users,
        const sparse_ix *test_indptr, const sparse_ix *test_indices,
        const sparse_ix *list_indptr, const sparse_ix *list_indices, size_t n_lists, const sparse_ix *list_of,
        int unite_test, int exclude_seen,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        unsigned int *out_rank, unsigned int *out_n_adm);

/* ---------------------------------------------------------------------------------------------
 * 1m. New rows against a resident B: the factors of users the model has never seen (the reference's predict_factors, ref:
 *     poismf/__init__.py:619-692), and their top-N (its topN_new) and exact ranks, without B travelling per request.  (Placed
 *     here, after the session's types, which three of the four entries take.)
 *
 * The n_new rows are a host CSR (Xr, Xr_indptr [n_new + 1], Xr_indices; item indices < dimB), as factors_multiple takes them.
 * They become a GUEST of the session: their CSR and an n_new x k factor of their own are kept on the device next to the
 * session's B, which the guest borrows (with its line-padded gather copy, refreshed for the session if it was stale).  The
 * guest is kept by the session and reused by the next call; nothing of it outlives the session.  A call allocates, uploads
 * and copies nothing in proportion to dimB x k, writes nothing to the session's A, B or matrix, and is ordered after the work
 * already enqueued on the session stream.
 *
 *   factors      bit for bit those of factors_multiple (section 1b) with the same B, Bsum, Amean, rows and solver arguments: the
 *                same half-sweep of the same row kernels under the same plan.  Of *p: l2_reg, w_mult, step_size, method,
 *                limit_step and maxupd mean what they mean there; reuse_prev is its reuse_mean; l1_reg and early_stop are
 *                ignored (Bsum [k] already carries l1).  Rows start at Amean [k], broadcast on the device (TNCG without
 *                reuse_prev: at 1e-3, set by the kernel).  An empty row's factors are zero; a call whose rows are all empty
 *                gives zeros without a launch (quirk Q7).
 *   top-N        section 1f's answer(u) for A = the new factors: the same total order, and score bits those of predict_multiple
 *                on these factors.  E(u) is the union of (a) with exclude_own the items of new row u itself, read from the
 *                guest's CSR on the device, nothing staged a second time -- a row that is not strictly ascending is treated as
 *                exclude_seen treats such a resident row: the rows are then scanned, not binary-searched, and an item named
 *                twice counts once -- and (b) the optional list excl_indptr [n_new + 1] / excl_indices of section 1f.
 *   ranks        section 1g's rank(u, t) and N(u) for the same factors and the same E(u).
 *   out_A        [n_new x k], host: the new factors.  Required by poismf_hip_session_factors_new; NULL elsewhere means the
 *                factors never leave the device.
 *
 * Return 0; 1 on a device error / out of memory; 2, with no output touched and before any device work, when: the session, p,
 * Bsum, Amean, Xr_indptr or a required output is NULL; row pointers decrease; an item index >= dimB; Xr or Xr_indices NULL
 * with a nonzero stored; and whatever is 2 in section 1f (top-N) or 1g (ranks) for users 0 .. n_new-1 -- "too few items
 * left" counts the union of the row's own items (with exclude_own) and its exclusion row.  n_new == 0 returns 0.
 *
 * poismf_hip_topn_new is the host-pointer drop-in: B [dimB x k] goes up once, to the device of POISMF_HIP_DEVICE, into a
 * temporary session; the same core runs and everything is freed before it returns.  Its solver arguments are
 * factors_multiple's, in that order.
 * ------------------------------------------------------------------------------------------- */
POISMF_HIP_API int poismf_hip_session_factors_new(poismf_hip_session *s, const real_t *Xr, const sparse_ix *Xr_indptr,
        const sparse_ix *Xr_indices, size_t n_new, const real_t *Bsum, const real_t *Amean,
        const poismf_hip_params *p, size_t niter, real_t *out_A);
POISMF_HIP_API int poismf_hip_session_topn_new(poismf_hip_session *s, const real_t *Xr, const sparse_ix *Xr_indptr,
        const sparse_ix *Xr_indices, size_t n_new, const real_t *Bsum, const real_t *Amean,
        const poismf_hip_params *p, size_t niter, size_t n_top, int exclude_own,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score, real_t *out_A);
POISMF_HIP_API int poismf_hip_session_rank_new(poismf_hip_session *s, const real_t *Xr, const sparse_ix *Xr_indptr,
        const sparse_ix *Xr_indices, size_t n_new, const real_t *Bsum, const real_t *Amean,
        const poismf_hip_params *p, size_t niter,
        const sparse_ix *test_indptr, const sparse_ix *test_indices, int exclude_own,
        const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        unsigned int *out_rank, unsigned int *out_n_adm, real_t *out_A);
POISMF_HIP_API int poismf_hip_topn_new(const real_t *B, const real_t *Bsum, const real_t *Amean,
        const real_t *Xr, const sparse_ix *Xr_indptr, const sparse_ix *Xr_indices,
        int k, size_t dimB, size_t n_new,
        real_t l2_reg, real_t w_mult, real_t step_size, size_t niter, size_t maxupd,
        int method, bool limit_step, bool reuse_mean,
        size_t n_top, int exclude_own, const sparse_ix *excl_indptr, const sparse_ix *excl_indices,
        sparse_ix *out_ix, real_t *out_score, real_t *out_A);

/* The log-likelihood of section 1e for the session's resident CSR shard (rows [rowA_begin,rowA_end) of A) under its resident
 * factors; with include_missing, M covers the shard's rows of A times all of B.  No factor or matrix is copied: one double
 * comes back in *out.  Ordered after the work already enqueued on the session stream; reads the compact factors, so writes
 * through poismf_hip_session_A/B are seen whether or not factors_dirty was called yet.  On a single-GPU session the result has
 * the same bits as eval_llk on the same matrix and factors.  Returns 0, or 1 on a device error. */
POISMF_HIP_API int poismf_hip_session_llk(poismf_hip_session *s, int full_llk, int include_missing, double *out);

/* Which row-kernel instances the most recent half-sweep of half `which` launched, as text ("kernel<instance> rows=N;"
 * per launch), NUL-terminated and truncated to cap bytes; returns the untruncated length.  Reporting only. */
POISMF_HIP_API size_t poismf_hip_session_plan(poismf_hip_session *s, int which, char *buf, size_t cap);

/* Profiling sessions (poismf_hip_session_profile(s, 1)) also bracket every row-bin launch with events on the stream it
 * is issued on.  This returns, for half `which`, "kernel<instance> rows=R nnz=Z calls=C ms=T;" per distinct launch since
 * profiling was switched on (T = summed milliseconds over the C calls; Z = nonzeros of the rows the launch covers, i.e.
 * what its algorithmic bytes are computed from).  Same buffer convention as poismf_hip_session_plan.  Reporting only. */
POISMF_HIP_API size_t poismf_hip_session_launch_profile(poismf_hip_session *s, int which, char *buf, size_t cap);

/* Profiling sessions also record what every row's inner solver decided in the most recent half-sweep of half `which`:
 * out[2 r] = iterations | rc << 24, out[2 r + 1] = evaluations, for local row r -- the numbers the reference's
 * minimize_nonneg_cg (niter, nfeval; ref src/nonnegcg.c:177-189) and tnc (nfeval, niter, rc; ref src/tnc.c:251-260) return and
 * cg_iteration / tncg_iteration discard.  Testing aid: pins the solvers' decisions, not only their results. */
POISMF_HIP_API int poismf_hip_session_decisions(poismf_hip_session *s, int which, unsigned *out, size_t nrows);
/* The same, summed over the rows of the shard: out[0] = sum of iterations, out[1] = sum of evaluations, out[2] = sum of
 * nnz x iterations, out[3] = sum of nnz x evaluations -- what a flop count of the reference's arithmetic for the same decisions
 * needs (a gradient is 4k+1 flops per nonzero, a function value 2k+L; ref src/poismf.c:126-133, :194-208).
 * Returns 1 when the session is not profiling. */
POISMF_HIP_API int poismf_hip_session_decision_stats(poismf_hip_session *s, int which, unsigned long long *out);
/* factors_multiple (below / ref src/pred.c:66-199) that also returns those two words per row. */
POISMF_HIP_API int poismf_hip_factors_multiple_decisions(real_t *A, real_t *B, real_t *Bsum, real_t *Amean, real_t *Xr,
                          sparse_ix *Xr_indptr, sparse_ix *Xr_indices, int k, size_t dimA, real_t l2_reg, real_t w_mult,
                          real_t step_size, size_t niter, size_t maxupd, int method, bool limit_step, bool reuse_mean,
                          unsigned *decisions);

/* The first stage of a half-sweep's column sums, shared between the ranks of a multi-GPU run (the sum itself: ref
 * src/poismf.c:77-83).  The sum over the FIXED factor of half `which` (A for which = 0, B for which = 1) is cut into
 * poismf_hip_session_colsum_blocks() blocks whose partial sums depend on the block number alone: a rank computes blocks [b_lo, b_hi) into
 * the session's partial array (poismf_hip_session_partials: [blocks x k] real_t in device memory), receives the others from its peers
 * into the same array, and declares it complete (poismf_hip_session_partials_ready): the next half-sweep (or its segment 0) then runs
 * only the fixed-order second stage.  Bit for bit the unsharded sum. */
POISMF_HIP_API int poismf_hip_session_colsum_blocks(poismf_hip_session *s, int which);
POISMF_HIP_API int poismf_hip_session_colsum_partial(poismf_hip_session *s, int which, int b_lo, int b_hi);
POISMF_HIP_API real_t *poismf_hip_session_partials(poismf_hip_session *s);
POISMF_HIP_API void poismf_hip_session_partials_ready(poismf_hip_session *s);

/* Nothing survives run_poismf by default: every device array the call allocated is freed before it returns, as the reference frees
 * its scratch (ref src/poismf.c:610-619).  A caller that fits repeatedly on matrices of one shape can OPT IN to keeping released
 * device arrays of 1 MB and more for the next request of the same size on the same device (repeated fits then allocate nothing and
 * their uploads run over two DMA queues at full rate): environment POISMF_HIP_DEVICE_CACHE_MB=<MB> or
 * poismf_hip_set_device_cache_mb(MB) at run time (returns the previous limit; lowering it frees what no longer fits; the limit is
 * per loaded flavour of the library).  poismf_hip_release_cache() hands whatever is kept back to the driver. */
POISMF_HIP_API void poismf_hip_release_cache(void);
POISMF_HIP_API size_t poismf_hip_set_device_cache_mb(size_t mb);

/* Testing aid (G1): the device's own objective / gradient wrappers at `point`, for every row of a CSR, through whichever row engine a CG
 * half-sweep would use for a row of that length.  which = 0: calc_fun_single + calc_grad_single[_w] (ref src/poismf.c:194-240);
 * which = 1: calc_fun_and_grad (ref src/poismf.c:242-273; no l2 term in f).  G [dimA x k] receives the gradients, f [dimA] the values. */
POISMF_HIP_API int poismf_hip_debug_row_eval(real_t *G, double *f, real_t *B, real_t *Bsum, real_t *point, real_t *Xr,
                          sparse_ix *Xr_indptr, sparse_ix *Xr_indices, int k, size_t dimA, real_t l2_reg, real_t w_mult, int which);

/* Testing aid: the planner alone, without a device (no HIP call is made).  A half of `nrows` rows with row_nnz[r] nonzeros each, gathering from a
 * factor of dimF rows, is cut into nseg segments as poismf_hip_session_set_segments cuts it, each segment's rows sorted by length (longest
 * first) and binned; buf receives the plan of one half-sweep call over segment `seg` (seg < 0: over all segments, as poismf_hip_half_sweep
 * runs them) on a device of num_cu compute units, worded as poismf_hip_session_plan words it and in launch order.  method, maxupd, w_mult,
 * limit_step: as in poismf_hip_params.  Same buffer convention as poismf_hip_session_plan. */
POISMF_HIP_API size_t poismf_hip_debug_plan(const unsigned *row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method,
                          size_t maxupd, real_t w_mult, int limit_step, int num_cu, char *buf, size_t cap);
/* The same plan; a lane launch whose instance is specialised on the used width of its factor rows (fp32 PG at k = 50: 50 elements of the 13
 * slots' 52) carries "[KU=<width>]" behind its name. */
POISMF_HIP_API size_t poismf_hip_debug_plan_widths(const unsigned *row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method,
                          size_t maxupd, real_t w_mult, int limit_step, int num_cu, char *buf, size_t cap);

/* The listing of poismf_hip_debug_plan_widths with the engine of the one-wave register launches marked as well: "[quad]" behind the name of a launch
 * that holds each nonzero in four lanes instead of sixteen (PG on floats, k = 50, the line-padded factor copy; poismf_hip_debug_reg_quad_off). */
POISMF_HIP_API size_t poismf_hip_debug_plan_engines(const unsigned *row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method,
                          size_t maxupd, real_t w_mult, int limit_step, int num_cu, char *buf, size_t cap);
/* Of the listing of poismf_hip_debug_plan_engines, only the launches for which the solver's row-kernel translation unit has no instance: what
 * the dispatcher itself answers when it is asked to find each planned launch's kernel without launching it (no HIP call is made).  Empty unless
 * the planner names an instance that was never compiled -- such a launch would fail at run time. */
POISMF_HIP_API size_t poismf_hip_debug_plan_missing(const unsigned *row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method,
                          size_t maxupd, real_t w_mult, int limit_step, int num_cu, char *buf, size_t cap);
/* Testing aid: full != 0 -- the lane launches this process plans from now on take the instances that carry every element of their slots, also
 * where one specialised on the used width exists (the two agree bit for bit; a -DPMF_LANE_KU50=0 build never selects the latter); 0 -- the
 * default again.  Returns the previous setting. */
POISMF_HIP_API int poismf_hip_debug_lane_full_width(int full);

/* Testing aid: off != 0 -- the one-wave register launches this process plans from now on take the sixteen-lane engine also where the quad engine
 * exists (PG on floats, k = 50, the line-padded factor copy: four lanes per nonzero, marked "[quad]" by poismf_hip_debug_plan_engines; a
 * -DPMF_REG_QUAD=0 build never selects it); 0 -- the default again.  Returns the previous setting. */
POISMF_HIP_API int poismf_hip_debug_reg_quad_off(int off);

/* Number of nonzeros held by this session for half `which` (shard only). */
POISMF_HIP_API size_t poismf_hip_session_nnz(poismf_hip_session *s, int which);

#ifdef __cplusplus
}
#endif
#endif /* POISMF_HIP_H */
