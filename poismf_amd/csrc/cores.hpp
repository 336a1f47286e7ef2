// cores.hpp -- the C++ cores that one translation unit defines and another calls, declared once: included by the unit that defines
// each function and by every caller.
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"

// serve.hip (cores on device-resident factors)
int poismf_hip_serve_predict(const real_t* dA, const real_t* dB, const sparse_ix* ixA, const sparse_ix* ixB, size_t n, int k, real_t* out,
                             size_t* max_a, size_t* max_b);
int poismf_hip_serve_topn(const real_t* d_a, const real_t* dB, int k, const sparse_ix* include_ix, size_t n_include,
                          const sparse_ix* exclude_ix, size_t n_exclude, sparse_ix* outp_ix, real_t* outp_score, size_t n_top, size_t n);
int poismf_hip_serve_topn_check(const sparse_ix*& include_ix, size_t n_include, const sparse_ix*& exclude_ix, size_t n_exclude, size_t n_top, size_t n);
// llk.hip (the likelihood on device-resident data)
size_t poismf_hip_llk_scratch(size_t nrows, size_t dimB, size_t k, size_t nnz);
int poismf_hip_llk_enqueue(const real_t* A, const real_t* B, size_t nrows, size_t dimB, size_t k, const unsigned long long* indptr,
                           const unsigned* col, const real_t* val, size_t nnz, int full_llk, int include_missing, double* scratch,
                           hipStream_t stream);
// list_eval.hip (section 1q): the argument checks of both entry points (0, or 2; no device call) and the core on a device-resident B
// (arguments already checked; *d_scratch / *scratch_cap: the caller's scratch, grown when it is smaller than the call needs; 0 or 1)
int poismf_hip_list_eval_check(const sparse_ix* lists, size_t n_users, size_t n_list, size_t dimB, size_t k, const real_t* item_inv_norm,
                               const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t budget_bytes, const unsigned int* out_pos,
                               const long long* out_cos, const unsigned int* out_len, const unsigned int* exposure);
int poismf_hip_list_eval_run(hipStream_t stream, const real_t* dB, size_t dimB, size_t k, const sparse_ix* lists, size_t n_users, size_t n_list,
                             const real_t* item_inv_norm, const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t budget_bytes,
                             void** d_scratch, size_t* scratch_cap, unsigned int* out_pos, long long* out_cos, unsigned int* out_len,
                             unsigned int* exposure);
// coo_convert.hip (rocPRIM-based helpers)
int poismf_hip_device_sort_rows(const unsigned long long* d_indptr, size_t nloc, unsigned base, unsigned* d_perm, unsigned* d_len_sorted,
                                hipStream_t stream);
int poismf_hip_device_narrow(const unsigned long long* d_src, size_t n, unsigned* d_dst, hipStream_t stream);
int poismf_hip_device_coo_to_cs(const unsigned* d_major, const unsigned* d_minor, const real_t* d_val, size_t n, size_t major_begin,
                                size_t major_end, unsigned* out_minor, real_t* out_val, unsigned long long* out_indptr,
                                size_t* nnz_out, hipStream_t stream);
