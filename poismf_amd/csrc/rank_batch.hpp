// rank_batch.hpp -- what the session (poismf_hip_host.hip) hands to the batched-rank core (rank_batch.hip)
#pragma once
#include "topn_batch.hpp"

int poismf_hip_rank_batch_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                const sparse_ix* test_indices, const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_rank_batch_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices,
                              PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch,
                              size_t* scratch_cap, unsigned int* out_rank, unsigned int* out_n_adm);
