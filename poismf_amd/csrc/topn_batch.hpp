// topn_batch.hpp -- what the session (poismf_hip_host.hip) hands to the batched top-N core (topn_batch.hip)
#pragma once
#include <cstddef>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"

// exclude_seen: the session's resident CSR shard, and what the session remembers about it between calls
struct PmfTopnSeen {
    const unsigned long long* d_indptr;          // [row_end - row_begin + 1], from 0
    const unsigned* d_indices;
    size_t row_begin, row_end;                   // the shard's rows of A
    std::vector<unsigned long long>* h_indptr;   // host copy of d_indptr (empty until the first call needs it)
    int* sorted;                                 // -1 not checked yet, 0 some row is not strictly ascending, 1 all are
};

int poismf_hip_topn_seen_sorted(PmfTopnSeen& seen, hipStream_t stream);
int poismf_hip_topn_batch_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_topn_batch_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, size_t n_top, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                              const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score);
