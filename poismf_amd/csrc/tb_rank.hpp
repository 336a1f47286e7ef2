// tb_rank.hpp -- what the batched ranks over the whole catalogue (rank_batch.hip, section 1g) and over per-user include lists
// (rank_include.hip, section 1j) have in common: the arguments of a chunk, the scalar score chain, the search in a user's ordered
// thresholds, and the three passes around the counting kernel of either --
//   rank_threshold_kernel  one thread per held-out cell: its score with the scalar chain (the "threshold"), and whether the cell leaves
//                          the ranking: its item is in E(u) or (INCL) not in the user's ascending include row, by binary search.
//   rank_order_kernel      one thread per cell: its position among the user's cells (valid ones best first under the total order, the
//                          others behind them), by counting -- quadratic in a row's length, hence POISMF_HIP_RANK_BATCH_MAX_ROW.
//   rank_finish_kernel     one thread per user: the rank of each valid cell from its counter and the running sum of the difference
//                          array, written at the cell's place in the caller's order; POISMF_HIP_RANK_EXCLUDED for the others.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"
#include "tb_tile.hpp"

namespace {

constexpr size_t RB_ROW_MAX = POISMF_HIP_RANK_BATCH_MAX_ROW;
constexpr unsigned RB_EXCLUDED = POISMF_HIP_RANK_EXCLUDED;

struct RbArgs {
    const real_t* A;                  // rows addressed by `arow`
    const real_t* B;                  // [dimB x k]
    int k;
    unsigned dimB, n_users, n_cells;
    const unsigned* arow;             // [n_users] the chunk's rows of A
    const unsigned* tptr;             // [n_users + 1] the chunk's held-out rows, from 0
    const unsigned* cell_row;         // [n_cells] chunk user of a cell
    const unsigned* cell_item;        // [n_cells]
    real_t* cell_score;               // [n_cells] thresholds in the caller's order
    unsigned* cell_excl;              // [n_cells] 1: the cell leaves the ranking (its item is in E(u), or not in I(u))
    real_t* s_score;                  // [n_cells] per user: valid thresholds best first, then the other cells
    unsigned* s_item;
    unsigned* s_origin;               // the cell an ordered entry came from
    unsigned* nvalid;                 // [n_users] cells that stay in the ranking
    unsigned* dense;                  // [n_cells] (ordered) candidates before the threshold
    unsigned* corr;                   // [n_cells] (ordered) difference array: entries whose first beaten threshold this is
    unsigned* rank;                   // [n_cells] (caller's order)
    unsigned* n_adm;                  // [n_users]
    const unsigned* grow;             // [ngroups] chunk user of a group            (section 1g only)
    const unsigned* gstart;           // [ngroups] its first ordered entry
    unsigned ngroups, nslices, tiles_per_slice;
    const unsigned* iptr;             // [n_users + 1] the chunk's include rows, from 0   (section 1j only)
    const unsigned* incl;             // the chunk's include lists, one after the other, each strictly ascending
    TbExcl excl;                      // E(u) of the chunk's users
};

__device__ __forceinline__ float rb_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double rb_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the k-ordered fused chain of pair_dot_kernel
__device__ __forceinline__ real_t rb_dot(const real_t* A, const real_t* B, int k, unsigned u, unsigned j)
{
    const real_t* p = A + (size_t)u * (size_t)k;
    const real_t* q = B + (size_t)j * (size_t)k;
    real_t s = 0;
    for (int c = 0; c < k; c++) s = rb_fma(p[c], q[c], s);
    return s;
}

// the first of n thresholds ordered best first that (s, j) comes before; n when there is none
__device__ __forceinline__ unsigned rb_first_beaten(const real_t* ts, const unsigned* tj, unsigned n, real_t s, unsigned j)
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (tb_better(s, j, ts[mid], tj[mid])) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

template <bool INCL> __global__ __launch_bounds__(256) void rank_threshold_kernel(RbArgs a)
{
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.n_cells) return;
    const unsigned i = a.cell_row[c], j = a.cell_item[c];
    a.cell_score[c] = rb_dot(a.A, a.B, a.k, a.arow[i], j);
    bool out = tb_excluded(a.excl, i, a.arow[i], j);
    if (INCL) out = out || !tb_sorted_has(a.incl, a.iptr[i], a.iptr[i + 1], j);   // not a candidate of this user
    a.cell_excl[c] = out ? 1u : 0u;
}

__global__ __launch_bounds__(256) void rank_order_kernel(RbArgs a)
{
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.n_cells) return;
    const unsigned i = a.cell_row[c];
    const unsigned p0 = a.tptr[i], p1 = a.tptr[i + 1];
    const real_t s = a.cell_score[c];
    const unsigned j = a.cell_item[c];
    const bool valid = a.cell_excl[c] == 0;
    unsigned pos = 0, nv = 0;
    for (unsigned q = p0; q < p1; q++) {
        const bool vq = a.cell_excl[q] == 0;
        nv += vq ? 1u : 0u;
        bool first;   // cell q stands before cell c
        if (vq && valid) first = tb_better(a.cell_score[q], a.cell_item[q], s, j);
        else if (vq != valid) first = vq;
        else first = q < c;
        pos += first ? 1u : 0u;
    }
    a.s_score[p0 + pos] = s;
    a.s_item[p0 + pos] = j;
    a.s_origin[p0 + pos] = c;
    if (c == p0) a.nvalid[i] = nv;
}

// INCL false (section 1g): `dense` counted every item and the difference array the items of E(u) among them, which leave again.
// INCL true (section 1j): excluded candidates were never counted; the difference array holds what was counted against thresholds
// searched in global memory, `dense` what was counted in LDS -- one of the two is zero for any one user.
template <bool INCL> __global__ __launch_bounds__(256) void rank_finish_kernel(RbArgs a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_users) return;
    const unsigned p0 = a.tptr[i], p1 = a.tptr[i + 1], nv = a.nvalid[i];
    unsigned run = 0;
    for (unsigned p = p0; p < p1; p++) {
        if (p - p0 < nv) {
            run += a.corr[p];
            a.rank[a.s_origin[p]] = INCL ? a.dense[p] + run : a.dense[p] - run;
        } else
            a.rank[a.s_origin[p]] = RB_EXCLUDED;
    }
}

}  // namespace
