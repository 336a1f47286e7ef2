// quad_eval.hpp -- the register-tile engine of reg_eval.hpp for ONE case: PG on floats, k = 50, one wave per row, the factor read from its
// line-padded copy (row stride 256 bytes).  A nonzero is held by FOUR lanes instead of sixteen.
//
// RegEval keeps a factor row in 16 lanes x 4 floats = 64 elements: at k = 50 lanes 13 .. 15 of every group multiply zeros (19 % of the packed
// ops of a pass), and every nonzero's dot product is a reduction over 16 lanes.  Here
//
//   lane = 4 j + q: step s (0 <= s < Q) handles the 16 nonzeros 16 s + j, one per quad; lane q of the quad holds elements 12 q .. 12 q + 11 of
//   F[ind] (three aligned 16-byte loads): t[s], twelve registers per lane and step.  Elements 48, 49 -- the tail -- are held ONCE per nonzero,
//   in the lane that finishes the nonzero: after the dots' butterfly lane q of quad j holds the prediction of step 4 b + q, nonzero
//   64 b + 16 q + j, the one whose index and value the lane loaded itself (idx[b], xr[b]); tt[b] is that nonzero's (e48, e49), one aligned
//   8-byte load per lane and batch of four steps, its address from the lane's own index.  The tile is 12 Q + 2 ceil(Q / 4) registers.
//   (The tail as a seventh register pair of every step -- (e48, e49) in lane 0 of the quad, zeros in lanes 1 .. 3 -- was the first layout: one
//   packed op in seven of either phase for two elements, and three of four of the fourth loads fetching zeros.  One element each in lanes 0
//   and 1 -- 13 registers per step -- needs the step-pair interleave to keep whole packed ops, and with it 2 x 13 accumulators and the
//   gather's swaps.)
//
//   dots     six packed ops and one add per step; the Q lane-partials are reduced over the quad by a transposing butterfly on quad_perm DPP
//            (four steps together: three folds), which leaves the prediction of step 4 b + q in lane q, and the lane adds its own tail: two
//            multiply-adds per batch -- 64 nonzeros in 64 lanes, one division each;
//   axpy     acc += coef_s * t[s] in step order, the coefficient from lane s % 4 of the quad by ds_swizzle; six packed ops per step, and per
//            batch one more for the tail, tail_acc += coef * tt[b], with the lane's own coefficient;
//   gradient the 14 accumulators -- twelve and the tail's two -- are reduced over the 16 quads by a second transposing butterfly -- lane ^ 4
//            and lane ^ 8 as banked DPP adds inside the 16-lane row, lane ^ 16 by ds_swizzle, lane ^ 32 by ds_bpermute -- after which every
//            main dimension's sum sits in ONE lane (dim_of below).  The butterfly joins lanes of equal q only, so the tail's totals (quads 11
//            and 7) are still one per q: two DPP adds masked to those two quads finish them, and all four lanes of either quad end with the
//            same bits.  Each lane carries its dimension alone through the solver's update: NC = 1;
//   point    the updated point goes back to the quads' 12 elements per lane and the tail's two by ds_bpermute with immediate offsets from one
//            address register; dimensions 48, 49 are read from the lane of the same q in quads 11, 7, which is why those carry copies.
//
// The association of every sum is a function of the layout alone: steps past the end of a row hold zeros and get a zero coefficient, so a row's
// bits do not depend on the instance (Q) it runs on.
#pragma once
#include "reg_eval.hpp"

namespace pmf {

// One level of the butterfly over the quads of a 16-lane DPP row, all folds in one block (reg_eval.hpp, PMF_FOLD2, on why asm).
// lane ^ 4: the classes are banks {0,2} | {1,3}; the partner of a lane of banks 0, 2 is four lanes up (row_shl:4), of banks 1, 3 four lanes down.
#define PMF_QFOLD4(Q, A, B) \
    "v_add_f32_dpp " Q ", " A ", " A " row_shl:4 row_mask:0xf bank_mask:0x5\n\t" \
    "v_add_f32_dpp " Q ", " B ", " B " row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
// fourteen inputs -> seven: output i collects input i in the quads of class 0 and input i + 7 in those of class 1
__device__ __forceinline__ void quad_fold14(const float (&p)[14], float (&q)[7])
{
    asm("s_nop 1\n\t"
        PMF_QFOLD4("%0", "%7", "%14")
        PMF_QFOLD4("%1", "%8", "%15")
        PMF_QFOLD4("%2", "%9", "%16")
        PMF_QFOLD4("%3", "%10", "%17")
        PMF_QFOLD4("%4", "%11", "%18")
        PMF_QFOLD4("%5", "%12", "%19")
        PMF_QFOLD4("%6", "%13", "%20")
        : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2]), "=&v"(q[3]), "=&v"(q[4]), "=&v"(q[5]), "=&v"(q[6])
        : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]),
          "v"(p[7]), "v"(p[8]), "v"(p[9]), "v"(p[10]), "v"(p[11]), "v"(p[12]), "v"(p[13]));
}
// lane ^ 8 (row_ror:8; banks {0,1} | {2,3}), seven inputs -> four: three pairs (i, i + 4) and input 3 on its own
__device__ __forceinline__ void quad_fold7(const float (&q)[7], float (&r)[4])
{
    asm("s_nop 1\n\t"
        PMF_FOLD2("row_ror:8", "0x3", "0xc", "%0", "%4", "%8")
        PMF_FOLD2("row_ror:8", "0x3", "0xc", "%1", "%5", "%9")
        PMF_FOLD2("row_ror:8", "0x3", "0xc", "%2", "%6", "%10")
        PMF_FOLD1("row_ror:8", "%3", "%7")
        : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
        : "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]));
}
// The tail's totals over the four lanes of their quads: lane ^ 1, then lane ^ 2, in quads 7 and 11 only -- DPP rows 1 and 2, bank 3; a
// masked-off lane keeps its value.  Both lanes of a pair add the same two operands at either level, so the quad's four lanes end with the
// same bits.  (s_nop 1: the two wait states between a VALU write and its DPP read, before either add.)
__device__ __forceinline__ float quad_tail_sum(float g)
{
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0x6 bank_mask:0x8\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0x6 bank_mask:0x8"
        : "+v"(g));
    return g;
}

template <int Q> struct QuadEval {
    using T = float;
    static_assert(Q >= 1 && Q <= 10, "one to ten steps of sixteen nonzeros");
    typedef float V2 __attribute__((ext_vector_type(2)));
    struct __attribute__((packed, aligned(4))) U4 { float v[4]; };
    struct __attribute__((packed, aligned(4))) U2 { float v[2]; };
    static constexpr int K = 50;                  // the one factor dimension this engine is built for
    static constexpr int NP = 6;                  // register pairs per lane and step
    static constexpr int NA = NP + 1;             // ... of the point and of the accumulators: the lane's twelve elements and the tail's two
    static constexpr int NE = 2 * NA;             // accumulators per lane
    static constexpr int NC = 1;                  // the solver's k-vectors: one element per lane
    static constexpr int NB = (Q + 3) / 4;        // batches of four steps = 64 nonzeros
    static constexpr int TILE_REGS = 2 * NP * Q + 2 * NB;
    static constexpr int NW = 1, M = 1;
    static constexpr bool PIPELINED = true;       // (as RegEval: sweep_rows prefetches the next row's indices during the solver)
    static constexpr int PIPE_MW = 1;
    static constexpr bool FUSED_SUMS = false, PREFETCH = false, MAY_CACHE = false, CACHED_GRAD = false;
    static constexpr bool PG_LEAN = true;
    static constexpr int SMEM_BYTES = 0;
    static_assert(K == 4 * 2 * NP + 2, "four lanes of twelve elements and a tail of two");

    V2 t[Q][NP];         // the tile: t[s][e] = this lane's elements 2 e, 2 e + 1 of the nonzero its quad holds in step s
    V2 tt[NB];           // the tail: elements 48, 49 of the nonzero whose prediction this lane finishes in batch b
    V2 a[NA];            // the current point: this lane's 12 elements, then elements 48, 49
    T xr[NB];            // x_j of the nonzero whose prediction this lane finishes in batch b: j = 64 b + jlane
    unsigned idx_n[NB];  // column indices of the row whose tile is requested next, same layout
    const T* F;
    unsigned zero_row;
    int k, ldF;
    int lane, q, wid, member;
    int jlane;           // 16 q + lane / 4
    int dim;             // the factor dimension this lane carries through the solver
    bool primary;        // ... and is the one lane to store it (lanes 56 .. 63 hold copies of lanes 48 .. 55, lanes 1 .. 3 of quads 7, 11 of their lane 0)
    bool cls1, cls2, cls16, cls32;
    int xor32_addr;      // the ds_bpermute address of lane ^ 32
    int quad_addr;       // the ds_bpermute address of lane q: the point's elements come from lanes q + 4 m (set_point_as_is)
    unsigned nnz;
    unsigned n_eval;
#ifdef PMF_PROBE
    unsigned* probe = nullptr;
#endif

    // the accumulator (0 .. 13) whose total the butterfly of cross_quads leaves in the lane of quad number `quad` (0 .. 15)
    static __host__ __device__ constexpr int acc_of(int quad)
    {
        const int n = ((quad >> 3) & 1) + 2 * ((quad >> 2) & 1) + 4 * ((quad >> 1) & 1);   // the levels lane ^ 32, ^ 16, ^ 8 pick bit 0, 1, 2
        return (n == 7 ? 3 : n) + 7 * (quad & 1);                                           // (n = 7: the unpaired input 3 of quad_fold7 again)
    }
    // ... and the quad that ends with accumulator e
    static __host__ __device__ constexpr int quad_of(int e)
    {
        const int n = e % 7;
        return (e / 7) + 2 * ((n >> 2) & 1) + 4 * ((n >> 1) & 1) + 8 * (n & 1);
    }
    // the dimension of accumulator e in lane q_ of a quad: one of the lane's own twelve, or -- in every lane -- one of the tail's two
    static __host__ __device__ constexpr int dim_of(int q_, int e) { return e < 2 * NP ? 2 * NP * q_ + e : 8 * NP + (e - 2 * NP); }

    __device__ __forceinline__ void init(const TileGeom& geo, const T* F_, unsigned char*)
    {
        lane = lane_id();
        F = F_;
        k = geo.k; ldF = geo.ldF; zero_row = geo.zero_row;
        q = lane & 3; wid = 0; member = 0;
        jlane = 16 * q + (lane >> 2);
        cls1 = (lane & 1) != 0; cls2 = (lane & 2) != 0; cls16 = (lane & 16) != 0; cls32 = (lane & 32) != 0;
        const int quad = lane >> 2;
        const int e = acc_of(quad);
        dim = dim_of(q, e);
        primary = (quad >> 1) != 7 && (e < 2 * NP || q == 0);
        // (opaque: left visible, the compiler rebuilds the addresses from the lane number wherever they are used -- in every pass)
        xor32_addr = (lane ^ 32) << 2;
        quad_addr = q << 2;
        asm volatile("" : "+v"(xor32_addr), "+v"(quad_addr));
    }

    // ---- k-vectors: element `dim` in its lane -----------------------------------------------------------
    __device__ __forceinline__ void load_vec(const T* p, T (&x)[NC]) const { x[0] = p[dim]; }
    __device__ __forceinline__ void start_point(const T* mrow, T (&x)[NC]) const { load_vec(mrow, x); }
    __device__ __forceinline__ void store_vec(T* p, const T (&x)[NC]) const
    {
        if (primary) p[dim] = x[0];
    }

    // ---- gather (RegEval's, in this layout) ----------------------------------------------------------------
    __device__ __forceinline__ void fetch_meta(const unsigned* ind, unsigned nnz_row)
    {
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const unsigned j = (unsigned)(64 * b + jlane);
            idx_n[b] = j < nnz_row ? ind[j] : zero_row;   // steps past the end of the row fetch the all-zero row behind F
        }
    }
    __device__ __forceinline__ void begin_row(const unsigned* ind, const T* val, unsigned nnz_row)
    {
        fetch_meta(ind, nnz_row);
        gather(val, nnz_row);
    }
    __device__ __forceinline__ unsigned* ticket_slot() const { return nullptr; }
    __device__ __forceinline__ void gather(const T* val, unsigned nnz_row)
    {
        nnz = nnz_row;
        unsigned idx[NB];
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const unsigned j = (unsigned)(64 * b + jlane);
            idx[b] = idx_n[b];
            xr[b] = j < nnz ? val[j] : (T)0;
        }
        // byte offsets into the padded copy: 24-bit multiply-add, 32-bit result (the planner's conditions for the register engine).  The three
        // slots of lane q start at byte 48 q of the row; the tail is bytes 192 .. 199 of the row of the lane's OWN index (a lane past the end of
        // the row carries the zero row there and reads zeros).
        const unsigned rowbytes = (unsigned)ldF * (unsigned)sizeof(T);
        const unsigned main_off = (unsigned)q * 48u;
#pragma unroll
        for (int b = 0; b < NB; b++) tt[b] = (V2){ (T)0, (T)0 };   // (a last batch of fewer than four steps leaves lanes without a nonzero)
        static_for<0, Q>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            // the index of nonzero 16 s + j sits in lane s % 4 of quad j
            const unsigned c = group_bcast<4, s % 4>(idx[s / 4]);
            // all three loads of a step back to back: the pieces of a factor row's two cache lines meet in flight
            const char* base = (const char*)F + (size_t)(__umul24(c, rowbytes) + main_off);
            const U4 v0 = *(const U4*)base;
            const U4 v1 = *(const U4*)(base + 16);
            const U4 v2 = *(const U4*)(base + 32);
            t[s][0] = (V2){ v0.v[0], v0.v[1] }; t[s][1] = (V2){ v0.v[2], v0.v[3] };
            t[s][2] = (V2){ v1.v[0], v1.v[1] }; t[s][3] = (V2){ v1.v[2], v1.v[3] };
            t[s][4] = (V2){ v2.v[0], v2.v[1] }; t[s][5] = (V2){ v2.v[2], v2.v[3] };
            // ... and that lane fetches the nonzero's tail, right behind the step's loads of the same factor row: the line is on its way for lanes 2, 3
            // of the quad.  (One load per batch for all 64 lanes, in front of or behind the batch's steps, asks for lines that are no longer, or not
            // yet, in the first-level cache: every launch of PG(1) ran 3-6 % longer.)
            if (q == s % 4) {
                const U2 w = *(const U2*)((const char*)F + (size_t)(__umul24(idx[s / 4], rowbytes) + 192u));
                tt[s / 4] = (V2){ w.v[0], w.v[1] };
            }
        });
    }
    // A row without nonzeros has no tile; saying so keeps the tile from being carried from one row of the kernel's loop to the next (RegEval::idle_tile)
    __device__ __forceinline__ void idle_tile()
    {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int s = 0; s < Q; s++) {
#pragma unroll
            for (int e = 0; e < NP; e++) t[s][e] = (V2){ (T)0, (T)0 };
        }
#pragma unroll
        for (int b = 0; b < NB; b++) tt[b] = (V2){ (T)0, (T)0 };
    }

    // ---- the point: every lane fetches its 14 elements from the lanes that carry them --------------------------
    // Every lane carries a dimension, and the solver's update is elementwise, so a copy computes its original's bits: nothing to mask
    // (reg_eval.hpp, PG_LEAN).
    __device__ __forceinline__ void set_point_as_is(const T (&x)[NC])
    {
        // (asm: through the builtin the compiler keeps quad_addr + offset in a register per element, fourteen of them, where the instruction has an
        // offset field; the wait is part of the block because the compiler does not count the LDS operations of inline asm)
#define PMF_QPERM(D, E) "ds_bpermute_b32 " D ", %14, %15 offset:%" E "\n\t"
        float r[NE];
        asm volatile(PMF_QPERM("%0", "16") PMF_QPERM("%1", "17") PMF_QPERM("%2", "18") PMF_QPERM("%3", "19") PMF_QPERM("%4", "20")
                     PMF_QPERM("%5", "21") PMF_QPERM("%6", "22") PMF_QPERM("%7", "23") PMF_QPERM("%8", "24") PMF_QPERM("%9", "25")
                     PMF_QPERM("%10", "26") PMF_QPERM("%11", "27") PMF_QPERM("%12", "28") PMF_QPERM("%13", "29")
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]), "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7]), "=&v"(r[8]), "=&v"(r[9]),
                       "=&v"(r[10]), "=&v"(r[11]), "=&v"(r[12]), "=&v"(r[13])
                     : "v"(quad_addr), "v"(x[0]), "n"(16 * quad_of(0)), "n"(16 * quad_of(1)), "n"(16 * quad_of(2)), "n"(16 * quad_of(3)),
                       "n"(16 * quad_of(4)), "n"(16 * quad_of(5)), "n"(16 * quad_of(6)), "n"(16 * quad_of(7)), "n"(16 * quad_of(8)), "n"(16 * quad_of(9)),
                       "n"(16 * quad_of(10)), "n"(16 * quad_of(11)), "n"(16 * quad_of(12)), "n"(16 * quad_of(13)));
#undef PMF_QPERM
        // element e of lane q is carried by lane q + 4 quad_of(e); e = 12, 13 -- dimensions 48, 49 -- by that quad's copy in lane q
#pragma unroll
        for (int e = 0; e < NA; e++) a[e] = (V2){ r[2 * e], r[2 * e + 1] };
    }
    __device__ __forceinline__ void set_point(const T (&x)[NC]) { set_point_as_is(x); }

    // N (1 .. 4) lane-partials p[u] -> lane q holds the sum over its quad of p[q] (lanes q >= N: unspecified)
    template <int N> __device__ __forceinline__ T quad_transpose_sum(const T (&p)[4]) const
    {
        T r0, r1;
        if constexpr (N >= 2) r0 = fold_pair<0xB1>(cls1, p[0], p[1]);             // quad_perm[1,0,3,2]  lane ^ 1
        else r0 = fold_one<0xB1>(p[0]);
        if constexpr (N == 4) r1 = fold_pair<0xB1>(cls1, p[2], p[3]);
        else if constexpr (N == 3) r1 = fold_one<0xB1>(p[2]);
        if constexpr (N >= 3) return fold_pair<0x4E>(cls2, r0, r1);               // quad_perm[2,3,0,1]  lane ^ 2
        else return fold_one<0x4E>(r0);
    }

    // the 14 per-lane sums over this quad's nonzeros -> the total over the wave of accumulator acc_of(lane / 4), i.e. of dimension `dim`
    __device__ __forceinline__ T cross_quads(const T (&part)[NE]) const
    {
        T l4[7], l8[4];
        quad_fold14(part, l4);      // lane ^ 4
        quad_fold7(l4, l8);         // lane ^ 8
        // lane ^ 16 stays inside a half-wave: ds_swizzle in bit-mask mode (and 0x1f, or 0, xor 0x10); lane ^ 32: ds_bpermute, its address a
        // launch constant.  The LDS crossbar, not VALU (reg_eval.hpp, combine_groups, on v_permlane*_swap in these kernels).
        T l16[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const T own = cls16 ? l8[i + 2] : l8[i];
            const T send = cls16 ? l8[i] : l8[i + 2];
            l16[i] = own + __builtin_bit_cast(T, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, send), 0x401f));
        }
        const T own = cls32 ? l16[1] : l16[0];
        const T send = cls32 ? l16[0] : l16[1];
        // the twelve main accumulators are totals now; the tail's two (quads 11, 7) are totals per q
        static_assert(quad_of(2 * NP) == 11 && quad_of(2 * NP + 1) == 7, "quad_tail_sum's masks: DPP rows 2 and 1, bank 3");
        return quad_tail_sum(own + __builtin_bit_cast(T, __builtin_amdgcn_ds_bpermute(xor32_addr, __builtin_bit_cast(int, send))));
    }

    // RegEval::eval's contract for what PG asks of it: the gradient, no function value, no cache
    template <bool WANT_F, bool WANT_G, bool FROM_CACHE = false, bool FRESH = false> __device__ __forceinline__ double eval(T sgn, T (&acc)[NC], T* = nullptr)
    {
        static_assert(!WANT_F && WANT_G && !FROM_CACHE, "the quad engine evaluates PG's gradient only");
        n_eval++;
        PMF_STAMP(*this, 0);
        V2 part2[NA];
        static_for<0, NB>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            constexpr int n = (Q - 4 * b) < 4 ? (Q - 4 * b) : 4;
            // the batch's dot products element by element, the steps side by side: n independent chains of packed ops (one step after the other
            // is one chain of six dependent ones, a wait state between every two)
            T p[4];
            V2 s2[n];
#pragma unroll
            for (int u = 0; u < n; u++) s2[u] = t[4 * b + u][0] * a[0];
#pragma unroll
            for (int e = 1; e < NP; e++) {
#pragma unroll
                for (int u = 0; u < n; u++) s2[u] = __builtin_elementwise_fma(t[4 * b + u][e], a[e], s2[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) p[u] = u < n ? s2[u < n ? u : 0].x + s2[u < n ? u : 0].y : (T)0;
            // elements 0 .. 47 summed over the quad, then the lane's own tail
            T pred = quad_transpose_sum<n>(p);
            pred = __builtin_fmaf(tt[b].x, a[NP].x, __builtin_fmaf(tt[b].y, a[NP].y, pred));
            const bool on = (unsigned)(64 * b + jlane) < nnz;
            const T coef = on ? coef_div(sgn * xr[b], pred) : (T)0;
            {
                const V2 c2 = { coef, coef };   // (the lane's own coefficient, before any broadcast)
                if constexpr (b == 0) part2[NP] = c2 * tt[0];
                else part2[NP] = __builtin_elementwise_fma(c2, tt[b], part2[NP]);
            }
            static_for<0, n>([&](auto uc) {
                constexpr int u = decltype(uc)::value;
                const T c = group_bcast<4, u>(coef);
                const V2 c2 = { c, c };
#pragma unroll
                for (int e = 0; e < NP; e++) {
                    if constexpr (b == 0 && u == 0) part2[e] = c2 * t[0][e];
                    else part2[e] = __builtin_elementwise_fma(c2, t[4 * b + u][e], part2[e]);
                }
            });
        });
        PMF_STAMP(*this, 5);
        T part[NE];
#pragma unroll
        for (int e = 0; e < NA; e++) { part[2 * e] = part2[e].x; part[2 * e + 1] = part2[e].y; }
        const T g = cross_quads(part);
        acc[0] = FRESH ? g : acc[0] + g;
        PMF_STAMP(*this, 6);
        return 0.0;
    }

    // acc_c += sum_j F[ind_j, c]  (adjustment_Bsum's gather pass, ref: src/poismf.c:108-110)
    __device__ __forceinline__ void tile_colsum(T (&acc)[NC])
    {
        T part[NE];
#pragma unroll
        for (int i = 0; i < NE; i++) part[i] = (T)0;
#pragma unroll
        for (int s = 0; s < Q; s++) {
#pragma unroll
            for (int e = 0; e < NP; e++) { part[2 * e] += t[s][e].x; part[2 * e + 1] += t[s][e].y; }   // steps past the row's end hold zeros
        }
#pragma unroll
        for (int b = 0; b < NB; b++) { part[2 * NP] += tt[b].x; part[2 * NP + 1] += tt[b].y; }   // (each nonzero's tail once, in the lane that holds it)
        acc[0] += cross_quads(part);
    }
};

}  // namespace pmf
