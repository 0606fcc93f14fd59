// Order-preserving logit keys and fixed-order block reductions shared by next-token selection (select.hip), beam search (beam.hip), scoring
// (score.hip) and action decoding (action.hip).
//
// sel_key maps a float to a uint32 whose unsigned order is the float order (0 = not a candidate: NaN, +-inf), so max / arg-max are integer
// reductions; packing (key << 32) | ~column into a uint64 makes the arg-max pick the lowest column on ties.  Block reductions: every wave
// reduces by butterfly (every lane ends with the same bits), writes one LDS slot, one barrier, every thread combines the NW slots in order --
// the same inputs give the same bits.  Consecutive reductions alternate between two slot sets, so a slot is never rewritten while a slower
// wave may still read it (one barrier per reduction).
//
// sel_top_rounds: the n best candidates of a row in the order of those packed pairs (logit descending, ties by the lower column), one
// block_max_u64 per round (db1_select_tokens_top, db1_score_rows_top).  A pair holds its column, so no two candidates share one and the
// winner of a round belongs to exactly one thread: only that thread looks for its next best pair, below the winner; every other thread's
// best pair is still its best.
#pragma once
#include "db1_common.h"

__device__ __forceinline__ unsigned sel_key(float f) {
    const unsigned b = __float_as_uint(f);
    if ((b & 0x7f800000u) == 0x7f800000u) return 0u;          // NaN, +-inf: never a candidate
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);          // finite keys are > 0x007fffff
}
__device__ __forceinline__ float sel_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)x, o, 64), hi = __shfl_xor((unsigned)(x >> 32), o, 64);
        const unsigned long long y = ((unsigned long long)hi << 32) | lo;
        x = y > x ? y : x;
    }
    return x;
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (unsigned)__shfl_xor(x, o, 64));
    return x;
}

template <int NW>
struct SelSharedT {
    unsigned long long u64[2][NW];
    float f[2][NW];
    int i[2][NW];
    unsigned u[2][NW];
};
template <int NW>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long x, SelSharedT<NW>& sh, int& ph) {
    x = wave_max_u64(x);
    if ((threadIdx.x & 63) == 0) sh.u64[ph][threadIdx.x >> 6] = x;
    __syncthreads();
    unsigned long long r = sh.u64[ph][0];
#pragma unroll
    for (int w = 1; w < NW; w++) r = sh.u64[ph][w] > r ? sh.u64[ph][w] : r;
    ph ^= 1;
    return r;
}
template <int NW>
__device__ __forceinline__ unsigned block_min_u32(unsigned x, SelSharedT<NW>& sh, int& ph) {
    x = wave_min_u32(x);
    if ((threadIdx.x & 63) == 0) sh.u[ph][threadIdx.x >> 6] = x;
    __syncthreads();
    unsigned r = sh.u[ph][0];
#pragma unroll
    for (int w = 1; w < NW; w++) r = min(r, sh.u[ph][w]);
    ph ^= 1;
    return r;
}
template <int NW>
__device__ __forceinline__ int block_sum_i(int x, SelSharedT<NW>& sh, int& ph) {   // x wave-uniform already
    if ((threadIdx.x & 63) == 0) sh.i[ph][threadIdx.x >> 6] = x;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) r += sh.i[ph][w];
    ph ^= 1;
    return r;
}
template <int NW>
__device__ __forceinline__ float block_sum_f(float x, SelSharedT<NW>& sh, int& ph) {
    x = wave_sum(x);   // (butterfly: every lane ends with the same bits)
    if ((threadIdx.x & 63) == 0) sh.f[ph][threadIdx.x >> 6] = x;
    __syncthreads();
    float r = sh.f[ph][0];
#pragma unroll
    for (int w = 1; w < NW; w++) r += sh.f[ph][w];
    ph ^= 1;
    return r;
}

// The threshold search of top-k / top-p: the largest x in [l, h] with ok(x), for a block-uniform, monotone ok (true up to some x, false above)
// that holds at l.  ok may reduce over the block: every thread walks the same midpoints.
template <typename Ok>
__device__ __forceinline__ unsigned sel_bisect_max(unsigned l, unsigned h, Ok ok) {
    while (l < h) {
        const unsigned mid = l + ((h - l) >> 1) + ((h - l) & 1);
        if (ok(mid)) l = mid; else h = mid - 1;
    }
    return l;
}

// the packed pair of a candidate (0: not a candidate)
__device__ __forceinline__ unsigned long long sel_pair(unsigned key, int col) {
    return key ? ((unsigned long long)key << 32) | (unsigned)~col : 0ull;
}
// A zero the compiler cannot see through (no instruction).  The scans below add it to the literal column offsets of their unrolled elements: a
// bare literal cannot be an operand of the select that keeps the best offset, so the compiler would load one register per element of the row
// with its literal and keep all of them alive across the rounds.
__device__ __forceinline__ int sel_opaque_zero() {
    int z = 0;
    asm volatile("" : "+v"(z));
    return z;
}
// One element of a thread's scan for its best pair strictly below a winner (key wk, column wc; ~0ull: below nothing).  The thread's elements are
// visited by ascending column; `off` = the element's column minus the thread's first one (sel_opaque_zero() + a literal) and d = wc minus that
// first column.  (bk, bo): the best key so far and its `off`.
__device__ __forceinline__ void sel_scan_step(unsigned k, int off, unsigned wk, int d, unsigned& bk, int& bo) {
    // (k > bk: among equal keys the first, the lowest column, stays; | and &, not || and &&: no branch per element)
    const bool up = ((k < wk) | ((k == wk) & (off > d))) & (k > bk);
    bk = up ? k : bk;
    bo = up ? off : bo;
}
// scan(below) -> the thread's best pair strictly below `below` (~0ull: its best pair; 0: it holds no such candidate); `first`: the block's best
// pair when the caller has reduced it already (round 0 then costs no reduction), else 0; emit(i, winner, own): round i's winner, `own` on the
// one thread that holds it.  Rounds end at n or when no pair is left -> the number of rounds that found one (block-uniform).  Every thread
// scans once, before round 0; after that only the owner of the last winner does.
template <int NW, typename Scan, typename Emit>
__device__ __forceinline__ int sel_top_rounds(int n, unsigned long long first, Scan scan, Emit emit, SelSharedT<NW>& sh, int& ph) {
    unsigned long long mine = 0, below = ~0ull;
    bool own = true;
    int i = 0;
#pragma nounroll
    for (; i < n; i++) {
        if (own) mine = scan(below);
        below = (i == 0 && first) ? first : block_max_u64(mine, sh, ph);
        if (!(unsigned)(below >> 32)) break;
        own = mine == below;
        emit(i, below, own);
    }
    return i;
}
