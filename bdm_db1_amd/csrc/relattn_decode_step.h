// The pieces of one attention step (32 keys x 16 queries per wave, d_head = 128) that the decode kernels (relattn_decode.hip,
// relattn_decode_kv8.hip) share: each kernel keeps its own loads, its append and its scheduling and calls these for the arithmetic -- one
// definition, so the kernels cannot drift apart bit-wise.  Lane (a = lane & 15, g = lane >> 4) holds query a of the tile and, of a 16-key
// block, keys 4 g .. 4 g + 3 (the header of relattn_decode.hip describes the geometry).  relattn_mem.hip takes the types and constants and
// keeps a copy of the step's arithmetic (its header says why).
// Also here: the layout of the partial units, which gemm_skinny.hip and decode_chain.hip read with merges of their own.
#pragma once
#include "db1_common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
#define LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))

#define DEC_D 128
#define DEC_WAVE_LDS (32 * 256 + 48 * 16 * 4)  // V tile [32][128] bf16 + T scratch [48][16] f32

// ---- partial units: [(b H + h) nunit + unit][DEC_PART_ROWS query rows][O[DEC_D] (unnormalised), m, l] fp32
#define DEC_PART_ROWS 64
#define DEC_PART_LD (DEC_D + 2)
#define DEC_PART_UNIT ((int64_t)DEC_PART_ROWS * DEC_PART_LD)   // floats per unit
__device__ __forceinline__ int64_t dec_part_off(int b, int H, int h, int nunit, int unit, int row) {
    return ((((int64_t)b * H + h) * nunit + unit) * DEC_PART_ROWS + row) * DEC_PART_LD;
}

// the arguments of the ring kernels (bf16 ring: bf16 rows; fp8 ring: slots of kv8_format.h)
struct DecodeRingArgs {
    const bf16_t* qkv; const bf16_t* u; const bf16_t* vb; unsigned char* ring; const int* state; const bf16_t* R;
    float* part; bf16_t* out; unsigned* tickets;
    int B, q, klen, mlen, H, shift, nd, nunit, cap;
    float scale;
};
// out[b, i, h, :] = the units of (b, h) merged in unit order, nunit <= 64 (relattn_decode.hip: relattn_decode_merge2_kernel)
int dec_launch_merge2(const float* part, bf16_t* out, int B, int q, int H, int nunit, hipStream_t st);

__device__ __forceinline__ bf16x8_t dec_add_bias(const bf16x8_t a, const bf16x8_t b) {   // q + bias, rounded to bf16 like db1_relattn_add_head_bias
    union { unsigned u[4]; bf16x8_t v; } o;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const float x0 = __uint_as_float((unsigned)(unsigned short)a[2 * t] << 16) + __uint_as_float((unsigned)(unsigned short)b[2 * t] << 16);
        const float x1 = __uint_as_float((unsigned)(unsigned short)a[2 * t + 1] << 16) + __uint_as_float((unsigned)(unsigned short)b[2 * t + 1] << 16);
        o.u[t] = f2bf_pk(x0, x1);
    }
    return o.v;
}
__device__ __forceinline__ void dec_st_agent(float* p, float a, float b) {   // 8 bytes, write-through (sc1)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), ((unsigned long long)__float_as_uint(b) << 32) | __float_as_uint(a), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void dec_ld_agent2(const float* p, float& a, float& b) {   // 8 bytes, L1-bypassing (sc1)
    const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a = __uint_as_float((unsigned)v); b = __uint_as_float((unsigned)(v >> 32));
}

// query i sees key j
__device__ __forceinline__ bool dec_visible(int i, int j, int q, int klen, int mlen, int shift) {
    return (j < klen) && (j <= i + mlen) && (j > i - shift) && (i < q);
}

// ---- relative term: T[dist][query] = R[dist] . (q + v) for the 48 distances d_lo .. d_lo + 47 (d_lo = mlen + i0 - j0 - 31) of a 16 x 32 block,
// 3 x 4 MFMA; row(tb, ks) = elements 32 ks + 8 g .. + 7 of the R row of distance d_lo + 16 tb + a (from registers or global memory)
template <class RowFn>
__device__ __forceinline__ void dec_rel_term(float* Tw, const bf16x8_t (&fqv)[4], int a, int g, RowFn row) {
#pragma unroll
    for (int tb = 0; tb < 3; tb++) {
        f32x4 acc_t = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ks++) acc_t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row(tb, ks), fqv[ks], acc_t, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) Tw[(16 * tb + 4 * g + r) * 16 + a] = acc_t[r];
    }
}
// ... read back skewed: the term of (query a, key j0 + bcol).  (The same wave wrote and reads the scratch; LDS operations of a wave complete in order)
__device__ __forceinline__ float dec_rel_read(const float* Tw, int a, int bcol) { return Tw[(a - bcol + 31) * 16 + a]; }

// ---- online softmax over the tile's 32 keys: lane-local statistics + two cross-group shuffles.  s: eight masked scores (-1e30 = masked)
__device__ __forceinline__ float dec_tile_max(const float (&s)[8]) {
    float mb = s[0];
#pragma unroll
    for (int t = 1; t < 8; t++) mb = fmaxf(mb, s[t]);
    mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
    mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
    return mb;
}
__device__ __forceinline__ float dec_tile_exp(float (&s)[8], float m) {   // s <- exp(s - m) (fp32 probabilities); returns their row sum
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < 8; t++) { s[t] = s[t] > -1.0e29f ? __expf(s[t] - m) : 0.f; rs += s[t]; }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    return rs;
}
// the update of the running (m, l); s becomes the probabilities; returns alpha, the factor that rescales what was accumulated before
__device__ __forceinline__ float dec_softmax_update(float (&s)[8], float& m_i, float& l_i) {
    const float m_new = fmaxf(m_i, dec_tile_max(s));
    const float alpha = __expf(m_i - m_new);
    const float rs = dec_tile_exp(s, m_new);
    l_i = l_i * alpha + rs;
    m_i = m_new;
    return alpha;
}
__device__ __forceinline__ bf16x8_t dec_pack_p(const float (&s)[8]) {
    union { unsigned u[4]; bf16x8_t v; } pb;
#pragma unroll
    for (int t = 0; t < 4; t++) pb.u[t] = f2bf_pk(s[2 * t], s[2 * t + 1]);
    return pb.v;
}

// ---- O^T[d][query] = alpha O^T + V^T . P^T over the 32 keys of the wave's unswizzled V tile [32][128] bf16 (8 MFMA; V^T via ds_read_b64_tr_b16,
// with the key permutation that makes the S registers directly the B operand: slots 0-3 = keys 4g..4g+3 of the first 16-key block, 4-7 of the second)
__device__ __forceinline__ void dec_pv(f32x4 (&acc_o)[8], const char* Vs, const bf16x8_t pb, const float alpha, int a, int g) {
#pragma unroll
    for (int db = 0; db < 8; db++) {
        const char* base = Vs + (a >> 2) * 256 + (db * 16 + (a & 3) * 4) * 2;
        const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(bf16x4_t, const_cast<char*>(base) + (4 * g) * 256));
        const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(bf16x4_t, const_cast<char*>(base) + (16 + 4 * g) * 256));
        const bf16x8_t vt = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int r = 0; r < 4; r++) acc_o[db][r] *= alpha;
        acc_o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt, pb, acc_o[db], 0, 0, 0);
    }
}

// ---- a workgroup's four waves (one 32-key step each; every wave must arrive) merged through LDS into ONE unit, waves in order: thread =
// (query qi = threadIdx.x & 15 of the tile, columns dg = (threadIdx.x >> 4) * 8 .. + 7) gets o8, the maximum and the sum.  smem: the
// workgroup's LDS, WAVE_LDS bytes per wave (each wave's own V stage / T scratch, >= 16 rows x 132 floats: it is done with them)
template <int WAVE_LDS>
__device__ __forceinline__ void dec_merge_waves(char* smem, const f32x4 (&acc_o)[8], float m_i, float l_i, float (&o8)[8], float& mx, float& lsum) {
    constexpr int OLD = DEC_D + 4;                       // floats per query row in LDS: O[128], m, l, pad
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, g = lane >> 4;
    float* mine = reinterpret_cast<float*>(smem + wave * WAVE_LDS);
#pragma unroll
    for (int db = 0; db < 8; db++) *reinterpret_cast<f32x4*>(mine + a * OLD + db * 16 + 4 * g) = acc_o[db];
    if (g == 0) { mine[a * OLD + DEC_D] = m_i; mine[a * OLD + DEC_D + 1] = l_i; }
    __syncthreads();
    const int qi = threadIdx.x & 15, dg = (threadIdx.x >> 4) * 8;
    const float* w0p = reinterpret_cast<const float*>(smem) + qi * OLD;
    float mw[4], lw[4];
    mx = -1.0e30f;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        mw[w] = w0p[w * (WAVE_LDS / 4) + DEC_D]; lw[w] = w0p[w * (WAVE_LDS / 4) + DEC_D + 1];
        mx = fmaxf(mx, mw[w]);
    }
    lsum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) o8[j] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) {   // (waves in order: deterministic)
        const float wt = lw[w] > 0.f ? __expf(mw[w] - mx) : 0.f;
        lsum += lw[w] * wt;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(w0p + w * (WAVE_LDS / 4) + dg), hi = *reinterpret_cast<const f32x4*>(w0p + w * (WAVE_LDS / 4) + dg + 4);
#pragma unroll
        for (int j = 0; j < 4; j++) { o8[j] += lo[j] * wt; o8[4 + j] += hi[j] * wt; }
    }
}
// this thread's piece of a unit row: columns dg .. dg + 7 and, from the dg == 0 thread, (m, l); through = as 8-byte write-through stores
__device__ __forceinline__ void dec_store_unit(float* dst, int dg, const float (&o8)[8], float mx, float lsum, bool through) {
    if (through) {
#pragma unroll
        for (int j = 0; j < 8; j += 2) dec_st_agent(dst + dg + j, o8[j], o8[j + 1]);
        if (dg == 0) dec_st_agent(dst + DEC_D, mx, lsum);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j += 2) *reinterpret_cast<float2*>(dst + dg + j) = make_float2(o8[j], o8[j + 1]);
        if (dg == 0) { dst[DEC_D] = mx; dst[DEC_D + 1] = lsum; }
    }
}

// ---- the merge over the chunks inside the attention launch (one launch less per layer): called by every workgroup (256 threads) of a ring
// kernel after its unit went out through dec_store_unit(.., true).  The workgroup that finishes last for this (batch, head, query tile)
// merges the units (ticket counter, zero on entry and left zero) -- the arithmetic of relattn_decode_merge2_kernel.
// Hand-off: the per-XCD L2s are not coherent and an L1 is never refreshed, so (1) the partials went out as write-through 8-byte stores,
// (2) every wave drains them (vmcnt(0)) before the barrier, (3) one relaxed agent-scope ticket per workgroup orders the workgroups, and
// (4) the merging workgroup reads the partials with L1-bypassing (sc1) loads.
__device__ __forceinline__ void dec_inlaunch_merge(const DecodeRingArgs& p, int b, int h, int nqt, int i0) {
    __shared__ unsigned ticket_s;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* tk = p.tickets + ((int64_t)b * p.H + h) * nqt + i0 / 16;
    if (threadIdx.x == 0) ticket_s = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (ticket_s != gridDim.x / nqt - 1) return;
    if (threadIdx.x == 0) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // thread = (query qi of the tile, 8 output columns): all units' pieces are requested at once (<= 16 chunks: klen <= 2048; slots past nunit
    // repeat the last unit and get weight zero), weighted in chunk order -- one round trip instead of one per row pair
    constexpr int NU = 16;
    const int qi = threadIdx.x & 15, dg = (threadIdx.x >> 4) * 8;
    const bool valid = i0 + qi < p.q;
    const float* src = p.part + dec_part_off(b, p.H, h, p.nunit, 0, valid ? i0 + qi : i0);
    float mlm[NU], mll[NU], ov[NU][8];
#pragma unroll
    for (int c = 0; c < NU; c++) {
        const float* u = src + (c < p.nunit ? c : p.nunit - 1) * DEC_PART_UNIT;
        dec_ld_agent2(u + DEC_D, mlm[c], mll[c]);
#pragma unroll
        for (int j = 0; j < 8; j += 2) dec_ld_agent2(u + dg + j, ov[c][j], ov[c][j + 1]);
    }
    float mx = -1.0e30f;
#pragma unroll
    for (int c = 0; c < NU; c++) mx = fmaxf(mx, c < p.nunit ? mlm[c] : -1.0e30f);
    float l = 0.f, o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NU; c++) {
        const float lc = c < p.nunit ? mll[c] : 0.f;
        const float wt = lc > 0.f ? __expf(mlm[c] - mx) : 0.f;
        l += lc * wt;
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] += ov[c][j] * wt;
    }
    if (valid) {
        uint4 w;
        w.x = f2bf_pk(l > 0.f ? o[0] / l : 0.f, l > 0.f ? o[1] / l : 0.f); w.y = f2bf_pk(l > 0.f ? o[2] / l : 0.f, l > 0.f ? o[3] / l : 0.f);
        w.z = f2bf_pk(l > 0.f ? o[4] / l : 0.f, l > 0.f ? o[5] / l : 0.f); w.w = f2bf_pk(l > 0.f ? o[6] / l : 0.f, l > 0.f ? o[7] / l : 0.f);
        *reinterpret_cast<uint4*>(p.out + ((int64_t)b * p.q + i0 + qi) * p.H * DEC_D + h * DEC_D + dg) = w;
    }
}
