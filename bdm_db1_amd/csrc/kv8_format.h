// The fp8 K/V slot format (include/db1_hip.h, "fp8 K/V ring"; tests/kv8_rule.py).  The quantising half: one definition for every kernel
// that writes slots -- the ring attention's append and db1_kv8_quantize (relattn_decode_kv8.hip), the prefill's slot writers (ring_prefill.hip).
// The widening half, at the end: a slot's payload to unscaled bf16 for the ring attention (relattn_decode_kv8.hip, which applies the scales
// to scores and probabilities) and to VALUES for the attention over a ring-resident memory (relattn_mem.hip).
#pragma once
#include "db1_common.h"

// the largest finite magnitude (bf16 bits without the sign) among the 8 bf16 of x
__device__ __forceinline__ unsigned kv8_amax8(uint4 x, unsigned m) {
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const unsigned lo = w[t] & 0x7fffu, hi = (w[t] >> 16) & 0x7fffu;
        m = max(m, lo < 0x7f80u ? lo : 0u);
        m = max(m, hi < 0x7f80u ? hi : 0u);
    }
    return m;
}
// the exponent e of the scale 2^e of a block whose largest finite magnitude has the bf16 bits m: the smallest power of two with
// amax <= 448 * 2^e (448 = 1.75 * 2^8), 0 for a block of zeros, at least -126 (a normal fp32)
__device__ __forceinline__ int kv8_scale_exp(unsigned m) {
    if (m == 0) return 0;
    const int e = (int)(m >> 7) - 127 - ((m & 0x7fu) > 96u ? 7 : 8);
    return e < -126 ? -126 : e;
}
// 8 bf16 times 2^-e -> 8 payload bytes (two dwords); a non-finite element becomes the NaN byte 0x7f
__device__ __forceinline__ uint2 kv8_narrow8(uint4 x, float inv) {
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
    unsigned o[2] = {0u, 0u};
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const float a = __uint_as_float(w[t] << 16) * inv, b = __uint_as_float(w[t] & 0xffff0000u) * inv;
        unsigned r = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
        if ((w[t] & 0x7f80u) == 0x7f80u) r = (r & 0xff00u) | 0x7fu;
        if ((w[t] & 0x7f800000u) == 0x7f800000u) r = (r & 0x00ffu) | 0x7f00u;
        o[t >> 1] |= r << (16 * (t & 1));
    }
    return make_uint2(o[0], o[1]);
}
// Eight consecutive lanes own one (row, K | V, head) block of 128 bf16 at src: lane c (0 .. 7) takes elements 16 c .. 16 c + 15 and stores
// their 16 payload bytes at pay + 16 c; lane 0 stores the scale.  Called by whole waves (shuffles): `active` switches the memory accesses.
__device__ __forceinline__ void kv8_quant_block(const bf16_t* src, unsigned char* pay, float* sc, int c, bool active) {
    uint4 x0 = make_uint4(0u, 0u, 0u, 0u), x1 = x0;
    if (active) {
        x0 = *reinterpret_cast<const uint4*>(src + c * 16);
        x1 = *reinterpret_cast<const uint4*>(src + c * 16 + 8);
    }
    unsigned m = kv8_amax8(x1, kv8_amax8(x0, 0u));
    m = max(m, (unsigned)__shfl_xor((int)m, 1, 64));
    m = max(m, (unsigned)__shfl_xor((int)m, 2, 64));
    m = max(m, (unsigned)__shfl_xor((int)m, 4, 64));
    const int e = kv8_scale_exp(m);
    const float inv = __uint_as_float((unsigned)(127 - e) << 23);
    const uint2 a = kv8_narrow8(x0, inv), b = kv8_narrow8(x1, inv);
    if (active) {
        *reinterpret_cast<uint4*>(pay + c * 16) = make_uint4(a.x, a.y, b.x, b.y);
        if (c == 0) *sc = __uint_as_float((unsigned)(e + 127) << 23);
    }
}

// ---- the widening half
typedef __attribute__((ext_vector_type(2))) float kv8fmt_f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned kv8fmt_u32x4;
typedef __attribute__((ext_vector_type(8))) short kv8fmt_bf16x8;
// four e4m3 bytes -> four bf16 (two dwords): v_cvt_pk_f32_fp8, then the upper halves of the two floats (the low 16 bits are zero)
__device__ __forceinline__ void kv8_widen4(unsigned w, unsigned& d0, unsigned& d1) {
    const kv8fmt_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    d0 = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
    d1 = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
}
__device__ __forceinline__ kv8fmt_bf16x8 kv8_widen8(uint2 w) {
    unsigned d0, d1, d2, d3;
    kv8_widen4(w.x, d0, d1);
    kv8_widen4(w.y, d2, d3);
    return __builtin_bit_cast(kv8fmt_bf16x8, (kv8fmt_u32x4){d0, d1, d2, d3});
}
// for a kernel that wants VALUES: 8 payload bytes times the block's scale -> 8 bf16 (v_cvt_pk_f32_fp8, the product in fp32,
// then the upper halves: a power of two times a 4-bit significand is exact in bf16 unless it is subnormal there; a NaN byte stays NaN)
__device__ __forceinline__ uint4 kv8_widen8_scaled(uint2 w, float sc) {
    const kv8fmt_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
    const kv8fmt_f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
    return make_uint4(__builtin_amdgcn_perm(__float_as_uint(a[1] * sc), __float_as_uint(a[0] * sc), 0x07060302u),
                      __builtin_amdgcn_perm(__float_as_uint(b[1] * sc), __float_as_uint(b[0] * sc), 0x07060302u),
                      __builtin_amdgcn_perm(__float_as_uint(c[1] * sc), __float_as_uint(c[0] * sc), 0x07060302u),
                      __builtin_amdgcn_perm(__float_as_uint(d[1] * sc), __float_as_uint(d[0] * sc), 0x07060302u));
}
