// The scalar tokenizer's arithmetic (scalar_tokenizer.py:28-63), one element at a time: shared by the tokenizer kernels (elementwise.hip:
// db1_mulaw_discretize / db1_mulaw_decode) and the action decoding kernels (action.hip: db1_obs_tokens / db1_select_actions), so that the
// ids and values of the two come out of the same instructions.
#pragma once
#include "db1_common.h"

// the denominator of the observation branch of mulaw_discretize_one and the base of the observation branch of mulaw_decode_one (host)
static inline float mulaw_den(float mu, float M) { return (float)log((double)(float)(mu * M + 1.0f)); }
static inline float mulaw_base(float mu, float M) { return (float)(1.0 + (double)M * (double)mu); }

// discretize: float32 op order of the reference with a correctly rounded logarithm (float64 log rounded once) -> ids identical to torch-CPU
__device__ __forceinline__ int mulaw_discretize_one(float v, int is_action, int nb, float mu, float den) {
    if (!is_action) {
        const float t = __fadd_rn(__fmul_rn(fabsf(v), mu), 1.0f);
        const float lg = (float)log((double)t);
        const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
        float y = __fdiv_rn(__fmul_rn(sg, lg), den);
        if (v != v) y = v;
        v = fminf(fmaxf(y, -1.f), 1.f);
    }
    const float z = __fmul_rn(__fdiv_rn(__fadd_rn(v, 1.0f), 2.0f), (float)nb);
    int id = (int)z;  // truncation toward zero, as torch .int()
    return id < 0 ? 0 : (id > nb - 1 ? nb - 1 : id);
}

// decode: id clipped to [0, nb - 1] (`bad` set when it was outside); x = id / nb * 2 - 1 in the reference's float32 op order; observations:
// sign(x) * (base^|x| - 1) / mu, the power taken in float64 and rounded once (within 1 ulp of torch's float32 pow)
__device__ __forceinline__ float mulaw_decode_one(long long id, int is_action, int nb, float mu, float base, int& bad) {
    if (id < 0 || id > nb - 1) { bad = 1; id = id < 0 ? 0 : nb - 1; }
    float x = __fsub_rn(__fmul_rn(__fdiv_rn((float)id, (float)nb), 2.0f), 1.0f);
    if (!is_action) {
        const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
        const float pw = (float)pow((double)base, (double)fabsf(x));
        x = __fdiv_rn(__fmul_rn(sg, __fsub_rn(pw, 1.0f)), mu);
    }
    return x;
}
