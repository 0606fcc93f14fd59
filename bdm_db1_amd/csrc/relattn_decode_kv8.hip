// The ring attention of relattn_decode.hip over an fp8 ring (include/db1_hip.h, "fp8 K/V ring"; tests/kv8_rule.py restates the format):
// a slot is H x 128 bytes of K payload (OCP e4m3fn), H x 128 bytes of V payload, H fp32 K scales, H fp32 V scales -- 264 H bytes against
// the 512 H of the bf16 slot.  The scales are powers of two, so everything the format adds to the arithmetic is exact, and the launch gives
// bit for bit what db1_relattn_decode_ring_fwd gives over the dequantised ring:
//   * same decomposition: a workgroup = one 16-query tile x one 128-key chunk, its four waves the chunk's four 32-key steps, merged through
//     LDS, then per chunk the partials / the second launch / the in-launch merge -- the arithmetic of relattn_decode_ring_kernel<true>;
//   * memory keys (j < mlen): the payload is widened to bf16 in registers (exact: 3 mantissa bits into 7) and goes through the same MFMAs;
//     the K scale multiplies the fp32 score of its key before the relative term is added, the V scale multiplies the probability before it
//     is rounded to bf16 (l sums the unscaled probability, as it does there);
//   * the call's own keys (j >= mlen) are read as bf16 from qkv_new, like there, and appended to the ring QUANTISED: eight lanes hold one
//     (row, K | V, head), reduce its largest magnitude with three shuffles and store 16 payload bytes each.
// Loads: a (row, head) of payload is 128 contiguous bytes.  V: 16 bytes per lane, widened on the way into the same LDS tile [32][128] bf16
// (the transposed reads stay as they are).  K: the MFMA operand wants elements 32 ks + 8 g .. + 7 in lane (key a, group g), so 8 bytes per
// lane and k-step; regrouping them would reorder the products inside the MFMA and give other bits than the bf16 kernel.
#include "db1_common.h"
#include "kv8_format.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float kv8_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 kv8_bf16x2;
typedef __attribute__((ext_vector_type(4))) unsigned kv8_u32x4;
#define LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))

#define KV8_D 128
#define KV8_KC 128                                        // keys per workgroup: four 32-key steps, one per wave
#define KV8_WAVE_LDS (32 * 256 + 48 * 16 * 4 + 64 * 4)    // V tile [32][128] bf16 + T scratch [48][16] f32 + the step's 32 K and 32 V scales

struct DecodeKv8Args {
    const bf16_t* qkv; const bf16_t* u; const bf16_t* vb; unsigned char* ring; const int* state; const bf16_t* R;
    float* part; bf16_t* out; unsigned* tickets;
    int B, q, klen, mlen, H, shift, nd, nunit, cap;
    float scale;
};

__device__ __forceinline__ unsigned kv8_pk(float lo, float hi) {
    kv8_f32x2 v = {lo, hi};
    kv8_bf16x2 r = __builtin_convertvector(v, kv8_bf16x2);
    return *reinterpret_cast<unsigned*>(&r);
}
__device__ __forceinline__ bf16x8_t kv8_add_bias(const bf16x8_t a, const bf16x8_t b) {
    union { unsigned u[4]; bf16x8_t v; } o;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const float x0 = __uint_as_float((unsigned)(unsigned short)a[2 * t] << 16) + __uint_as_float((unsigned)(unsigned short)b[2 * t] << 16);
        const float x1 = __uint_as_float((unsigned)(unsigned short)a[2 * t + 1] << 16) + __uint_as_float((unsigned)(unsigned short)b[2 * t + 1] << 16);
        o.u[t] = kv8_pk(x0, x1);
    }
    return o.v;
}
__device__ __forceinline__ void kv8_st_agent(float* p, float a, float b) {   // 8 bytes, write-through (sc1)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), ((unsigned long long)__float_as_uint(b) << 32) | __float_as_uint(a), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void kv8_ld_agent2(const float* p, float& a, float& b) {   // 8 bytes, L1-bypassing (sc1)
    const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a = __uint_as_float((unsigned)v); b = __uint_as_float((unsigned)(v >> 32));
}

// ---- the format
// four e4m3 bytes -> four bf16 (two dwords): v_cvt_pk_f32_fp8, then the upper halves of the two floats (the low 16 bits are zero)
__device__ __forceinline__ void kv8_widen4(unsigned w, unsigned& d0, unsigned& d1) {
    const kv8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    d0 = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
    d1 = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
}
__device__ __forceinline__ bf16x8_t kv8_widen8(uint2 w) {
    unsigned d0, d1, d2, d3;
    kv8_widen4(w.x, d0, d1);
    kv8_widen4(w.y, d2, d3);
    return __builtin_bit_cast(bf16x8_t, (kv8_u32x4){d0, d1, d2, d3});
}
// (the quantising half -- kv8_amax8, kv8_scale_exp, kv8_narrow8, kv8_quant_block -- lives in kv8_format.h: ring_prefill.hip writes slots too)

__global__ __launch_bounds__(256) void relattn_decode_ring_kv8_kernel(DecodeKv8Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // blockIdx.x = chunk * (number of 16-query tiles) + tile -- every workgroup is ONE query tile against ONE 128-key chunk
    const int nqt = (p.q + 15) / 16;
    const int i0 = ((int)blockIdx.x % nqt) * 16;
    const int chunk = (int)blockIdx.x / nqt, h = blockIdx.y, b = blockIdx.z;
    const int a = lane & 15, g = lane >> 4;
    const int HD = p.H * KV8_D;
    const int64_t slot = (int64_t)264 * p.H;
    char* Vs = smem + wave * KV8_WAVE_LDS;
    float* Tw = reinterpret_cast<float*>(Vs + 32 * 256);
    float* Sc = Tw + 48 * 16;
    const int qi = i0 + a < p.q ? i0 + a : p.q - 1;  // rows beyond q repeat the last query (never stored)
    const bf16_t* qrow = p.qkv + ((int64_t)b * p.q + qi) * 3 * HD + h * KV8_D + g * 8;
    bf16x8_t qraw[4], uraw[4], vraw[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        qraw[ks] = *reinterpret_cast<const bf16x8_t*>(qrow + ks * 32);
        uraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.u + h * KV8_D + g * 8 + ks * 32);
        vraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.vb + h * KV8_D + g * 8 + ks * 32);
    }
    const int start = p.state[0];
    unsigned char* ringb = p.ring + (int64_t)b * p.cap * slot;
    const bf16_t* newkv = p.qkv + (int64_t)b * p.q * 3 * HD + HD + h * KV8_D;   // new row i: K at i * 3 HD, V at i * 3 HD + HD
    if (i0 == 0) {   // append: the new keys / values of this chunk enter the ring quantised (one query tile of the chunk; all 256 threads)
        const int ja = chunk * KV8_KC > p.mlen ? chunk * KV8_KC : p.mlen, jb = (chunk + 1) * KV8_KC < p.klen ? (chunk + 1) * KV8_KC : p.klen;
        const int nblk = (jb - ja) * 2;                        // (row, K | V) blocks of this head, 32 per pass
        for (int base = 0; base < nblk; base += 32) {
            const int blk = base + (int)(threadIdx.x >> 3);
            const bool active = blk < nblk;
            const int j = ja + ((active ? blk : 0) >> 1), kv = blk & 1;
            int r = start + j;
            r = r >= p.cap ? r - p.cap : r;
            unsigned char* dst = ringb + (int64_t)r * slot;
            kv8_quant_block(newkv + (int64_t)(j - p.mlen) * 3 * HD + kv * HD, dst + kv * HD + h * KV8_D,
                            reinterpret_cast<float*>(dst + 2 * HD) + kv * p.H + h, (int)(threadIdx.x & 7), active);
        }
    }
    bf16x8_t fqu[4], fqv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        fqu[ks] = kv8_add_bias(qraw[ks], uraw[ks]);
        fqv[ks] = kv8_add_bias(qraw[ks], vraw[ks]);
    }
    auto mrow = [&](int j) -> const unsigned char* {   // the slot of memory key j (j < mlen)
        int r = start + j;
        r = r >= p.cap ? r - p.cap : r;
        return ringb + (int64_t)r * slot;
    };
    const bf16_t* Rg = p.R + h * KV8_D;
    f32x4 acc_o[8];
#pragma unroll
    for (int db = 0; db < 8; db++) acc_o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_i = -1.0e30f, l_i = 0.f;
    const int i = i0 + a;  // this lane's query
    const int j0 = chunk * KV8_KC + wave * 32;
    // (the step is skipped when it lies past klen or outside the window of every query of the tile: wave-uniform)
    if (j0 < p.klen && !(j0 > i0 + 15 + p.mlen || j0 + 31 <= i0 - p.shift)) {
        const bool has_mem = j0 < p.mlen, has_new = j0 + 31 >= p.mlen;   // (wave-uniform; rows past klen are clamped to klen - 1, a new row)
        // ---- every global load of the step is requested before the first use
        uint2 kq[2][4];
        uint4 vq[4];
        bf16x8_t rreg[3][4];
#pragma unroll
        for (int blk = 0; blk < 2; blk++)
#pragma unroll
            for (int ks = 0; ks < 4; ks++) kq[blk][ks] = make_uint2(0u, 0u);
#pragma unroll
        for (int it = 0; it < 4; it++) vq[it] = make_uint4(0u, 0u, 0u, 0u);   // (defined on both paths: they stay in registers)
        float sc = 1.f;
        if (has_mem) {
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int row = it * 8 + (lane >> 3), ch = lane & 7;
                const int jr = j0 + row < p.mlen ? j0 + row : p.mlen - 1;
                vq[it] = *reinterpret_cast<const uint4*>(mrow(jr) + HD + h * KV8_D + ch * 16);
            }
#pragma unroll
            for (int blk = 0; blk < 2; blk++) {
                const int jr = j0 + 16 * blk + a < p.mlen ? j0 + 16 * blk + a : p.mlen - 1;
                const unsigned char* kr = mrow(jr) + h * KV8_D + g * 8;
#pragma unroll
                for (int ks = 0; ks < 4; ks++) kq[blk][ks] = *reinterpret_cast<const uint2*>(kr + ks * 32);
            }
            const int js = j0 + (lane & 31);   // lanes 0 .. 31: the K scale of key j0 + lane, lanes 32 .. 63: the V scale of key j0 + lane - 32
            if (js < p.mlen) sc = *(reinterpret_cast<const float*>(mrow(js) + 2 * HD) + (lane >> 5) * p.H + h);
        }
        const int d_lo = p.mlen + i0 - j0 - 31;
        // (query a reads T rows a - bcol + 31 = a .. a + 31: the third block of 16 distances serves queries a >= 1 only.  With ONE query in the
        // tile -- every token step of a decoding loop -- it is not requested: a third of the R rows, which at fp8 are more lines than K and V)
        const bool wide = p.q - i0 > 1;
#pragma unroll
        for (int tb = 0; tb < 3; tb++) {
            int dr = d_lo + 16 * tb + a;
            dr = dr < 0 ? 0 : (dr > p.nd - 1 ? p.nd - 1 : dr);  // out-of-range distances belong to masked pairs
            const bf16_t* rr = Rg + (int64_t)dr * HD + g * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                rreg[tb][ks] = (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
                if (tb < 2 || wide) rreg[tb][ks] = *reinterpret_cast<const bf16x8_t*>(rr + ks * 32);
            }
        }
        // ---- the V tile [32][128] bf16 and the scales go to LDS, K to the MFMA operand registers
        Sc[lane] = sc;
        if (has_mem) {
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int row = it * 8 + (lane >> 3), ch = lane & 7;
                uint4 w0, w1;
                kv8_widen4(vq[it].x, w0.x, w0.y); kv8_widen4(vq[it].y, w0.z, w0.w);
                kv8_widen4(vq[it].z, w1.x, w1.y); kv8_widen4(vq[it].w, w1.z, w1.w);
                *reinterpret_cast<uint4*>(Vs + row * 256 + ch * 32) = w0;
                *reinterpret_cast<uint4*>(Vs + row * 256 + ch * 32 + 16) = w1;
            }
        }
        // ---- S^T[key][query] for the two 16-key blocks (the memory keys; rows of the call's own keys are replaced below)
        f32x4 acc_s[2];
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            acc_s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) acc_s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kv8_widen8(kq[blk][ks]), fqu[ks], acc_s[blk], 0, 0, 0);
        }
        // ---- relative term  ->  Tw[dist][query]
#pragma unroll
        for (int tb = 0; tb < 3; tb++) {
            f32x4 acc_t = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) acc_t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rreg[tb][ks], fqv[ks], acc_t, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r++) Tw[(16 * tb + 4 * g + r) * 16 + a] = acc_t[r];
        }
        if (has_new) {   // the call's own K / V rows of the step, bf16 as they are: requested only now, when the memory's K and the R registers
            // are free (one step per call and (batch, head) pays the round trip; held from the start they cost every step 64 registers and
            // a workgroup per CU).  Their score rows replace those computed above (a row of the MFMA depends on its own key only), their V
            // rows are stored over the clamped memory rows (LDS operations of a wave complete in order).
            uint4 vn[8];
            bf16x8_t kn[2][4];
#pragma unroll
            for (int blk = 0; blk < 2; blk++) {
                int jr = j0 + 16 * blk + a < p.klen ? j0 + 16 * blk + a : p.klen - 1;
                jr = jr < p.mlen ? p.mlen : jr;
                const bf16_t* kr = newkv + (int64_t)(jr - p.mlen) * 3 * HD + g * 8;
#pragma unroll
                for (int ks = 0; ks < 4; ks++) kn[blk][ks] = *reinterpret_cast<const bf16x8_t*>(kr + ks * 32);
            }
#pragma unroll
            for (int it = 0; it < 8; it++) {
                const int row = it * 4 + (lane >> 4), ch = lane & 15;
                int jr = j0 + row < p.klen ? j0 + row : p.klen - 1;
                jr = jr < p.mlen ? p.mlen : jr;
                vn[it] = *reinterpret_cast<const uint4*>(newkv + (int64_t)(jr - p.mlen) * 3 * HD + HD + ch * 8);
            }
#pragma unroll
            for (int blk = 0; blk < 2; blk++) {
                f32x4 acc_n = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ks++) acc_n = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kn[blk][ks], fqu[ks], acc_n, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) acc_s[blk][r] = j0 + 16 * blk + 4 * g + r >= p.mlen ? acc_n[r] : acc_s[blk][r];
            }
#pragma unroll
            for (int it = 0; it < 8; it++) {
                const int row = it * 4 + (lane >> 4), ch = lane & 15;
                if (j0 + row >= p.mlen) *reinterpret_cast<uint4*>(Vs + row * 256 + ch * 16) = vn[it];
            }
        }
        float s[8], vsc[8];
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            const f32x4 ksc4 = *reinterpret_cast<const f32x4*>(Sc + 16 * blk + 4 * g), vsc4 = *reinterpret_cast<const f32x4*>(Sc + 32 + 16 * blk + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int bcol = 16 * blk + 4 * g + r;  // key j0 + bcol
                const int j = j0 + bcol;
                const float v = (acc_s[blk][r] * ksc4[r] + Tw[(a - bcol + 31) * 16 + a]) * p.scale;   // (the K scale: exact, a power of two)
                const bool vis = (j < p.klen) && (j <= i + p.mlen) && (j > i - p.shift) && (i < p.q);
                s[blk * 4 + r] = vis ? v : -1.0e30f;
                vsc[blk * 4 + r] = vsc4[r];
            }
        }
        float mb = s[0];
#pragma unroll
        for (int t = 1; t < 8; t++) mb = fmaxf(mb, s[t]);
        mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
        mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
        const float m_new = fmaxf(m_i, mb);
        const float alpha = __expf(m_i - m_new);
        float rs = 0.f;
#pragma unroll
        for (int t = 0; t < 8; t++) { s[t] = s[t] > -1.0e29f ? __expf(s[t] - m_new) : 0.f; rs += s[t]; }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l_i = l_i * alpha + rs;
        m_i = m_new;
        union { unsigned u[4]; bf16x8_t v; } pb;
#pragma unroll
        for (int t = 0; t < 4; t++) pb.u[t] = kv8_pk(s[2 * t] * vsc[2 * t], s[2 * t + 1] * vsc[2 * t + 1]);   // (the V scale, before the rounding)
#pragma unroll
        for (int db = 0; db < 8; db++) {
            const int t16 = lane & 15;
            const char* base = Vs + (t16 >> 2) * 256 + (db * 16 + (t16 & 3) * 4) * 2;
            const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(bf16x4_t, const_cast<char*>(base) + (4 * g) * 256));
            const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(bf16x4_t, const_cast<char*>(base) + (16 + 4 * g) * 256));
            const bf16x8_t vt = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int r = 0; r < 4; r++) acc_o[db][r] *= alpha;
            acc_o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt, pb.v, acc_o[db], 0, 0, 0);
        }
    }
    // ---- the four waves' partial results (one 32-key step each) are merged here, through LDS, into ONE unit per chunk
    constexpr int OLD = KV8_D + 4;                       // floats per query row in LDS: O[128], m, l, pad
    float* mine = reinterpret_cast<float*>(Vs);          // (the wave's own V stage / T scratch, >= 16 rows x 132 floats: it is done with them)
#pragma unroll
    for (int db = 0; db < 8; db++) *reinterpret_cast<f32x4*>(mine + a * OLD + db * 16 + 4 * g) = acc_o[db];
    if (g == 0) { mine[a * OLD + KV8_D] = m_i; mine[a * OLD + KV8_D + 1] = l_i; }
    __syncthreads();
    const bool inlaunch = p.tickets != nullptr;   // the merge over the chunks happens in this launch too: partials as write-through stores
    {
        const int qi = threadIdx.x & 15, dg = (threadIdx.x >> 4) * 8;
        const float* w0p = reinterpret_cast<const float*>(smem) + qi * OLD;
        float mw[4], lw[4], mx = -1.0e30f;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            mw[w] = w0p[w * (KV8_WAVE_LDS / 4) + KV8_D]; lw[w] = w0p[w * (KV8_WAVE_LDS / 4) + KV8_D + 1];
            mx = fmaxf(mx, mw[w]);
        }
        float lsum_ = 0.f, o8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < 4; w++) {   // (waves in order: deterministic)
            const float wt = lw[w] > 0.f ? __expf(mw[w] - mx) : 0.f;
            lsum_ += lw[w] * wt;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(w0p + w * (KV8_WAVE_LDS / 4) + dg), hi = *reinterpret_cast<const f32x4*>(w0p + w * (KV8_WAVE_LDS / 4) + dg + 4);
#pragma unroll
            for (int j = 0; j < 4; j++) { o8[j] += lo[j] * wt; o8[4 + j] += hi[j] * wt; }
        }
        if (i0 + qi < p.q) {
            float* dst = p.part + ((((int64_t)b * p.H + h) * p.nunit + chunk) * 64 + i0 + qi) * (KV8_D + 2);
            if (inlaunch) {
#pragma unroll
                for (int j = 0; j < 8; j += 2) kv8_st_agent(dst + dg + j, o8[j], o8[j + 1]);
                if (dg == 0) kv8_st_agent(dst + KV8_D, mx, lsum_);
            } else {
#pragma unroll
                for (int j = 0; j < 8; j += 2) *reinterpret_cast<float2*>(dst + dg + j) = make_float2(o8[j], o8[j + 1]);
                if (dg == 0) { dst[KV8_D] = mx; dst[KV8_D + 1] = lsum_; }
            }
        }
    }
    if (!inlaunch) return;
    // ---- the chunk that finishes last for this (batch, head) merges the units (ticket counter, zero on entry and left zero); the hand-off
    // of relattn_decode_ring_kernel: write-through stores above, every wave drains them, one relaxed agent-scope ticket per workgroup, and
    // the merging workgroup reads the partials with L1-bypassing loads
    __shared__ unsigned ticket_s;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* tk = p.tickets + ((int64_t)b * p.H + h) * nqt + i0 / 16;
    if (threadIdx.x == 0) ticket_s = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (ticket_s != gridDim.x / nqt - 1) return;
    if (threadIdx.x == 0) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    {   // thread = (query qi of the tile, 8 output columns): all units' pieces are requested at once (<= 16 chunks: klen <= 2048), weighted in chunk order
        constexpr int NU = 16;
        const int qi = threadIdx.x & 15, dg = (threadIdx.x >> 4) * 8;
        const bool valid = i0 + qi < p.q;
        const float* src = p.part + ((((int64_t)b * p.H + h) * p.nunit) * 64 + (valid ? i0 + qi : i0)) * (KV8_D + 2);
        const int64_t cs = (int64_t)64 * (KV8_D + 2);
        float mlm[NU], mll[NU], ov[NU][8];
#pragma unroll
        for (int c = 0; c < NU; c++) {
            const float* u = src + (c < p.nunit ? c : p.nunit - 1) * cs;
            kv8_ld_agent2(u + KV8_D, mlm[c], mll[c]);
#pragma unroll
            for (int j = 0; j < 8; j += 2) kv8_ld_agent2(u + dg + j, ov[c][j], ov[c][j + 1]);
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
            *reinterpret_cast<uint4*>(p.out + ((int64_t)b * p.q + i0 + qi) * p.H * KV8_D + h * KV8_D + dg) = w;
        }
    }
}
// one 128-thread block per (query, head, batch): the arithmetic of relattn_decode_merge2_kernel
__global__ __launch_bounds__(128) void relattn_decode_kv8_merge_kernel(const float* __restrict__ part, bf16_t* __restrict__ out, int q, int H, int nunit) {
    __shared__ float wgt[64];
    __shared__ float red[2];
    const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
    const float* src = part + ((((int64_t)b * H + h) * nunit) * 64 + i) * (KV8_D + 2);
    const int64_t cs = (int64_t)64 * (KV8_D + 2);
    if (d < 64) {   // first wave: nunit <= 64 units
        const float m = d < nunit ? src[d * cs + KV8_D] : -1.0e30f;
        const float l = d < nunit ? src[d * cs + KV8_D + 1] : 0.f;
        float mx = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float w = l > 0.f ? __expf(m - mx) : 0.f;
        wgt[d] = w;
        float ls = l * w;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o, 64);
        if (d == 0) red[0] = ls;
    }
    __syncthreads();
    float o = 0.f;
#pragma unroll 8
    for (int c = 0; c < nunit; c++) o += src[c * cs + d] * wgt[c];   // (units in order: deterministic)
    const float l = red[0];
    out[((int64_t)b * q + i) * H * KV8_D + h * KV8_D + d] = f2bf(l > 0.f ? o / l : 0.f);
}

// src bf16 [n, mlen, 2, H, 128] -> slots at dst + row * dst_row_stride + pos * 264 H: one pass, eight lanes per (row, pos, K | V, head)
__global__ __launch_bounds__(256) void kv8_quantize_kernel(const bf16_t* __restrict__ src, unsigned char* __restrict__ dst, int64_t nblk, int mlen, int H,
                                                           int64_t dst_row_stride) {
    const int64_t blk = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool active = blk < nblk;
    const int64_t bk = active ? blk : 0;
    const int h = (int)(bk % H), kv = (int)((bk / H) & 1);
    const int64_t rp = bk / (2 * H);
    unsigned char* slot = dst + (rp / mlen) * dst_row_stride + (rp % mlen) * 264 * H;
    kv8_quant_block(src + bk * KV8_D, slot + (kv * H + h) * KV8_D, reinterpret_cast<float*>(slot + 2 * H * KV8_D) + kv * H + h, (int)(threadIdx.x & 7), active);
}

extern "C" int64_t db1_kv8_slot_bytes(int H, int D) { return (D == KV8_D && H > 0 && H % 2 == 0) ? (int64_t)264 * H : 0; }

extern "C" int db1_kv8_quantize_supported(int H, int D) { return db1_kv8_slot_bytes(H, D) > 0 && H <= 65535 ? 1 : 0; }

extern "C" int db1_kv8_quantize(const void* src, void* dst, int n, int mlen, int H, int D, int64_t dst_row_stride, void* stream) {
    if (!db1_kv8_quantize_supported(H, D)) DB1_FAIL(DB1_ERR_UNSUPPORTED, "kv8_quantize: needs d_head = 128 and an even number of heads (got H=%d D=%d)", H, D);
    if (n < 0 || mlen < 1 || !src || !dst || dst_row_stride < (int64_t)mlen * 264 * H)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "kv8_quantize: n=%d mlen=%d, a null buffer, or a destination row stride below mlen slots", n, mlen);
    if (!db1_aligned16(src) || !db1_aligned16(dst) || dst_row_stride % 16) DB1_FAIL(DB1_ERR_BAD_ALIGN, "kv8_quantize: operands and the row stride must be multiples of 16 bytes");
    const int64_t nblk = (int64_t)n * mlen * 2 * H;
    if (nblk == 0) return DB1_OK;
    if ((nblk + 31) / 32 > 0x7fffffffLL) DB1_FAIL(DB1_ERR_UNSUPPORTED, "kv8_quantize: too many rows for one launch");
    kv8_quantize_kernel<<<dim3((unsigned)((nblk + 31) / 32)), 256, 0, (hipStream_t)stream>>>((const bf16_t*)src, (unsigned char*)dst, nblk, mlen, H, dst_row_stride);
    DB1_CHECK_LAUNCH("kv8_quantize");
    return DB1_OK;
}

extern "C" int db1_relattn_decode_ring_kv8_supported(int B, int q, int klen, int H, int D) {
    return (db1_kv8_slot_bytes(H, D) > 0 && db1_relattn_decode_supported(B, q, klen, H, D, DB1_BF16) && klen <= 64 * 32) ? 1 : 0;
}
extern "C" int64_t db1_relattn_decode_ring_kv8_workspace_bytes(int B, int q, int klen, int H) {   // (the partials: one unit per 128-key chunk is used)
    return db1_relattn_decode_ring_workspace_bytes(B, q, klen, H);
}
extern "C" int db1_relattn_decode_ring_kv8_fwd(const void* qkv_new, const void* u, const void* vb, void* kv_ring, const int* ring_state, int cap, const void* R,
                                               int nd, void* out, int B, int q, int mlen, int H, int D, int shift, float scale, void* ws, int64_t ws_bytes,
                                               void* tickets, void* stream) {
    const int klen = mlen + q;
    if (!db1_relattn_decode_ring_kv8_supported(B, q, klen, H, D))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "relattn_decode_ring_kv8: needs d_head = 128, an even number of heads, 1 <= q <= 64, klen <= 2048 (got q=%d klen=%d H=%d D=%d)", q, klen, H, D);
    if (cap < klen || nd < 1 || !R || !ring_state || !kv_ring || !u || !vb || !qkv_new)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_decode_ring_kv8: ring capacity %d < klen %d, or null buffer", cap, klen);
    if (!db1_aligned16(qkv_new) || !db1_aligned16(kv_ring) || !db1_aligned16(R) || (out && !db1_aligned16(out)) || !db1_aligned16(u) || !db1_aligned16(vb))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "relattn_decode_ring_kv8: operands must be 16-byte aligned");
    DecodeKv8Args a;
    a.qkv = (const bf16_t*)qkv_new; a.u = (const bf16_t*)u; a.vb = (const bf16_t*)vb; a.ring = (unsigned char*)kv_ring; a.state = ring_state; a.R = (const bf16_t*)R;
    a.out = (bf16_t*)out; a.B = B; a.q = q; a.klen = klen; a.mlen = mlen; a.H = H; a.shift = shift; a.nd = nd; a.cap = cap; a.scale = scale;
    const int nchunk = (klen + KV8_KC - 1) / KV8_KC, nqt = (q + 15) / 16;
    a.tickets = ((int64_t)B * H * nqt <= 2048 && out) ? (unsigned*)tickets : nullptr;   // (the ticket buffer of db1_linear_decode_tickets_bytes)
    a.nunit = nchunk;
    DB1_NEED_WS(ws, ws_bytes, db1_relattn_decode_ring_kv8_workspace_bytes(B, q, klen, H), "relattn_decode_ring_kv8");
    a.part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    relattn_decode_ring_kv8_kernel<<<dim3((unsigned)(nchunk * nqt), (unsigned)H, (unsigned)B), 256, 4 * KV8_WAVE_LDS, st>>>(a);
    DB1_CHECK_LAUNCH("relattn_decode_ring_kv8");
    if (out && !a.tickets) {
        relattn_decode_kv8_merge_kernel<<<dim3((unsigned)q, (unsigned)H, (unsigned)B), 128, 0, st>>>(a.part, a.out, q, H, a.nunit);
        DB1_CHECK_LAUNCH("relattn_decode_kv8_merge");
    }
    return DB1_OK;
}
