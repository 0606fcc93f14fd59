// The ring attention of relattn_decode.hip over an fp8 ring (include/db1_hip.h, "fp8 K/V ring"; tests/kv8_rule.py restates the format):
// a slot is H x 128 bytes of K payload (OCP e4m3fn), H x 128 bytes of V payload, H fp32 K scales, H fp32 V scales -- 264 H bytes against
// the 512 H of the bf16 slot.  The scales are powers of two, so everything the format adds to the arithmetic is exact, and the launch gives
// bit for bit what db1_relattn_decode_ring_fwd gives over the dequantised ring:
//   * same decomposition: a workgroup = one 16-query tile x one 128-key chunk, its four waves the chunk's four 32-key steps, merged through
//     LDS, then per chunk the partials / the second launch / the in-launch merge -- relattn_decode_ring_kernel's, by the same functions
//     (relattn_decode_step.h);
//   * memory keys (j < mlen): the payload is widened to bf16 in registers (exact: 3 mantissa bits into 7) and goes through the same MFMAs;
//     the K scale multiplies the fp32 score of its key before the relative term is added, the V scale multiplies the probability before it
//     is rounded to bf16 (l sums the unscaled probability, as it does there);
//   * the call's own keys (j >= mlen) are read as bf16 from qkv_new, like there, and appended to the ring QUANTISED: eight lanes hold one
//     (row, K | V, head), reduce its largest magnitude with three shuffles and store 16 payload bytes each.
// Loads: a (row, head) of payload is 128 contiguous bytes.  V: 16 bytes per lane, widened on the way into the same LDS tile [32][128] bf16
// (the transposed reads stay as they are).  K: the MFMA operand wants elements 32 ks + 8 g .. + 7 in lane (key a, group g), so 8 bytes per
// lane and k-step; regrouping them would reorder the products inside the MFMA and give other bits than the bf16 kernel.
#include "relattn_decode_step.h"
#include "kv8_format.h"

#define KV8_KC 128                                        // keys per workgroup: four 32-key steps, one per wave
#define KV8_WAVE_LDS (DEC_WAVE_LDS + 64 * 4)              // V tile + T scratch + the step's 32 K and 32 V scales

__global__ __launch_bounds__(256) void relattn_decode_ring_kv8_kernel(DecodeRingArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // blockIdx.x = chunk * (number of 16-query tiles) + tile -- every workgroup is ONE query tile against ONE 128-key chunk
    const int nqt = (p.q + 15) / 16;
    const int i0 = ((int)blockIdx.x % nqt) * 16;
    const int chunk = (int)blockIdx.x / nqt, h = blockIdx.y, b = blockIdx.z;
    const int a = lane & 15, g = lane >> 4;
    const int HD = p.H * DEC_D;
    const int64_t slot = (int64_t)264 * p.H;
    char* Vs = smem + wave * KV8_WAVE_LDS;
    float* Tw = reinterpret_cast<float*>(Vs + 32 * 256);
    float* Sc = Tw + 48 * 16;
    const int qi = i0 + a < p.q ? i0 + a : p.q - 1;  // rows beyond q repeat the last query (never stored)
    const bf16_t* qrow = p.qkv + ((int64_t)b * p.q + qi) * 3 * HD + h * DEC_D + g * 8;
    bf16x8_t qraw[4], uraw[4], vraw[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        qraw[ks] = *reinterpret_cast<const bf16x8_t*>(qrow + ks * 32);
        uraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.u + h * DEC_D + g * 8 + ks * 32);
        vraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.vb + h * DEC_D + g * 8 + ks * 32);
    }
    const int start = p.state[0];
    unsigned char* ringb = p.ring + (int64_t)b * p.cap * slot;
    const bf16_t* newkv = p.qkv + (int64_t)b * p.q * 3 * HD + HD + h * DEC_D;   // new row i: K at i * 3 HD, V at i * 3 HD + HD
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
            kv8_quant_block(newkv + (int64_t)(j - p.mlen) * 3 * HD + kv * HD, dst + kv * HD + h * DEC_D,
                            reinterpret_cast<float*>(dst + 2 * HD) + kv * p.H + h, (int)(threadIdx.x & 7), active);
        }
    }
    bf16x8_t fqu[4], fqv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        fqu[ks] = dec_add_bias(qraw[ks], uraw[ks]);
        fqv[ks] = dec_add_bias(qraw[ks], vraw[ks]);
    }
    auto mrow = [&](int j) -> const unsigned char* {   // the slot of memory key j (j < mlen)
        int r = start + j;
        r = r >= p.cap ? r - p.cap : r;
        return ringb + (int64_t)r * slot;
    };
    const bf16_t* Rg = p.R + h * DEC_D;
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
                vq[it] = *reinterpret_cast<const uint4*>(mrow(jr) + HD + h * DEC_D + ch * 16);
            }
#pragma unroll
            for (int blk = 0; blk < 2; blk++) {
                const int jr = j0 + 16 * blk + a < p.mlen ? j0 + 16 * blk + a : p.mlen - 1;
                const unsigned char* kr = mrow(jr) + h * DEC_D + g * 8;
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
        dec_rel_term(Tw, fqv, a, g, [&](int tb, int ks) { return rreg[tb][ks]; });
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
                const float v = (acc_s[blk][r] * ksc4[r] + dec_rel_read(Tw, a, bcol)) * p.scale;   // (the K scale: exact, a power of two)
                s[blk * 4 + r] = dec_visible(i, j0 + bcol, p.q, p.klen, p.mlen, p.shift) ? v : -1.0e30f;
                vsc[blk * 4 + r] = vsc4[r];
            }
        }
        const float alpha = dec_softmax_update(s, m_i, l_i);
#pragma unroll
        for (int t = 0; t < 8; t++) s[t] *= vsc[t];   // (the V scale, before the rounding; l sums the unscaled probability)
        dec_pv(acc_o, Vs, dec_pack_p(s), alpha, a, g);
    }
    // ---- the four waves' partial results (one 32-key step each) are merged here, through LDS, into ONE unit per chunk
    float o8[8], mx, lsum;
    dec_merge_waves<KV8_WAVE_LDS>(smem, acc_o, m_i, l_i, o8, mx, lsum);
    const bool inlaunch = p.tickets != nullptr;   // the merge over the chunks happens in this launch too: partials as write-through stores
    const int qt = threadIdx.x & 15, dg = (threadIdx.x >> 4) * 8;
    if (i0 + qt < p.q) dec_store_unit(p.part + dec_part_off(b, p.H, h, p.nunit, chunk, i0 + qt), dg, o8, mx, lsum, inlaunch);
    if (inlaunch) dec_inlaunch_merge(p, b, h, nqt, i0);
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
    kv8_quant_block(src + bk * DEC_D, slot + (kv * H + h) * DEC_D, reinterpret_cast<float*>(slot + 2 * H * DEC_D) + kv * H + h, (int)(threadIdx.x & 7), active);
}

extern "C" int64_t db1_kv8_slot_bytes(int H, int D) { return (D == DEC_D && H > 0 && H % 2 == 0) ? (int64_t)264 * H : 0; }

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
    DecodeRingArgs a;
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
    if (out && !a.tickets) return dec_launch_merge2(a.part, a.out, B, q, H, a.nunit, st);
    return DB1_OK;
}
