// Relative-position attention for inference with Transformer-XL memory (evaluate_rl.py:157-266; transformer_xl.py:124-133,
// 160-225): 1 .. 64 new queries against klen = mlen + q cached keys / values (bf16, d_head = 128).
//     s[i,j] = ((q_i+u).k_j + (q_i+v).R[mlen+i-j]) / sqrt(d),   visible iff  i - shift < j <= i + mlen,   j in [0, klen)
// The materialised path ran two batched GEMMs, a softmax and another batched GEMM per layer on the generic strided kernel
// (135 us for P.V alone at q = 1); here one launch covers them, split over the keys ("flash decoding"):
//   grid = (key chunks of 64, heads, batch); the 4 waves of a workgroup are the 4 possible 16-query tiles (a wave whose tile
//   is empty exits); every wave is self-contained (own LDS: a 32-key V tile for the transposed reads + the skew scratch).
//   Per 32-key step and wave: S^T = K.Qu^T (2 x 4 v_mfma_f32_16x16x32_bf16, K fragments straight from global), the relative
//   term for the 47 distances the 16 x 32 block touches (3 x 4 MFMA against R rows) written to LDS [48 dist][16 q] and read
//   back skewed (element (a, a - b + 31)), online softmax (statistics lane-local + two cross-group shuffles), O^T += V^T.P^T
//   (8 MFMA; V^T via ds_read_b64_tr_b16 from the staged rows, with the key permutation that makes the S registers directly
//   the B operand: slots 0-3 = keys 4g..4g+3 of the first 16-key block, slots 4-7 = the same keys of the second).
//   Partials (m, l, O) per chunk go to a workspace; relattn_decode_merge_kernel combines them in chunk order.
// The step's arithmetic, shared with the fp8 ring kernel and the memory kernel, and the layout of the partials: relattn_decode_step.h.
#include "relattn_decode_step.h"

#define DEC_KC 64                        // keys per workgroup (two 32-key steps: the chunks, not the loop, provide the parallelism)

struct DecodeArgs {
    const bf16_t* qu; const bf16_t* qv; const bf16_t* k; const bf16_t* v; const bf16_t* R;
    float* part;   // [B][H][nchunk] units (relattn_decode_step.h)
    bf16_t* out;
    int64_t kv_rs, kv_bs;
    int B, q, klen, mlen, H, shift, nd, nchunk;
    float scale;
};

__global__ __launch_bounds__(256) void relattn_decode_kernel(DecodeArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = wave * 16;
    if (i0 >= p.q) return;  // waves are independent: no workgroup barrier below
    const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int a = lane & 15, g = lane >> 4;
    const int HD = p.H * DEC_D;
    char* Vs = smem + wave * DEC_WAVE_LDS;
    float* Tw = reinterpret_cast<float*>(Vs + 32 * 256);
    const int qi = i0 + a < p.q ? i0 + a : p.q - 1;  // rows beyond q repeat the last query (never stored)
    const bf16_t* qu = p.qu + ((int64_t)b * p.q + qi) * HD + h * DEC_D + g * 8;
    const bf16_t* qv = p.qv + ((int64_t)b * p.q + qi) * HD + h * DEC_D + g * 8;
    bf16x8_t fqu[4], fqv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        fqu[ks] = *reinterpret_cast<const bf16x8_t*>(qu + ks * 32);
        fqv[ks] = *reinterpret_cast<const bf16x8_t*>(qv + ks * 32);
    }
    const bf16_t* kg = p.k + (int64_t)b * p.kv_bs + h * DEC_D;
    const bf16_t* vg = p.v + (int64_t)b * p.kv_bs + h * DEC_D;
    const bf16_t* Rg = p.R + h * DEC_D;
    f32x4 acc_o[8];
#pragma unroll
    for (int db = 0; db < 8; db++) acc_o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_i = -1.0e30f, l_i = 0.f;
    const int i = i0 + a;  // this lane's query
    const int jc0 = chunk * DEC_KC;
    for (int st = 0; st < DEC_KC / 32; st++) {
        const int j0 = jc0 + st * 32;
        if (j0 >= p.klen) break;
        // whole step outside the window of every query of the tile?  (wave-uniform)
        if (j0 > i0 + 15 + p.mlen || j0 + 31 <= i0 - p.shift) continue;
        // ---- stage V rows j0 .. j0+31 (rows past klen are clamped: their probabilities are exactly zero)
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int row = it * 4 + (lane >> 4), ch = lane & 15;
            const int jr = j0 + row < p.klen ? j0 + row : p.klen - 1;
            const uint4 val = *reinterpret_cast<const uint4*>(vg + (int64_t)jr * p.kv_rs + ch * 8);
            *reinterpret_cast<uint4*>(Vs + row * 256 + ch * 16) = val;
        }
        // ---- S^T[key][query] for the two 16-key blocks
        f32x4 acc_s[2];
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            acc_s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int jr = j0 + 16 * blk + a < p.klen ? j0 + 16 * blk + a : p.klen - 1;
            const bf16_t* kr = kg + (int64_t)jr * p.kv_rs + g * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ks++)
                acc_s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(kr + ks * 32), fqu[ks], acc_s[blk], 0, 0, 0);
        }
        // ---- relative term: distances d_lo .. d_lo+47 with d_lo = mlen + i0 - j0 - 31  ->  Tw[dist][query], R rows straight from global
        const int d_lo = p.mlen + i0 - j0 - 31;
        dec_rel_term(Tw, fqv, a, g, [&](int tb, int ks) {
            int dr = d_lo + 16 * tb + a;
            dr = dr < 0 ? 0 : (dr > p.nd - 1 ? p.nd - 1 : dr);  // out-of-range distances belong to masked pairs
            return *reinterpret_cast<const bf16x8_t*>(Rg + (int64_t)dr * HD + g * 8 + ks * 32);
        });
        float s[8];
#pragma unroll
        for (int blk = 0; blk < 2; blk++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int bcol = 16 * blk + 4 * g + r;  // key j0 + bcol
                const float v = (acc_s[blk][r] + dec_rel_read(Tw, a, bcol)) * p.scale;
                s[blk * 4 + r] = dec_visible(i, j0 + bcol, p.q, p.klen, p.mlen, p.shift) ? v : -1.0e30f;
            }
        const float alpha = dec_softmax_update(s, m_i, l_i);
        dec_pv(acc_o, Vs, dec_pack_p(s), alpha, a, g);
    }
    // ---- partial results of this chunk: lane holds query a, d = db*16 + 4g + r
    if (i < p.q) {
        float* dst = p.part + dec_part_off(b, p.H, h, p.nchunk, chunk, i);
#pragma unroll
        for (int db = 0; db < 8; db++)
            *reinterpret_cast<float2*>(dst + db * 16 + 4 * g) = make_float2(acc_o[db][0], acc_o[db][1]),
            *reinterpret_cast<float2*>(dst + db * 16 + 4 * g + 2) = make_float2(acc_o[db][2], acc_o[db][3]);
        if (g == 0) { dst[DEC_D] = m_i; dst[DEC_D + 1] = l_i; }
    }
}

// one 128-thread block per (query, head, batch): combine the chunk partials in chunk order
__global__ __launch_bounds__(128) void relattn_decode_merge_kernel(DecodeArgs p) {
    const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
    const float* src = p.part + dec_part_off(b, p.H, h, p.nchunk, 0, i);
    const int64_t cs = DEC_PART_UNIT;
    float m = -1.0e30f;
    for (int c = 0; c < p.nchunk; c++) m = fmaxf(m, src[c * cs + DEC_D]);
    float l = 0.f, o = 0.f;
    for (int c = 0; c < p.nchunk; c++) {
        const float lc = src[c * cs + DEC_D + 1];
        if (lc > 0.f) {
            const float w = __expf(src[c * cs + DEC_D] - m);
            l += lc * w;
            o += src[c * cs + d] * w;
        }
    }
    p.out[((int64_t)b * p.q + i) * p.H * DEC_D + h * DEC_D + d] = f2bf(l > 0.f ? o / l : 0.f);
}

// ======================================================================================= ring variant (hipGraph-friendly inference)
// The K / V of the memory live in a ring [B, cap, 2, H, D] (cap >= mlen + q): logical key j < mlen is ring row (start + j) % cap, the
// q new keys / values are read from the packed projections of this call, qkv_new [B, q, 3, H, D], and copied into ring rows
// (start + mlen + i) % cap by the workgroups that visit them -- so a call appends in place instead of concatenating 8 MB per layer, and
// `start` is a DEVICE scalar (advanced by db1_ring_advance after the last layer): the same captured graph serves every call.
// q + u and q + v are formed here from qkv_new (rounded to bf16 like db1_relattn_add_head_bias does).
// A workgroup = one 16-query tile x one 128-key chunk, its four waves are the chunk's four 32-key steps, merged through LDS into one
// partial per (tile, chunk).  (An earlier form -- a wave is one of four 16-query tiles and walks the chunk's steps itself -- took 38.6 us
// per launch at q = 22 against 8.8 us at q = 1: four dependent rounds of loads per wave.)
#define DECR_KC 128
__global__ __launch_bounds__(256) void relattn_decode_ring_kernel(DecodeRingArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // blockIdx.x = chunk * (number of 16-query tiles) + tile -- every workgroup is ONE query tile against ONE 128-key chunk
    const int nqt = (p.q + 15) / 16;
    const int i0 = ((int)blockIdx.x % nqt) * 16;
    const int chunk = (int)blockIdx.x / nqt, h = blockIdx.y, b = blockIdx.z;
    const int a = lane & 15, g = lane >> 4;
    const int HD = p.H * DEC_D;
    char* Vs = smem + wave * DEC_WAVE_LDS;
    float* Tw = reinterpret_cast<float*>(Vs + 32 * 256);
    const int qi = i0 + a < p.q ? i0 + a : p.q - 1;  // rows beyond q repeat the last query (never stored)
    const bf16_t* qrow = p.qkv + ((int64_t)b * p.q + qi) * 3 * HD + h * DEC_D + g * 8;
    // (requested before the append so that they travel while the ring origin arrives and the new rows are copied)
    bf16x8_t qraw[4], uraw[4], vraw[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        qraw[ks] = *reinterpret_cast<const bf16x8_t*>(qrow + ks * 32);
        uraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.u + h * DEC_D + g * 8 + ks * 32);
        vraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.vb + h * DEC_D + g * 8 + ks * 32);
    }
    {   // append: the new keys / values of this chunk enter the ring (all 256 threads; 32 sixteen-byte pieces per row and head)
        const int start_ = p.state[0];
        const int ja = chunk * DECR_KC > p.mlen ? chunk * DECR_KC : p.mlen, jb = (chunk + 1) * DECR_KC < p.klen ? (chunk + 1) * DECR_KC : p.klen;
        const bf16_t* nk = p.qkv + (int64_t)b * p.q * 3 * HD + HD + h * DEC_D;
        bf16_t* rg = reinterpret_cast<bf16_t*>(p.ring) + (int64_t)b * p.cap * 2 * HD + h * DEC_D;
        for (int idx = threadIdx.x; idx < (i0 == 0 ? (jb - ja) * 32 : 0); idx += 256) {   // (one query tile of the chunk copies)
            const int j = ja + (idx >> 5), pc = idx & 31;          // piece 0..15: K, 16..31: V
            int r = start_ + j;
            r = r >= p.cap ? r - p.cap : r;
            *reinterpret_cast<uint4*>(rg + (int64_t)r * 2 * HD + (pc >> 4) * HD + (pc & 15) * 8) =
                *reinterpret_cast<const uint4*>(nk + (int64_t)(j - p.mlen) * 3 * HD + (pc >> 4) * HD + (pc & 15) * 8);
        }
    }
    if (i0 >= p.q) return;  // (never taken: i0 = 16 tile < q; a workgroup-uniform exit, so the barriers below stay whole)
    bf16x8_t fqu[4], fqv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        fqu[ks] = dec_add_bias(qraw[ks], uraw[ks]);
        fqv[ks] = dec_add_bias(qraw[ks], vraw[ks]);
    }
    const int start = p.state[0];
    const bf16_t* ring = reinterpret_cast<const bf16_t*>(p.ring) + (int64_t)b * p.cap * 2 * HD + h * DEC_D;   // row r: K at r * 2 HD, V at r * 2 HD + HD
    const bf16_t* newkv = p.qkv + (int64_t)b * p.q * 3 * HD + HD + h * DEC_D;  // new row i: K at i * 3 HD, V at i * 3 HD + HD
    // K row of logical key j (V: + HD); j clamped by the caller.  A select, not a branch: with a divergent if / else around them the
    // compiler issued the 28 loads of a step one round trip at a time (14.6 us per launch at q = 1, almost all of it memory latency)
    auto krow = [&](int j) -> const bf16_t* {
        int r = start + j;
        r = r >= p.cap ? r - p.cap : r;
        const int64_t off_ring = (int64_t)r * 2 * HD, off_new = (int64_t)(j - p.mlen) * 3 * HD;
        const bf16_t* base = j >= p.mlen ? newkv : ring;
        return base + (j >= p.mlen ? off_new : off_ring);
    };
    const bf16_t* Rg = p.R + h * DEC_D;
    f32x4 acc_o[8];
#pragma unroll
    for (int db = 0; db < 8; db++) acc_o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_i = -1.0e30f, l_i = 0.f;
    const int i = i0 + a;  // this lane's query
    const int jc0 = chunk * DECR_KC;
    // (one step per wave, st = wave.  Kept in the shape of a loop: as one `if` the compiler schedules the step's prologue differently and a
    // launch at q = 1 took 6.9 us instead of 6.7 us)
    for (int st = wave; st < wave + 1; st++) {
        const int j0 = jc0 + st * 32;
        if (j0 >= p.klen) break;
        if (j0 > i0 + 15 + p.mlen || j0 + 31 <= i0 - p.shift) continue;   // whole step outside the window of every query of the tile (wave-uniform)
        // ---- every global load of the step is requested before the first use: V rows j0 .. j0+31 (rows past klen are clamped: their
        // probabilities are exactly zero), the two 16-key K blocks and the three 16-distance R blocks (d_lo = mlen + i0 - j0 - 31)
        uint4 vreg[8];
        bf16x8_t kreg[2][4], rreg[3][4];
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int row = it * 4 + (lane >> 4), ch = lane & 15;
            const int jr = j0 + row < p.klen ? j0 + row : p.klen - 1;
            vreg[it] = *reinterpret_cast<const uint4*>(krow(jr) + HD + ch * 8);
        }
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            const int jr = j0 + 16 * blk + a < p.klen ? j0 + 16 * blk + a : p.klen - 1;
            const bf16_t* kr = krow(jr) + g * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) kreg[blk][ks] = *reinterpret_cast<const bf16x8_t*>(kr + ks * 32);
        }
        const int d_lo = p.mlen + i0 - j0 - 31;
#pragma unroll
        for (int tb = 0; tb < 3; tb++) {
            int dr = d_lo + 16 * tb + a;
            dr = dr < 0 ? 0 : (dr > p.nd - 1 ? p.nd - 1 : dr);  // out-of-range distances belong to masked pairs
            const bf16_t* rr = Rg + (int64_t)dr * HD + g * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) rreg[tb][ks] = *reinterpret_cast<const bf16x8_t*>(rr + ks * 32);
        }
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int row = it * 4 + (lane >> 4), ch = lane & 15;
            *reinterpret_cast<uint4*>(Vs + row * 256 + ch * 16) = vreg[it];
        }
        // ---- S^T[key][query] for the two 16-key blocks
        f32x4 acc_s[2];
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            acc_s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) acc_s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kreg[blk][ks], fqu[ks], acc_s[blk], 0, 0, 0);
        }
        // ---- relative term  ->  Tw[dist][query].  From here to the end of the step this kernel keeps its OWN COPY of dec_rel_term, dec_visible,
        // dec_softmax_update and dec_pv (relattn_decode_step.h; the fp8 kernel calls them): through the functions the compiler scheduled the
        // step differently and generation at 16 and 64 rows took 2 - 4 % longer per token.  Keep the order of operations equal to theirs.
#pragma unroll
        for (int tb = 0; tb < 3; tb++) {
            f32x4 acc_t = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) acc_t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rreg[tb][ks], fqv[ks], acc_t, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r++) Tw[(16 * tb + 4 * g + r) * 16 + a] = acc_t[r];
        }
        float s[8];
#pragma unroll
        for (int blk = 0; blk < 2; blk++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int bcol = 16 * blk + 4 * g + r;  // key j0 + bcol
                const int j = j0 + bcol;
                const float v = (acc_s[blk][r] + Tw[(a - bcol + 31) * 16 + a]) * p.scale;
                const bool vis = (j < p.klen) && (j <= i + p.mlen) && (j > i - p.shift) && (i < p.q);
                s[blk * 4 + r] = vis ? v : -1.0e30f;
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
        for (int t = 0; t < 4; t++) pb.u[t] = f2bf_pk(s[2 * t], s[2 * t + 1]);
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
    // ---- the four waves' partial results (one 32-key step each) are merged here, through LDS, into ONE unit per chunk (every wave reaches
    // this point: a skipped step contributes (0, -1e30, 0))
    float o8[8], mx, lsum;
    dec_merge_waves<DEC_WAVE_LDS>(smem, acc_o, m_i, l_i, o8, mx, lsum);
    const bool inlaunch = p.tickets != nullptr;   // the merge over the chunks happens in this launch too: partials as write-through stores
    const int qt = threadIdx.x & 15, dg = (threadIdx.x >> 4) * 8;
    if (i0 + qt < p.q) dec_store_unit(p.part + dec_part_off(b, p.H, h, p.nunit, chunk, i0 + qt), dg, o8, mx, lsum, inlaunch);
    if (inlaunch) dec_inlaunch_merge(p, b, h, nqt, i0);
}
// one 128-thread block per (query, head, batch): the units' (m, l) first (independent loads, weights through LDS), then the weighted sum
__global__ __launch_bounds__(128) void relattn_decode_merge2_kernel(const float* __restrict__ part, bf16_t* __restrict__ out, int q, int H, int nunit) {
    __shared__ float wgt[64];
    __shared__ float red[2];
    const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
    const float* src = part + dec_part_off(b, H, h, nunit, 0, i);
    const int64_t cs = DEC_PART_UNIT;
    if (d < 64) {   // first wave: nunit <= 64 units
        const float m = d < nunit ? src[d * cs + DEC_D] : -1.0e30f;
        const float l = d < nunit ? src[d * cs + DEC_D + 1] : 0.f;
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
    out[((int64_t)b * q + i) * H * DEC_D + h * DEC_D + d] = f2bf(l > 0.f ? o / l : 0.f);
}
int dec_launch_merge2(const float* part, bf16_t* out, int B, int q, int H, int nunit, hipStream_t st) {
    relattn_decode_merge2_kernel<<<dim3((unsigned)q, (unsigned)H, (unsigned)B), 128, 0, st>>>(part, out, q, H, nunit);
    DB1_CHECK_LAUNCH("relattn_decode_merge2");
    return DB1_OK;
}
__global__ void ring_advance_kernel(int* state, int q, int cap) { int s = state[0] + q; state[0] = s >= cap ? s - cap : s; }

extern "C" int db1_ring_advance(int* state, int q, int cap, void* stream) {
    if (!state || q < 0 || cap <= 0) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_advance");
    ring_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state, q, cap);
    DB1_CHECK_LAUNCH("ring_advance");
    return DB1_OK;
}
extern "C" int64_t db1_relattn_decode_ring_workspace_bytes(int B, int q, int klen, int H) {
    (void)q;
    return (int64_t)B * H * ((klen + 31) / 32) * DEC_PART_UNIT * (int64_t)sizeof(float);
}
extern "C" int db1_relattn_decode_ring_fwd(const void* qkv_new, const void* u, const void* vb, void* kv_ring, const int* ring_state, int cap, const void* R,
                                           int nd, void* out, int B, int q, int mlen, int H, int D, int shift, float scale, void* ws, int64_t ws_bytes,
                                           void* tickets, void* stream) {
    const int klen = mlen + q;
    if (!db1_relattn_decode_supported(B, q, klen, H, D, DB1_BF16) || klen > 64 * 32)
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "relattn_decode_ring: needs bf16, d_head = 128, 1 <= q <= 64, klen <= 2048 (got q=%d klen=%d D=%d)", q, klen, D);
    if (cap < klen || nd < 1 || !R || !ring_state || !kv_ring || !u || !vb) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_decode_ring: ring capacity %d < klen %d, or null buffer", cap, klen);
    if (!db1_aligned16(qkv_new) || !db1_aligned16(kv_ring) || !db1_aligned16(R) || (out && !db1_aligned16(out)) || !db1_aligned16(u) || !db1_aligned16(vb))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "relattn_decode_ring: operands must be 16-byte aligned");
    DecodeRingArgs a;
    a.qkv = (const bf16_t*)qkv_new; a.u = (const bf16_t*)u; a.vb = (const bf16_t*)vb; a.ring = (unsigned char*)kv_ring; a.state = ring_state; a.R = (const bf16_t*)R;
    a.out = (bf16_t*)out; a.B = B; a.q = q; a.klen = klen; a.mlen = mlen; a.H = H; a.shift = shift; a.nd = nd; a.cap = cap; a.scale = scale;
    const int nchunk = (klen + DECR_KC - 1) / DECR_KC, nqt = (q + 15) / 16;
    a.tickets = ((int64_t)B * H * nqt <= 2048 && out) ? (unsigned*)tickets : nullptr;   // (the ticket buffer of db1_linear_decode_tickets_bytes)
    a.nunit = nchunk;   // (the four waves of a workgroup are merged inside it)
    DB1_NEED_WS(ws, ws_bytes, db1_relattn_decode_ring_workspace_bytes(B, q, klen, H), "relattn_decode_ring");
    a.part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    relattn_decode_ring_kernel<<<dim3((unsigned)(nchunk * nqt), (unsigned)H, (unsigned)B), 256, 4 * DEC_WAVE_LDS, st>>>(a);
    DB1_CHECK_LAUNCH("relattn_decode_ring");
    if (out && !a.tickets) return dec_launch_merge2(a.part, a.out, B, q, H, a.nunit, st);
    return DB1_OK;
}

extern "C" int db1_relattn_decode_supported(int B, int q, int klen, int H, int D, int dt) {
    return (dt == DB1_BF16 && D == DEC_D && B > 0 && H > 0 && q >= 1 && q <= 64 && klen >= q && B <= 65535 && H <= 65535) ? 1 : 0;
}

extern "C" int64_t db1_relattn_decode_workspace_bytes(int B, int q, int klen, int H) {  // per (b, h, key chunk): 64 rows x (out, max, sum)
    (void)q;
    return (int64_t)B * H * ((klen + DEC_KC - 1) / DEC_KC) * DEC_PART_UNIT * (int64_t)sizeof(float);
}

extern "C" int db1_relattn_decode_fwd(const void* qu, const void* qv, const void* k, const void* v, int64_t kv_row_stride,
                                      int64_t kv_batch_stride, const void* R, int nd, void* out, int B, int q, int klen, int mlen, int H,
                                      int D, int shift, float scale, void* ws, int64_t ws_bytes, void* stream) {
    if (!db1_relattn_decode_supported(B, q, klen, H, D, DB1_BF16))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "relattn_decode: needs bf16, d_head = 128, 1 <= q <= 64 (got q=%d klen=%d D=%d)", q, klen, D);
    if (mlen != klen - q) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_decode: klen (%d) must be mlen (%d) + q (%d)", klen, mlen, q);
    if (nd < 1 || !R) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_decode: R rows");
    if ((kv_row_stride % 8) || (kv_batch_stride % 8) || !db1_aligned16(qu) || !db1_aligned16(qv) || !db1_aligned16(k) || !db1_aligned16(v) ||
        !db1_aligned16(R) || !db1_aligned16(out))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "relattn_decode: operands must be 16-byte aligned, strides multiples of 8 elements");
    DecodeArgs a;
    a.qu = (const bf16_t*)qu; a.qv = (const bf16_t*)qv; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.R = (const bf16_t*)R;
    a.out = (bf16_t*)out; a.kv_rs = kv_row_stride; a.kv_bs = kv_batch_stride;
    a.B = B; a.q = q; a.klen = klen; a.mlen = mlen; a.H = H; a.shift = shift; a.nd = nd; a.scale = scale;
    a.nchunk = (klen + DEC_KC - 1) / DEC_KC;
    DB1_NEED_WS(ws, ws_bytes, db1_relattn_decode_workspace_bytes(B, q, klen, H), "relattn_decode");
    a.part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    relattn_decode_kernel<<<dim3((unsigned)a.nchunk, (unsigned)H, (unsigned)B), 256, 4 * DEC_WAVE_LDS, st>>>(a);
    DB1_CHECK_LAUNCH("relattn_decode");
    relattn_decode_merge_kernel<<<dim3((unsigned)q, (unsigned)H, (unsigned)B), 128, 0, st>>>(a);
    DB1_CHECK_LAUNCH("relattn_decode_merge");
    return DB1_OK;
}

// ======================================================================================= grouped variant (beam search / best-of-n sampling)
// The M = G W rows of a beam search or a best-of-n sampling share their group's prompt: ONE base ring row per group [G, cap_b, 2, H, D]
// (filled by the prefill, never moved while decoding) and a short tail ring per row [M, cap_t, 2, H, D] with the keys the row generated
// itself (the rule: include/db1_hip.h, "grouped K/V ring"; tests/group_ring_rule.py).  One new token per row (q = 1), one launch of
//   shared units  (128 base positions, head, group, 16-row tile of the group): the chunk's K / V are loaded ONCE, the MFMA's 16 query columns
//                 are the rows g W + 16 tile + a (columns past W repeat the last row, never stored).  Every column is query 0, so a key's
//                 distance is the same in all columns: the relative term is R[dist(key)] . (q + v) accumulated onto K . (q + u) by the same
//                 accumulator -- 32 R rows per 32-key step, no LDS scratch, no skewed read-back.
//   private units (128 tail positions, head, row): the ring kernel's q = 1 form over the row's own tail and the call's own key, which the
//                 unit that holds tail position Lt appends.
// A workgroup's four waves are its four 32-position steps, merged through LDS as in the ring kernel; a step outside [first, last] visible
// position loads nothing.  Partials: [G][H][nunit][64][D + 2] with (G, W) in the place of (B, q) and the units in the order (shared chunks by
// position, private chunks by position): relattn_decode_merge2_kernel merges them in that fixed order.
struct DecodeGroupArgs {
    const bf16_t* qkv; const bf16_t* u; const bf16_t* vb; const bf16_t* base; const int* state_b; bf16_t* tail; const int* state_t; const int* n_tail;
    const bf16_t* R; float* part; int* status;
    int G, W, mlen, Lt, H, shift, nd, nunit, nb, ntile, cap_b, cap_t;
    float scale;
};
template <bool PRIV>
__device__ __forceinline__ void decode_group_unit(const DecodeGroupArgs& p, char* smem, const int chunk, const int sub, const int sb, const int st_, const int ntl) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y, grp = blockIdx.z;
    const int a = lane & 15, lg = lane >> 4;
    const int HD = p.H * DEC_D;
    char* Vs = smem + wave * DEC_WAVE_LDS;
    // PRIV: sub = the row inside the group, every column is that row.  Shared: sub = the 16-row tile, column a is row 16 sub + a (clamped)
    const int wq = PRIV ? sub : (16 * sub + a < p.W ? 16 * sub + a : p.W - 1);
    const int64_t row = (int64_t)grp * p.W + wq;
    const bf16_t* qrow = p.qkv + row * 3 * HD + h * DEC_D + lg * 8;
    bf16x8_t qraw[4], uraw[4], vraw[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        qraw[ks] = *reinterpret_cast<const bf16x8_t*>(qrow + ks * 32);
        uraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.u + h * DEC_D + lg * 8 + ks * 32);
        vraw[ks] = *reinterpret_cast<const bf16x8_t*>(p.vb + h * DEC_D + lg * 8 + ks * 32);
    }
    // positions: shared -- base position x in [ntl, mlen) is logical key x - ntl; private -- tail position x in [Lt - ntl, Lt] is logical key
    // x - Lt + mlen (x == Lt: the call's own key).  lo .. hi are the positions inside the window; the distance of logical key j is mlen - j.
    const int lo = PRIV ? p.Lt - ntl : ntl, hi = PRIV ? p.Lt : p.mlen - 1;
    const int joff = PRIV ? p.mlen - p.Lt : -ntl;
    const bf16_t* newkv = p.qkv + row * 3 * HD + HD + h * DEC_D;       // (private only) K of the call's own key, V at + HD
    if (PRIV && chunk == p.Lt / DECR_KC && threadIdx.x < 32) {           // append: 16 sixteen-byte pieces of K, 16 of V
        int r = st_ + p.Lt;
        r = r >= p.cap_t ? r - p.cap_t : r;
        const int pc = threadIdx.x;
        *reinterpret_cast<uint4*>(p.tail + (row * p.cap_t + r) * 2 * HD + h * DEC_D + (pc >> 4) * HD + (pc & 15) * 8) =
            *reinterpret_cast<const uint4*>(newkv + (pc >> 4) * HD + (pc & 15) * 8);
    }
    // K row of position x (V: + HD), x clamped into [lo, hi] by the caller: a slot outside the window is never read (it may hold anything).
    // A select between the sources, not a branch (the ring kernel's comment records what the branch cost).
    const bf16_t* ringrow = PRIV ? p.tail + row * p.cap_t * 2 * HD + h * DEC_D : p.base + (int64_t)grp * p.cap_b * 2 * HD + h * DEC_D;
    const int origin = PRIV ? st_ : sb, cap = PRIV ? p.cap_t : p.cap_b;
    auto krow = [&](int x) -> const bf16_t* {
        int r = origin + x;
        r = r >= cap ? r - cap : r;
        const bf16_t* ringp = ringrow + (int64_t)r * 2 * HD;
        return (PRIV && x == p.Lt) ? newkv : ringp;
    };
    const bf16_t* Rg = p.R + h * DEC_D;
    f32x4 acc_o[8];
#pragma unroll
    for (int db = 0; db < 8; db++) acc_o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_i = -1.0e30f, l_i = 0.f;
    const int x0 = chunk * DECR_KC + wave * 32;
    if (lo <= hi && x0 <= hi && x0 + 31 >= lo) {   // (wave-uniform) a step outside the window loads nothing and contributes (0, -1e30, 0)
        bf16x8_t fqu[4], fqv[4];
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            fqu[ks] = dec_add_bias(qraw[ks], uraw[ks]);
            fqv[ks] = dec_add_bias(qraw[ks], vraw[ks]);
        }
        // ---- every global load of the step is requested before the first use: 32 V rows, two 16-key K blocks, two 16-distance R blocks
        uint4 vreg[8];
        bf16x8_t kreg[2][4], rreg[2][4];
#pragma unroll
        for (int it = 0; it < 8; it++) {
            int x = x0 + it * 4 + (lane >> 4);
            x = x < lo ? lo : (x > hi ? hi : x);
            vreg[it] = *reinterpret_cast<const uint4*>(krow(x) + HD + (lane & 15) * 8);
        }
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            int x = x0 + 16 * blk + a;
            x = x < lo ? lo : (x > hi ? hi : x);
            const bf16_t* kr = krow(x) + lg * 8;
            int dr = p.mlen - (x + joff);
            dr = dr < 0 ? 0 : (dr > p.nd - 1 ? p.nd - 1 : dr);
            const bf16_t* rr = Rg + (int64_t)dr * HD + lg * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                kreg[blk][ks] = *reinterpret_cast<const bf16x8_t*>(kr + ks * 32);
                rreg[blk][ks] = *reinterpret_cast<const bf16x8_t*>(rr + ks * 32);
            }
        }
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int vrow = it * 4 + (lane >> 4), ch = lane & 15;
            *reinterpret_cast<uint4*>(Vs + vrow * 256 + ch * 16) = vreg[it];
        }
        // ---- S^T[key][row] = K . (q + u)^T + R[dist(key)] . (q + v)^T for the two 16-key blocks, one fp32 accumulator
        f32x4 acc_s[2];
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            acc_s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) acc_s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kreg[blk][ks], fqu[ks], acc_s[blk], 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 4; ks++) acc_s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rreg[blk][ks], fqv[ks], acc_s[blk], 0, 0, 0);
        }
        float s[8];
#pragma unroll
        for (int blk = 0; blk < 2; blk++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int x = x0 + 16 * blk + 4 * lg + r;
                const bool vis = x >= lo && x <= hi && x + joff > -p.shift;
                s[blk * 4 + r] = vis ? acc_s[blk][r] * p.scale : -1.0e30f;
            }
        m_i = dec_tile_max(s);         // (one step per wave: no running maximum, nothing accumulated to rescale)
        l_i = dec_tile_exp(s, m_i);
        dec_pv(acc_o, Vs, dec_pack_p(s), 1.f, a, lg);
    }
    // ---- the four waves' partial results (one 32-position step each) merged through LDS into ONE unit, waves in order
    float o8[8], mx, lsum;
    dec_merge_waves<DEC_WAVE_LDS>(smem, acc_o, m_i, l_i, o8, mx, lsum);
    const int qi = threadIdx.x & 15, dg = (threadIdx.x >> 4) * 8;
    const int wrow = PRIV ? sub : 16 * sub + qi;          // the row inside the group this thread's column stands for
    if (PRIV ? qi == 0 : wrow < p.W) dec_store_unit(p.part + dec_part_off(grp, p.H, h, p.nunit, PRIV ? p.nb + chunk : chunk, wrow), dg, o8, mx, lsum, false);
}
// grid = (nb ntile shared units + nt W private units, heads, groups)
__global__ __launch_bounds__(256) void relattn_decode_group_kernel(DecodeGroupArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // guard: a count or an origin out of range is clamped (every access stays in bounds) and reported by one thread
    int ntl = p.n_tail[0], sb = p.state_b[0], st_ = p.state_t[0];
    const int lim = p.Lt < p.mlen ? p.Lt : p.mlen;
    const bool bad = ntl < 0 || ntl > lim || sb < 0 || sb >= p.cap_b || st_ < 0 || st_ >= p.cap_t;
    ntl = ntl < 0 ? 0 : (ntl > lim ? lim : ntl);
    sb = sb < 0 ? 0 : (sb >= p.cap_b ? p.cap_b - 1 : sb);
    st_ = st_ < 0 ? 0 : (st_ >= p.cap_t ? p.cap_t - 1 : st_);
    if (bad && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) atomicOr(p.status, 1);
    const int nshared = p.nb * p.ntile, x = blockIdx.x;
    if (x < nshared) decode_group_unit<false>(p, smem, x / p.ntile, x % p.ntile, sb, st_, ntl);
    else decode_group_unit<true>(p, smem, (x - nshared) / p.W, (x - nshared) % p.W, sb, st_, ntl);
}
__global__ void group_ring_advance_kernel(int* state_t, int* n_tail, int cap_t, int lim) {
    const int s = state_t[0] + 1, n = n_tail[0] + 1;
    state_t[0] = s >= cap_t ? s - cap_t : s;
    n_tail[0] = n > lim ? lim : n;
}

extern "C" int db1_relattn_decode_group_supported(int G, int W, int mlen, int Lt, int cap_b, int cap_t, int H, int D, int dt) {
    return (dt == DB1_BF16 && D == DEC_D && G > 0 && G <= 65535 && H > 0 && H <= 65535 && W >= 1 && W <= 64 && mlen >= 1 && mlen + 1 <= 2048 && Lt >= 1 &&
            Lt <= 4096 && cap_b >= mlen && cap_t >= Lt + 1) ? 1 : 0;
}
static inline int dec_group_units(int mlen, int Lt) { return (mlen + DECR_KC - 1) / DECR_KC + (Lt + 1 + DECR_KC - 1) / DECR_KC; }
extern "C" int64_t db1_relattn_decode_group_workspace_bytes(int G, int W, int mlen, int Lt, int H) {
    (void)W;
    if (G <= 0 || H <= 0 || mlen < 1 || Lt < 1) return 0;
    return (int64_t)G * H * dec_group_units(mlen, Lt) * DEC_PART_UNIT * (int64_t)sizeof(float);
}
extern "C" int db1_relattn_decode_group_fwd(const void* qkv_new, const void* u, const void* vb, const void* base, const int32_t* state_b, int cap_b, void* tail,
                                            const int32_t* state_t, int cap_t, const int32_t* n_tail, int Lt, const void* R, int nd, void* out, int G, int W,
                                            int mlen, int H, int D, int shift, float scale, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
    if (!db1_relattn_decode_group_supported(G, W, mlen, Lt, cap_b, cap_t, H, D, DB1_BF16))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "relattn_decode_group: needs bf16, d_head = 128, 1 <= W <= 64, 1 <= mlen <= 2047, 1 <= Lt <= 4096, cap_b >= mlen, cap_t > Lt "
                 "(got W=%d mlen=%d Lt=%d cap_b=%d cap_t=%d D=%d)", W, mlen, Lt, cap_b, cap_t, D);
    if (nd < 1 || shift < 0 || !qkv_new || !u || !vb || !base || !state_b || !tail || !state_t || !n_tail || !R || !out || !status)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_decode_group: null buffer, nd %d < 1 or shift %d < 0", nd, shift);
    if (!db1_aligned16(qkv_new) || !db1_aligned16(u) || !db1_aligned16(vb) || !db1_aligned16(base) || !db1_aligned16(tail) || !db1_aligned16(R) || !db1_aligned16(out))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "relattn_decode_group: operands must be 16-byte aligned");
    DecodeGroupArgs a;
    a.qkv = (const bf16_t*)qkv_new; a.u = (const bf16_t*)u; a.vb = (const bf16_t*)vb; a.base = (const bf16_t*)base; a.state_b = state_b; a.tail = (bf16_t*)tail;
    a.state_t = state_t; a.n_tail = n_tail; a.R = (const bf16_t*)R; a.status = status;
    a.G = G; a.W = W; a.mlen = mlen; a.Lt = Lt; a.H = H; a.shift = shift; a.nd = nd; a.cap_b = cap_b; a.cap_t = cap_t; a.scale = scale;
    a.nb = (mlen + DECR_KC - 1) / DECR_KC; a.ntile = (W + 15) / 16; a.nunit = dec_group_units(mlen, Lt);
    DB1_NEED_WS(ws, ws_bytes, db1_relattn_decode_group_workspace_bytes(G, W, mlen, Lt, H), "relattn_decode_group");
    a.part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nx = (unsigned)(a.nb * a.ntile + (a.nunit - a.nb) * W);
    relattn_decode_group_kernel<<<dim3(nx, (unsigned)H, (unsigned)G), 256, 4 * DEC_WAVE_LDS, st>>>(a);
    DB1_CHECK_LAUNCH("relattn_decode_group");
    return dec_launch_merge2(a.part, (bf16_t*)out, G, W, H, a.nunit, st);
}
extern "C" int db1_group_ring_advance(int32_t* state_t, int32_t* n_tail, int cap_t, int Lt, int mlen, void* stream) {
    if (!state_t || !n_tail || cap_t <= 0 || Lt < 1 || mlen < 1 || cap_t < Lt + 1) DB1_FAIL(DB1_ERR_BAD_SHAPE, "group_ring_advance: cap_t=%d Lt=%d mlen=%d", cap_t, Lt, mlen);
    group_ring_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state_t, n_tail, cap_t, Lt < mlen ? Lt : mlen);
    DB1_CHECK_LAUNCH("group_ring_advance");
    return DB1_OK;
}
