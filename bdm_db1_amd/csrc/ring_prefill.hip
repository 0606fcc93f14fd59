// db1_ring_prefill_rows: the ring slots of new tenants written straight from (a K/V memory, a call's own K/V) -- the prefill's counterpart of
// db1_ring_load_rows, without the projected [n, mlen, slot] source in between (include/db1_hip.h states the rule, tests/ring_prefill_rule.py
// restates it in NumPy).  One launch per layer, while the call's qkv buffer is alive.
//   grid = (ceil(mlen / 8), n_dst): workgroup (chunk, i) writes logical positions 8 chunk .. 8 chunk + 7 of destination i, ring row rows[i],
//   from source s = src[i]: position j is row c = j + q of cat(memory (mlen rows), new (q rows)) -- memory row c for c < mlen, new row
//   c - mlen otherwise (q >= mlen: everything comes from the call) -- and goes to slot (state[0] + j) % cap.
//   bf16 ring: a pure copy of the K row and the V row (H * 256 bytes each) in 16-byte words, four positions in flight per thread.
//   fp8 ring: kv8_quant_block per (position, K | V, head), eight lanes each, 32 blocks per pass -- the code db1_kv8_quantize runs, so the
//   slots are bit for bit what it produces.
// Nothing but the target slots is written; the only atomic is the atomicOr on the status word (one thread per skipped destination).
#include "db1_common.h"
#include "kv8_format.h"

#define RPF_THREADS 256
#define RPF_POS 8                       // logical positions per workgroup
#define RPF_D 128

struct RingPrefillArgs {
    unsigned char* ring;
    const bf16_t* k_new; const bf16_t* v_new; const bf16_t* k_mem; const bf16_t* v_mem;
    int64_t n_rs, n_bs, m_rs, m_bs;
    const int* state; const int* rows; const int* src; int* status;
    int M, cap, mlen, q, H, n_src;
};

template <bool FP8>
__global__ __launch_bounds__(RPF_THREADS) void ring_prefill_rows_kernel(RingPrefillArgs a) {
    const int i = blockIdx.y;
    const int row = a.rows[i], s = a.src ? a.src[i] : i, s0 = *a.state;
    const bool bad_row = row < 0 || row >= a.M, bad_origin = s0 < 0 || s0 >= a.cap, bad_src = s < 0 || s >= a.n_src;
    if (bad_row || bad_origin || bad_src) {     // (block-uniform) never written through: reported once per destination
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, (bad_row ? 1 : 0) | (bad_origin ? 2 : 0) | (bad_src ? 4 : 0));
        return;
    }
    const int HD = a.H * RPF_D;
    const int64_t slot = FP8 ? (int64_t)264 * a.H : (int64_t)4 * HD;                 // bytes
    const int j0 = blockIdx.x * RPF_POS, npos = min(RPF_POS, a.mlen - j0);
    unsigned char* ringb = a.ring + (int64_t)row * a.cap * slot;
    const bf16_t* kn = a.k_new + (int64_t)s * a.n_bs;
    const bf16_t* vn = a.v_new + (int64_t)s * a.n_bs;
    const bf16_t* km = a.k_mem + (int64_t)s * a.m_bs;
    const bf16_t* vm = a.v_mem + (int64_t)s * a.m_bs;
    const int q = a.q, mlen = a.mlen, cap = a.cap;
    const int64_t m_rs = a.m_rs, n_rs = a.n_rs;
    // the K (kv_ = 0) or V row of logical position j_: row c = j_ + q of cat(memory, new); its slot: (origin + j_) % cap
#define RPF_SRC_ROW(j_, kv_) \
    ((j_) + q < mlen ? ((kv_) ? vm : km) + (int64_t)((j_) + q) * m_rs : ((kv_) ? vn : kn) + (int64_t)((j_) + q - mlen) * n_rs)
#define RPF_DST_SLOT(j_) (ringb + (int64_t)(s0 + (j_) >= cap ? s0 + (j_) - cap : s0 + (j_)) * slot)
    if (FP8) {
        const int nblk = npos * 2 * a.H;                       // (position, K | V, head) blocks, 32 per pass; the bound is block-uniform
        for (int base = 0; base < nblk; base += 32) {
            const int blk = base + (int)(threadIdx.x >> 3);
            const bool active = blk < nblk;
            const int bk = active ? blk : 0;
            const int pos = bk / (2 * a.H), r = bk - pos * 2 * a.H;
            const int kv = r >= a.H ? 1 : 0, h = r - kv * a.H;
            unsigned char* dst = RPF_DST_SLOT(j0 + pos);
            kv8_quant_block(RPF_SRC_ROW(j0 + pos, kv) + h * RPF_D, dst + (kv * a.H + h) * RPF_D, reinterpret_cast<float*>(dst + 2 * HD) + kv * a.H + h,
                            (int)(threadIdx.x & 7), active);
        }
    } else {
        const int W = a.H * 16;                                // 16-byte words of one K (or V) row
        for (int w = threadIdx.x; w < 2 * W; w += RPF_THREADS) {
            const int kv = w >= W ? 1 : 0, wo = w - kv * W;
#pragma unroll 1
            for (int p0 = 0; p0 < npos; p0 += 4) {
                uint4 v[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int j = j0 + (p0 + t < npos ? p0 + t : npos - 1);          // (past the chunk's end: its last position again, not stored)
                    v[t] = reinterpret_cast<const uint4*>(RPF_SRC_ROW(j, kv))[wo];
                }
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (p0 + t < npos) reinterpret_cast<uint4*>(RPF_DST_SLOT(j0 + p0 + t))[w] = v[t];
            }
        }
    }
}

extern "C" int db1_ring_prefill_rows_supported(int fp8, int q, int mlen, int cap, int H, int D) {
    return (D == RPF_D && H > 0 && H <= 65535 && (!fp8 || H % 2 == 0) && q >= 1 && mlen >= 1 && mlen < cap) ? 1 : 0;
}

extern "C" int db1_ring_prefill_rows(void* ring, int fp8, int M, int cap, const void* k_new, const void* v_new, int64_t new_row_stride,
                                     int64_t new_batch_stride, const void* k_mem, const void* v_mem, int64_t mem_row_stride, int64_t mem_batch_stride,
                                     const int32_t* state, const int32_t* rows, const int32_t* src, int n_dst, int n_src, int q, int mlen, int H, int D,
                                     int32_t* status, void* stream) {
    if (!db1_ring_prefill_rows_supported(fp8, q, mlen, cap, H, D))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "ring_prefill_rows: needs d_head = 128, an even number of heads on an fp8 ring, q >= 1, 1 <= mlen < cap "
                                      "(got fp8=%d q=%d mlen=%d cap=%d H=%d D=%d)", fp8, q, mlen, cap, H, D);
    if (M <= 0 || n_dst < 0 || n_dst > 65535 || n_dst > M || n_src <= 0) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_prefill_rows: M=%d n_dst=%d n_src=%d", M, n_dst, n_src);
    if (n_dst == 0) return DB1_OK;
    if (!ring || !k_new || !v_new || !k_mem || !v_mem || !state || !rows || !status) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_prefill_rows: null buffer");
    if (new_row_stride < (int64_t)H * RPF_D || new_batch_stride < 0 || mem_batch_stride < 0 || (mem_row_stride != 0 && mem_row_stride < (int64_t)H * RPF_D))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_prefill_rows: a key / value row stride below H * D (the memory's may be 0)");
    if ((new_row_stride % 8) || (new_batch_stride % 8) || (mem_row_stride % 8) || (mem_batch_stride % 8) || !db1_aligned16(ring) || !db1_aligned16(k_new) ||
        !db1_aligned16(v_new) || !db1_aligned16(k_mem) || !db1_aligned16(v_mem) || (((uintptr_t)state | (uintptr_t)rows | (uintptr_t)src | (uintptr_t)status) & 3))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "ring_prefill_rows: operands must be 16-byte aligned, strides multiples of 8 elements");
    RingPrefillArgs a;
    a.ring = (unsigned char*)ring;
    a.k_new = (const bf16_t*)k_new; a.v_new = (const bf16_t*)v_new; a.k_mem = (const bf16_t*)k_mem; a.v_mem = (const bf16_t*)v_mem;
    a.n_rs = new_row_stride; a.n_bs = new_batch_stride; a.m_rs = mem_row_stride; a.m_bs = mem_batch_stride;
    a.state = state; a.rows = rows; a.src = src; a.status = status;
    a.M = M; a.cap = cap; a.mlen = mlen; a.q = q; a.H = H; a.n_src = n_src;
    const dim3 grid((unsigned)((mlen + RPF_POS - 1) / RPF_POS), (unsigned)n_dst);
    if (fp8) ring_prefill_rows_kernel<true><<<grid, RPF_THREADS, 0, (hipStream_t)stream>>>(a);
    else ring_prefill_rows_kernel<false><<<grid, RPF_THREADS, 0, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH("ring_prefill_rows");
    return DB1_OK;
}
