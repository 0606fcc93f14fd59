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

// db1_ring_fork_rows: db1_ring_prefill_rows with a RING as the memory (a prefix cache's row continued by a call; include/db1_hip.h states the
// rule, tests/ring_fork_rule.py restates it).  Destination i, from call row s = src[i] over base ring row r = base_rows[s]: position j is row
// c = j + q of cat(memory of r, new rows of s).  c < mlen: the SLOT BYTES of base slot (base origin + c) % cap_base, copied as they are -- an
// fp8 slot keeps its payload and scales, nothing is requantised; otherwise new row c - mlen, copied (bf16) or quantised (fp8) as above.
// Same grid and in-flight scheme: (ceil(mlen / 8), n_dst), four 16-byte words in flight per thread; a chunk's copied positions come first.
struct RingForkArgs {
    unsigned char* ring; const unsigned char* base;
    const bf16_t* k_new; const bf16_t* v_new;
    int64_t n_rs, n_bs;
    const int* state; const int* state_base; const int* rows; const int* src; const int* base_rows; int* status;
    int M, cap, M_base, cap_base, mlen, q, H, n_src;
};

template <bool FP8>
__global__ __launch_bounds__(RPF_THREADS) void ring_fork_rows_kernel(RingForkArgs a) {
    const int i = blockIdx.y;
    const int row = a.rows[i], s = a.src ? a.src[i] : i, s0 = *a.state, sb = *a.state_base;
    const bool bad_row = row < 0 || row >= a.M, bad_origin = s0 < 0 || s0 >= a.cap, bad_src = s < 0 || s >= a.n_src;
    const int r = bad_src ? -1 : (a.base_rows ? a.base_rows[s] : s);
    const bool bad_base = (!bad_src && (r < 0 || r >= a.M_base)) || sb < 0 || sb >= a.cap_base;
    if (bad_row || bad_origin || bad_src || bad_base) {     // (block-uniform) never written through: reported once per destination
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, (bad_row ? 1 : 0) | (bad_origin ? 2 : 0) | (bad_src ? 4 : 0) | (bad_base ? 8 : 0));
        return;
    }
    const int HD = a.H * RPF_D;
    const int64_t slot = FP8 ? (int64_t)264 * a.H : (int64_t)4 * HD;                 // bytes
    const int j0 = blockIdx.x * RPF_POS, npos = min(RPF_POS, a.mlen - j0);
    unsigned char* ringb = a.ring + (int64_t)row * a.cap * slot;
    const unsigned char* baseb = a.base + (int64_t)r * a.cap_base * slot;
    const bf16_t* kn = a.k_new + (int64_t)s * a.n_bs;
    const bf16_t* vn = a.v_new + (int64_t)s * a.n_bs;
    const int q = a.q, mlen = a.mlen, cap = a.cap, cap_base = a.cap_base;
    const int64_t n_rs = a.n_rs;
    // position j_: its destination slot, the base slot it is copied from (j_ + q < mlen) or the K (kv_ = 0) / V row of the call it comes from
#define RFK_DST_SLOT(j_) (ringb + (int64_t)(s0 + (j_) >= cap ? s0 + (j_) - cap : s0 + (j_)) * slot)
#define RFK_BASE_SLOT(j_) (baseb + (int64_t)(sb + (j_) + q >= cap_base ? sb + (j_) + q - cap_base : sb + (j_) + q) * slot)
#define RFK_NEW_ROW(j_, kv_) (((kv_) ? vn : kn) + (int64_t)((j_) + q - mlen) * n_rs)
    if (FP8) {
        const int ncopy = max(0, min(npos, mlen - q - j0));   // the chunk's first ncopy positions are base slots (block-uniform)
        const int SW = 33 * (a.H >> 1);                       // 16-byte words of a slot
        const int nw = ncopy * SW;
#pragma unroll 1
        for (int w0 = threadIdx.x; w0 < nw; w0 += 4 * RPF_THREADS) {
            uint4 v[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int w = min(w0 + t * RPF_THREADS, nw - 1);                     // (past the end: the last word again, not stored)
                const int pos = w / SW;
                v[t] = reinterpret_cast<const uint4*>(RFK_BASE_SLOT(j0 + pos))[w - pos * SW];
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int w = w0 + t * RPF_THREADS, pos = w / SW;
                if (w < nw) reinterpret_cast<uint4*>(RFK_DST_SLOT(j0 + pos))[w - pos * SW] = v[t];
            }
        }
        const int nblk = (npos - ncopy) * 2 * a.H;             // (position, K | V, head) blocks of the call's rows, 32 per pass
        for (int base = 0; base < nblk; base += 32) {
            const int blk = base + (int)(threadIdx.x >> 3);
            const bool active = blk < nblk;
            const int bk = active ? blk : 0;
            const int pos = ncopy + bk / (2 * a.H), rr = bk - (pos - ncopy) * 2 * a.H;
            const int kv = rr >= a.H ? 1 : 0, h = rr - kv * a.H;
            unsigned char* dst = RFK_DST_SLOT(j0 + pos);
            kv8_quant_block(RFK_NEW_ROW(j0 + pos, kv) + h * RPF_D, dst + (kv * a.H + h) * RPF_D, reinterpret_cast<float*>(dst + 2 * HD) + kv * a.H + h,
                            (int)(threadIdx.x & 7), active);
        }
    } else {
        const int W = a.H * 16;                                // 16-byte words of one K (or V) row; a bf16 slot is the K row, then the V row
        for (int w = threadIdx.x; w < 2 * W; w += RPF_THREADS) {
            const int kv = w >= W ? 1 : 0, wo = w - kv * W;
#pragma unroll 1
            for (int p0 = 0; p0 < npos; p0 += 4) {
                uint4 v[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int j = j0 + (p0 + t < npos ? p0 + t : npos - 1);          // (past the chunk's end: its last position again, not stored)
                    v[t] = j + q < mlen ? reinterpret_cast<const uint4*>(RFK_BASE_SLOT(j))[w] : reinterpret_cast<const uint4*>(RFK_NEW_ROW(j, kv))[wo];
                }
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (p0 + t < npos) reinterpret_cast<uint4*>(RFK_DST_SLOT(j0 + p0 + t))[w] = v[t];
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

extern "C" int db1_ring_fork_rows_supported(int fp8, int q, int mlen, int cap_base, int cap, int H, int D) {
    return (db1_ring_prefill_rows_supported(fp8, q, mlen, cap, H, D) && mlen < cap_base) ? 1 : 0;
}

extern "C" int db1_ring_fork_rows(void* ring, int fp8, int M, int cap, const void* base, int M_base, int cap_base, const int32_t* state_base,
                                  const int32_t* base_rows, const void* k_new, const void* v_new, int64_t new_row_stride, int64_t new_batch_stride,
                                  const int32_t* state, const int32_t* rows, const int32_t* src, int n_dst, int n_src, int q, int mlen, int H, int D,
                                  int32_t* status, void* stream) {
    if (!db1_ring_fork_rows_supported(fp8, q, mlen, cap_base, cap, H, D))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "ring_fork_rows: needs d_head = 128, an even number of heads on fp8 rings, q >= 1, 1 <= mlen < cap and cap_base "
                                      "(got fp8=%d q=%d mlen=%d cap=%d cap_base=%d H=%d D=%d)", fp8, q, mlen, cap, cap_base, H, D);
    if (M <= 0 || M_base <= 0 || n_dst < 0 || n_dst > 65535 || n_dst > M || n_src <= 0 || (!base_rows && n_src > M_base))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_fork_rows: M=%d M_base=%d n_dst=%d n_src=%d (without base_rows n_src <= M_base)", M, M_base, n_dst, n_src);
    if (n_dst == 0) return DB1_OK;
    if (!ring || !base || !k_new || !v_new || !state || !state_base || !rows || !status) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_fork_rows: null buffer");
    const int64_t slot = fp8 ? (int64_t)264 * H : (int64_t)4 * H * RPF_D;
    const uintptr_t d0 = (uintptr_t)ring, d1 = d0 + (uintptr_t)((int64_t)M * cap * slot), b0 = (uintptr_t)base, b1 = b0 + (uintptr_t)((int64_t)M_base * cap_base * slot);
    if (d0 < b1 && b0 < d1) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_fork_rows: the base ring and the destination ring overlap");
    if (new_row_stride < (int64_t)H * RPF_D || new_batch_stride < 0) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_fork_rows: a key / value row stride below H * D");
    if ((new_row_stride % 8) || (new_batch_stride % 8) || !db1_aligned16(ring) || !db1_aligned16(base) || !db1_aligned16(k_new) || !db1_aligned16(v_new) ||
        (((uintptr_t)state | (uintptr_t)state_base | (uintptr_t)rows | (uintptr_t)src | (uintptr_t)base_rows | (uintptr_t)status) & 3))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "ring_fork_rows: operands must be 16-byte aligned, strides multiples of 8 elements");
    RingForkArgs a;
    a.ring = (unsigned char*)ring; a.base = (const unsigned char*)base;
    a.k_new = (const bf16_t*)k_new; a.v_new = (const bf16_t*)v_new; a.n_rs = new_row_stride; a.n_bs = new_batch_stride;
    a.state = state; a.state_base = state_base; a.rows = rows; a.src = src; a.base_rows = base_rows; a.status = status;
    a.M = M; a.cap = cap; a.M_base = M_base; a.cap_base = cap_base; a.mlen = mlen; a.q = q; a.H = H; a.n_src = n_src;
    const dim3 grid((unsigned)((mlen + RPF_POS - 1) / RPF_POS), (unsigned)n_dst);
    if (fp8) ring_fork_rows_kernel<true><<<grid, RPF_THREADS, 0, (hipStream_t)stream>>>(a);
    else ring_fork_rows_kernel<false><<<grid, RPF_THREADS, 0, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH("ring_fork_rows");
    return DB1_OK;
}
