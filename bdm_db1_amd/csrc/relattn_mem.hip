// Relative-position attention over Transformer-XL memory for ANY number of new queries (prompt prefill, long-text scoring): q = 1 .. 8192
// new queries against klen = mlen + q keys / values (bf16, d_head = 128), operands and rule of relattn_decode.hip:
//     s[i,j] = ((q_i+u).k_j + (q_i+v).R[clip(mlen+i-j, 0, nd-1)]) * scale,   visible iff  i - shift < j <= i + mlen,   j in [0, klen)
// One launch, no partials, no merge, no workspace, no atomics: a workgroup of 256 threads owns 64 consecutive queries of one (b, h) and walks
// every 32-key step that any of its rows can see, in key order -- two launches on the same inputs give the same bits.
//   grid = (ceil(q / 64), heads, batch); wave w owns queries 16 w .. 16 w + 15 of the block, as in relattn_decode_kernel.
//   K and V of a step are staged ONCE per workgroup in LDS (the four waves read the same keys), double-buffered: the rows of step s + 1
//   travel in registers while step s is computed and are written to the other buffer before the step's single barrier.  Because of the
//   barrier no wave leaves the loop early: a wave without rows, or outside its own window, walks the block's steps and computes nothing.
//   16-byte slots are XOR-swizzled so that both kinds of read are conflict-free: K (ds_read_b128, row = key) slot ^ (row & 15);
//   V (ds_read_b64_tr_b16, 8 rows x 32 bytes per 32-lane half) slot ^ 2 (row & 7).
//   The R rows live in an LDS ring of 128 rows indexed by the (unclamped) distance mod 128: the 64 x 32 block of a step touches the 96
//   distances mlen + ib0 - j0 - 31 .. + 95, the next step the same window moved down by 32, so a step fetches 32 new rows (holding
//   R[clip(distance)]) into the quarter of the ring the current window does not use -- 24 KB of loads per step and workgroup instead of the
//   64 KB that four waves fetching their own 48 rows need (measured: that form ran at the L2's rate, 0.90 ms at the caption prompt's shape).
//   Per step and wave the arithmetic is the decode kernel's: S^T = K.Qu^T (2 x 4 v_mfma_f32_16x16x32_bf16), the relative term for the 47
//   distances the 16 x 32 block touches (3 x 4 MFMA against R rows) through the wave's LDS scratch [48 dist][16 q]
//   and the skewed read-back, online softmax, P rounded to bf16, O^T += V^T.P^T (8 MFMA).  Then ONE normalisation, one bf16 store, and
//   lse = m + log(l) (the sum over the fp32 probabilities).
//   The step is this kernel's OWN COPY of what relattn_decode_step.h holds for the decode kernels (only the types and constants come from
//   there): through that header's functions -- even the mask predicate alone -- the compiler scheduled this loop differently, and the
//   launch took 693 us instead of 581 us at the caption prompt's shape.  Keep the order of operations equal to the header's.
#include "relattn_decode_step.h"
#include "kv8_format.h"

#define MEM_QB 64                       // queries per workgroup
#define MEM_TILE (32 * 256)             // one 32-key tile of K or V: [32][128] bf16
#define MEM_TW (48 * 16 * 4)            // the wave's distance scratch [48][16] f32
#define MEM_RING (128 * 256)            // R rows of 128 consecutive distances: [128][128] bf16
#define MEM_LDS (4 * MEM_TILE + MEM_RING + 4 * MEM_TW)   // K[2], V[2], R ring, T scratch x 4 waves: 76 KB, two workgroups per CU
#define MEM_MAX_Q 8192
#define MEM_MAX_KLEN 16384

struct MemArgs {
    const bf16_t* qu; const bf16_t* qv; const bf16_t* k; const bf16_t* v; const bf16_t* R;
    bf16_t* out; float* lse;
    int64_t kv_rs, kv_bs;
    int B, q, klen, mlen, H, shift, nd;
    float scale;
    const bf16_t* km; const bf16_t* vm;     // KV mode: the memory's keys / values (rows j < mlen); k, v then hold the call's own q rows
    int64_t m_rs, m_bs;                     // ... their row / batch strides (0: one row / one memory for all)
    const unsigned char* base;              // RING mode: the memory lives in the slots of a K/V ring's layer buffer [M_base, cap_base, slot] ...
    const int* state_base; const int* base_rows; int* status;   // ... its origin, the ring row of every call row (NULL: b), the guard's status word
    int M_base, cap_base;
};

// KV = false: k, v hold all klen rows.  KV = true (db1_relattn_mem_kv_fwd): logical key j < mlen is row j of km / vm, key j >= mlen row
// j - mlen of k / v -- only the staged rows' addresses differ, so the result is bit for bit that of KV = false over the concatenation.
// RING (with KV; db1_relattn_mem_ring_fwd): logical key j < mlen is slot (origin + j) % cap_base of ring row base_rows[b] of a K/V ring --
// RING = 1 a bf16 ring, the slot's [2, H, D] pair as it is; RING = 2 an fp8 ring (kv8_format.h), a thread's 16-byte piece widened from 8
// payload bytes and multiplied by its block's scale on the way into LDS (exact: a power of two) -- so the LDS tiles, and with them every
// bit of the result, are those of KV = true over the unpacked, linearised memory.
template <bool KV, int RING = 0>
__global__ __launch_bounds__(256) void relattn_mem_kernel(MemArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // MEM_LDS bytes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ib0 = blockIdx.x * MEM_QB, h = blockIdx.y, b = blockIdx.z;
    const int i0 = ib0 + wave * 16;
    const int a = lane & 15, g = lane >> 4;
    const int HD = p.H * DEC_D;
    char* Rr = smem + 4 * MEM_TILE;
    float* Tw = reinterpret_cast<float*>(smem + 4 * MEM_TILE + MEM_RING + wave * MEM_TW);
    const int i = i0 + a;                                  // this lane's query
    const int qi = i < p.q ? i : p.q - 1;                  // rows beyond q repeat the last query (never stored)
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
    const bf16_t* kmg = KV ? p.km + (int64_t)b * p.m_bs + h * DEC_D : nullptr;
    const bf16_t* vmg = KV ? p.vm + (int64_t)b * p.m_bs + h * DEC_D : nullptr;
    // RING: the call row's ring row and the origin, clamped into range -- every read stays in bounds, one thread per call row reports it
    const unsigned char* ringb = nullptr;
    int rs0 = 0;
    const int64_t rslot = RING == 2 ? (int64_t)264 * p.H : (int64_t)4 * HD;      // bytes
    if (RING) {
        int rrow = p.base_rows ? p.base_rows[b] : b;
        rs0 = p.state_base[0];
        const bool bad_row = rrow < 0 || rrow >= p.M_base, bad_origin = rs0 < 0 || rs0 >= p.cap_base;
        if ((bad_row || bad_origin) && blockIdx.x == 0 && h == 0 && threadIdx.x == 0) atomicOr(p.status, 8);
        rrow = bad_row ? 0 : rrow;
        rs0 = bad_origin ? 0 : rs0;
        ringb = p.base + (int64_t)rrow * p.cap_base * rslot;
    }
    // the block's steps: keys max(0, ib0 - shift + 1) .. ilast + mlen (= the last row's diagonal key < klen), aligned at multiples of 32
    const int ilast = ib0 + MEM_QB - 1 < p.q ? ib0 + MEM_QB - 1 : p.q - 1;
    const int jlo = ib0 - p.shift + 1 > 0 ? ib0 - p.shift + 1 : 0;
    const int st_lo = jlo >> 5, st_hi = (ilast + p.mlen) >> 5;
    // staging: thread t moves the 16-byte pieces (row = idx >> 4, slot = idx & 15), idx = t and t + 256, of K and of V
    const int srow = threadIdx.x >> 4, sch = threadIdx.x & 15;               // piece 0; piece 1 is row srow + 16 (same row & 15, row & 7)
    const int soff_k = srow * 256 + ((sch ^ (srow & 15)) << 4), soff_v = srow * 256 + ((sch ^ ((srow & 7) << 1)) << 4);
    uint4 kst0, kst1, vst0, vst1;
    float ksc0 = 1.f, ksc1 = 1.f, vsc0 = 1.f, vsc1 = 1.f;   // RING = 2: the scales of the staged pieces that hold payload (fpay bit 0: piece 0, bit 1: piece 1)
    unsigned fpay = 0u;
    // the thread's K and V piece of memory key j_ (< mlen) from its ring slot; on an fp8 ring 8 payload bytes (.x, .y) and the block's scale
    auto ring_load = [&](int j_, uint4& kx_, uint4& vx_, float& ks_, float& vs_) {
        const int r_ = rs0 + j_ >= p.cap_base ? rs0 + j_ - p.cap_base : rs0 + j_;
        const unsigned char* sl_ = ringb + (int64_t)r_ * rslot;
        if (RING == 2) {
            const uint2 kp_ = *reinterpret_cast<const uint2*>(sl_ + h * DEC_D + sch * 8), vp_ = *reinterpret_cast<const uint2*>(sl_ + HD + h * DEC_D + sch * 8);
            kx_ = make_uint4(kp_.x, kp_.y, 0u, 0u);
            vx_ = make_uint4(vp_.x, vp_.y, 0u, 0u);
            ks_ = reinterpret_cast<const float*>(sl_ + 2 * HD)[h];
            vs_ = reinterpret_cast<const float*>(sl_ + 2 * HD)[p.H + h];
        } else {
            kx_ = *reinterpret_cast<const uint4*>(sl_ + (h * DEC_D + sch * 8) * 2);
            vx_ = *reinterpret_cast<const uint4*>(sl_ + (HD + h * DEC_D + sch * 8) * 2);
        }
    };
    // rows past klen are clamped: their probabilities are exactly zero
#define MEM_STAGE_LOAD(st_)                                                                                   \
    {                                                                                                         \
        const int ja_ = (st_) * 32 + srow < p.klen ? (st_) * 32 + srow : p.klen - 1;                          \
        const int jb_ = (st_) * 32 + srow + 16 < p.klen ? (st_) * 32 + srow + 16 : p.klen - 1;                \
        if (KV && !((st_) * 32 < p.mlen && (st_) * 32 + 32 > p.mlen)) {   /* a whole step of one source (workgroup-uniform) */ \
            const bool mm_ = (st_) * 32 < p.mlen;                                                             \
            if (RING && mm_) {   /* every staged row is a ring slot; the slot index wraps per row */          \
                ring_load(ja_, kst0, vst0, ksc0, vsc0);                                                       \
                ring_load(jb_, kst1, vst1, ksc1, vsc1);                                                       \
                fpay = 3u;                                                                                    \
            } else {                                                                                          \
                const bf16_t* kb_ = mm_ ? kmg : kg;                                                           \
                const bf16_t* vb_ = mm_ ? vmg : vg;                                                           \
                const int64_t rs_ = mm_ ? p.m_rs : p.kv_rs;                                                   \
                const int sub_ = mm_ ? 0 : p.mlen;                                                            \
                kst0 = *reinterpret_cast<const uint4*>(kb_ + (int64_t)(ja_ - sub_) * rs_ + sch * 8);          \
                vst0 = *reinterpret_cast<const uint4*>(vb_ + (int64_t)(ja_ - sub_) * rs_ + sch * 8);          \
                kst1 = *reinterpret_cast<const uint4*>(kb_ + (int64_t)(jb_ - sub_) * rs_ + sch * 8);          \
                vst1 = *reinterpret_cast<const uint4*>(vb_ + (int64_t)(jb_ - sub_) * rs_ + sch * 8);          \
                fpay = 0u;                                                                                    \
            }                                                                                                 \
        } else if (KV && RING) {   /* the seam step over a ring: the source is picked per staged row */       \
            const bool ma_ = ja_ < p.mlen, mb_ = jb_ < p.mlen;                                                \
            fpay = (ma_ ? 1u : 0u) | (mb_ ? 2u : 0u);                                                         \
            if (ma_) ring_load(ja_, kst0, vst0, ksc0, vsc0);                                                  \
            else {                                                                                            \
                kst0 = *reinterpret_cast<const uint4*>(kg + (int64_t)(ja_ - p.mlen) * p.kv_rs + sch * 8);     \
                vst0 = *reinterpret_cast<const uint4*>(vg + (int64_t)(ja_ - p.mlen) * p.kv_rs + sch * 8);     \
            }                                                                                                 \
            if (mb_) ring_load(jb_, kst1, vst1, ksc1, vsc1);                                                  \
            else {                                                                                            \
                kst1 = *reinterpret_cast<const uint4*>(kg + (int64_t)(jb_ - p.mlen) * p.kv_rs + sch * 8);     \
                vst1 = *reinterpret_cast<const uint4*>(vg + (int64_t)(jb_ - p.mlen) * p.kv_rs + sch * 8);     \
            }                                                                                                 \
        } else if (KV) {   /* the step that straddles the seam: the source is picked per staged row */         \
            const bool ma_ = ja_ < p.mlen, mb_ = jb_ < p.mlen;                                                \
            const int64_t oa_ = ma_ ? (int64_t)ja_ * p.m_rs : (int64_t)(ja_ - p.mlen) * p.kv_rs;              \
            const int64_t ob_ = mb_ ? (int64_t)jb_ * p.m_rs : (int64_t)(jb_ - p.mlen) * p.kv_rs;              \
            kst0 = *reinterpret_cast<const uint4*>((ma_ ? kmg : kg) + oa_ + sch * 8);                         \
            vst0 = *reinterpret_cast<const uint4*>((ma_ ? vmg : vg) + oa_ + sch * 8);                         \
            kst1 = *reinterpret_cast<const uint4*>((mb_ ? kmg : kg) + ob_ + sch * 8);                         \
            vst1 = *reinterpret_cast<const uint4*>((mb_ ? vmg : vg) + ob_ + sch * 8);                         \
        } else {                                                                                              \
            kst0 = *reinterpret_cast<const uint4*>(kg + (int64_t)ja_ * p.kv_rs + sch * 8);                    \
            vst0 = *reinterpret_cast<const uint4*>(vg + (int64_t)ja_ * p.kv_rs + sch * 8);                    \
            kst1 = *reinterpret_cast<const uint4*>(kg + (int64_t)jb_ * p.kv_rs + sch * 8);                    \
            vst1 = *reinterpret_cast<const uint4*>(vg + (int64_t)jb_ * p.kv_rs + sch * 8);                    \
        }                                                                                                     \
    }
#define MEM_STAGE_STORE(buf_)                                                                                 \
    {                                                                                                         \
        if (RING == 2 && (fpay & 1u)) {   /* payload -> bf16 values, only now: the loads travelled during the step's arithmetic */ \
            kst0 = kv8_widen8_scaled(make_uint2(kst0.x, kst0.y), ksc0);                                       \
            vst0 = kv8_widen8_scaled(make_uint2(vst0.x, vst0.y), vsc0);                                       \
        }                                                                                                     \
        if (RING == 2 && (fpay & 2u)) {                                                                       \
            kst1 = kv8_widen8_scaled(make_uint2(kst1.x, kst1.y), ksc1);                                       \
            vst1 = kv8_widen8_scaled(make_uint2(vst1.x, vst1.y), vsc1);                                       \
        }                                                                                                     \
        *reinterpret_cast<uint4*>(smem + (buf_) * MEM_TILE + soff_k) = kst0;                                  \
        *reinterpret_cast<uint4*>(smem + (buf_) * MEM_TILE + soff_k + 16 * 256) = kst1;                       \
        *reinterpret_cast<uint4*>(smem + (2 + (buf_)) * MEM_TILE + soff_v) = vst0;                            \
        *reinterpret_cast<uint4*>(smem + (2 + (buf_)) * MEM_TILE + soff_v + 16 * 256) = vst1;                 \
    }
    // R ring: 32 rows of consecutive distances u0 .. u0 + 31 (row srow and srow + 16 per thread); out-of-range distances hold the clamped
    // row (they belong to masked pairs).  u & 127 and u & 15 are the residues of a negative u too (two's complement).
    uint4 rst0, rst1;
#define MEM_R_STAGE_LOAD(u0_)                                                                                 \
    {                                                                                                         \
        const int ua_ = (u0_) + srow, ub_ = (u0_) + srow + 16;                                                \
        const int da_ = ua_ < 0 ? 0 : (ua_ > p.nd - 1 ? p.nd - 1 : ua_);                                      \
        const int db_ = ub_ < 0 ? 0 : (ub_ > p.nd - 1 ? p.nd - 1 : ub_);                                      \
        rst0 = *reinterpret_cast<const uint4*>(Rg + (int64_t)da_ * HD + sch * 8);                             \
        rst1 = *reinterpret_cast<const uint4*>(Rg + (int64_t)db_ * HD + sch * 8);                             \
    }
#define MEM_R_STAGE_STORE(u0_)                                                                                \
    {                                                                                                         \
        const int ua_ = (u0_) + srow, ub_ = (u0_) + srow + 16;                                                \
        *reinterpret_cast<uint4*>(Rr + (ua_ & 127) * 256 + ((sch ^ (ua_ & 15)) << 4)) = rst0;                 \
        *reinterpret_cast<uint4*>(Rr + (ub_ & 127) * 256 + ((sch ^ (ub_ & 15)) << 4)) = rst1;                 \
    }
    const int DL0 = p.mlen + ib0 - 31;           // the block's lowest distance at step st is DL0 - 32 st
    f32x4 acc_o[8];
#pragma unroll
    for (int db = 0; db < 8; db++) acc_o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_i = -1.0e30f, l_i = 0.f;
    MEM_STAGE_LOAD(st_lo)
#pragma unroll
    for (int t = 0; t < 3; t++) {                // the first step's window: 96 rows
        MEM_R_STAGE_LOAD(DL0 - 32 * st_lo + 32 * t)
        MEM_R_STAGE_STORE(DL0 - 32 * st_lo + 32 * t)
    }
    MEM_STAGE_STORE(0)
    __syncthreads();
    for (int st = st_lo; st <= st_hi; st++) {
        const int cur = (st - st_lo) & 1;
        const int j0 = st * 32;
        // this wave's tile has a row and the step meets the window of one of its rows?  (wave-uniform; the barrier below is reached either way)
        const bool act = i0 < p.q && !(j0 > i0 + 15 + p.mlen || j0 + 31 <= i0 - p.shift);
        if (st < st_hi) {   // the next step's rows are requested before this step's arithmetic
            MEM_STAGE_LOAD(st + 1)
            MEM_R_STAGE_LOAD(DL0 - 32 * (st + 1))
        }
        if (act) {
            // ---- relative term: distances d_lo .. d_lo + 47 with d_lo = mlen + i0 - j0 - 31, rows of the ring  ->  Tw[dist][query]
            const int d_lo = p.mlen + i0 - j0 - 31;
#pragma unroll
            for (int tb = 0; tb < 3; tb++) {
                const int u = d_lo + 16 * tb + a;
                const char* rrow = Rr + (u & 127) * 256;
                f32x4 acc_t = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ks++) {
                    const bf16x8_t rf = *reinterpret_cast<const bf16x8_t*>(rrow + (((ks * 4 + g) ^ (u & 15)) << 4));
                    acc_t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rf, fqv[ks], acc_t, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; r++) Tw[(16 * tb + 4 * g + r) * 16 + a] = acc_t[r];
            }
            const char* Ks = smem + cur * MEM_TILE;
            const char* Vs = smem + (2 + cur) * MEM_TILE;
            // ---- S^T[key][query] for the two 16-key blocks
            f32x4 acc_s[2];
#pragma unroll
            for (int blk = 0; blk < 2; blk++) {
                acc_s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
                const int row = 16 * blk + a;
#pragma unroll
                for (int ks = 0; ks < 4; ks++) {
                    const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(Ks + row * 256 + (((ks * 4 + g) ^ (row & 15)) << 4));
                    acc_s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, fqu[ks], acc_s[blk], 0, 0, 0);
                }
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
            // ---- O^T[d][query] += V^T . P^T over the 32 keys (key permutation of relattn_decode_kernel: slots 0-3 = keys 4g..4g+3 of the
            // first 16-key block, slots 4-7 = the same keys of the second); lane reads 8 bytes of row 4g + (a >> 2) (+ 16), columns db*16 + (a & 3)*4
            const int vrow = 4 * g + (a >> 2);                       // (vrow & 7) == ((vrow + 16) & 7): one swizzle for both reads
            const int vsw = (vrow & 7) << 1;
#pragma unroll
            for (int db = 0; db < 8; db++) {
                const int slot = (db * 2 + ((a & 3) >> 1)) ^ vsw;
                const char* base = Vs + vrow * 256 + (slot << 4) + ((a & 1) << 3);
                const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(bf16x4_t, const_cast<char*>(base)));
                const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(bf16x4_t, const_cast<char*>(base) + 16 * 256));
                const bf16x8_t vt = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int r = 0; r < 4; r++) acc_o[db][r] *= alpha;
                acc_o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt, pb.v, acc_o[db], 0, 0, 0);
            }
        }
        if (st < st_hi) {   // (every wave finished reading that buffer, and that quarter of the ring, before the previous step's barrier)
            MEM_STAGE_STORE(cur ^ 1)
            MEM_R_STAGE_STORE(DL0 - 32 * (st + 1))
        }
        __syncthreads();
    }
    // ---- one normalisation, one store: lane holds query a, d = db*16 + 4g + r.  Every row i < q saw at least one key (shift + mlen >= 1)
    if (i < p.q) {
        const float inv = l_i > 0.f ? 1.0f / l_i : 0.f;
        bf16_t* dst = p.out + ((int64_t)b * p.q + i) * HD + h * DEC_D + 4 * g;
#pragma unroll
        for (int db = 0; db < 8; db++) {
            uint2 w;
            w.x = f2bf_pk(acc_o[db][0] * inv, acc_o[db][1] * inv);
            w.y = f2bf_pk(acc_o[db][2] * inv, acc_o[db][3] * inv);
            *reinterpret_cast<uint2*>(dst + db * 16) = w;
        }
        if (p.lse && g == 0) p.lse[((int64_t)b * p.H + h) * p.q + i] = m_i + __logf(l_i);
    }
}

extern "C" int db1_relattn_mem_supported(int B, int q, int klen, int mlen, int H, int D, int shift, int dt) {
    return (dt == DB1_BF16 && D == DEC_D && B > 0 && H > 0 && B <= 65535 && H <= 65535 && q >= 1 && q <= MEM_MAX_Q && mlen >= 0 &&
            klen == mlen + q && klen <= MEM_MAX_KLEN && shift >= 0 && (int64_t)shift + mlen >= 1) ? 1 : 0;
}

extern "C" int64_t db1_relattn_mem_workspace_bytes(int B, int q, int klen, int H) {
    (void)B; (void)q; (void)klen; (void)H;
    return 0;
}

extern "C" int db1_relattn_mem_fwd(const void* qu, const void* qv, const void* k, const void* v, int64_t kv_row_stride, int64_t kv_batch_stride,
                                   const void* R, int nd, void* out, float* lse, int B, int q, int klen, int mlen, int H, int D, int shift,
                                   float scale, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    if (q >= 1 && mlen >= 0 && klen != mlen + q) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem: klen (%d) must be mlen (%d) + q (%d)", klen, mlen, q);
    if (!db1_relattn_mem_supported(B, q, klen, mlen, H, D, shift, DB1_BF16))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "relattn_mem: needs bf16, d_head = 128, 1 <= q <= 8192, klen = mlen + q <= 16384, shift >= 0, shift + mlen >= 1 "
                                      "(got q=%d klen=%d mlen=%d D=%d shift=%d)", q, klen, mlen, D, shift);
    if (nd < 1 || !R || !qu || !qv || !k || !v || !out) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem: R rows (%d) or a null operand", nd);
    if (kv_row_stride < (int64_t)H * DEC_D || kv_batch_stride < 0) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem: key / value row stride below H * D");
    if ((kv_row_stride % 8) || (kv_batch_stride % 8) || !db1_aligned16(qu) || !db1_aligned16(qv) || !db1_aligned16(k) || !db1_aligned16(v) ||
        !db1_aligned16(R) || !db1_aligned16(out) || (((uintptr_t)lse) & 3))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "relattn_mem: operands must be 16-byte aligned, strides multiples of 8 elements");
    MemArgs a;
    a.qu = (const bf16_t*)qu; a.qv = (const bf16_t*)qv; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.R = (const bf16_t*)R;
    a.out = (bf16_t*)out; a.lse = lse; a.kv_rs = kv_row_stride; a.kv_bs = kv_batch_stride;
    a.B = B; a.q = q; a.klen = klen; a.mlen = mlen; a.H = H; a.shift = shift; a.nd = nd; a.scale = scale;
    a.km = a.vm = nullptr; a.m_rs = a.m_bs = 0;
    static Db1PerDeviceOnce attr_once;
    attr_once.run([] { hipFuncSetAttribute((const void*)relattn_mem_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, MEM_LDS); });
    relattn_mem_kernel<false><<<dim3((unsigned)((q + MEM_QB - 1) / MEM_QB), (unsigned)H, (unsigned)B), 256, MEM_LDS, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH("relattn_mem");
    return DB1_OK;
}

// ---- the same attention with the keys / values in two places (include/db1_hip.h): a memory of mlen rows and the call's own q rows
extern "C" int db1_relattn_mem_kv_supported(int B, int q, int mlen, int H, int D, int shift, int dt) {
    return (mlen >= 1 && mlen <= MEM_MAX_KLEN && q <= MEM_MAX_KLEN && db1_relattn_mem_supported(B, q, mlen + q, mlen, H, D, shift, dt)) ? 1 : 0;
}

extern "C" int64_t db1_relattn_mem_kv_workspace_bytes(int B, int q, int mlen, int H) {
    (void)B; (void)q; (void)mlen; (void)H;
    return 0;
}

extern "C" int db1_relattn_mem_kv_fwd(const void* qu, const void* qv, const void* k_new, const void* v_new, int64_t new_row_stride,
                                      int64_t new_batch_stride, const void* k_mem, const void* v_mem, int64_t mem_row_stride,
                                      int64_t mem_batch_stride, const void* R, int nd, void* out, float* lse, int B, int q, int mlen, int H, int D,
                                      int shift, float scale, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    if (!db1_relattn_mem_kv_supported(B, q, mlen, H, D, shift, DB1_BF16))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "relattn_mem_kv: needs bf16, d_head = 128, 1 <= q <= 8192, mlen >= 1, mlen + q <= 16384, shift >= 0 "
                                      "(got q=%d mlen=%d D=%d shift=%d)", q, mlen, D, shift);
    if (nd < 1 || !R || !qu || !qv || !k_new || !v_new || !k_mem || !v_mem || !out) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem_kv: R rows (%d) or a null operand", nd);
    if (new_row_stride < (int64_t)H * DEC_D || new_batch_stride < 0 || mem_batch_stride < 0 || (mem_row_stride != 0 && mem_row_stride < (int64_t)H * DEC_D))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem_kv: a key / value row stride below H * D (the memory's may be 0)");
    if ((new_row_stride % 8) || (new_batch_stride % 8) || (mem_row_stride % 8) || (mem_batch_stride % 8) || !db1_aligned16(qu) || !db1_aligned16(qv) ||
        !db1_aligned16(k_new) || !db1_aligned16(v_new) || !db1_aligned16(k_mem) || !db1_aligned16(v_mem) || !db1_aligned16(R) || !db1_aligned16(out) ||
        (((uintptr_t)lse) & 3))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "relattn_mem_kv: operands must be 16-byte aligned, strides multiples of 8 elements");
    MemArgs a;
    a.qu = (const bf16_t*)qu; a.qv = (const bf16_t*)qv; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.R = (const bf16_t*)R;
    a.out = (bf16_t*)out; a.lse = lse; a.kv_rs = new_row_stride; a.kv_bs = new_batch_stride;
    a.km = (const bf16_t*)k_mem; a.vm = (const bf16_t*)v_mem; a.m_rs = mem_row_stride; a.m_bs = mem_batch_stride;
    a.B = B; a.q = q; a.klen = mlen + q; a.mlen = mlen; a.H = H; a.shift = shift; a.nd = nd; a.scale = scale;
    static Db1PerDeviceOnce attr_once;
    attr_once.run([] { hipFuncSetAttribute((const void*)relattn_mem_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, MEM_LDS); });
    relattn_mem_kernel<true><<<dim3((unsigned)((q + MEM_QB - 1) / MEM_QB), (unsigned)H, (unsigned)B), 256, MEM_LDS, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH("relattn_mem_kv");
    return DB1_OK;
}

// ---- the same attention with the memory in the slots of a K/V ring, bf16 or fp8 (include/db1_hip.h): a prefix cache's row continued by a call
extern "C" int db1_relattn_mem_ring_supported(int B, int q, int mlen, int cap_base, int fp8, int H, int D, int shift, int dt) {
    return (mlen >= 1 && mlen < cap_base && (!fp8 || H % 2 == 0) && db1_relattn_mem_kv_supported(B, q, mlen, H, D, shift, dt)) ? 1 : 0;
}

extern "C" int64_t db1_relattn_mem_ring_workspace_bytes(int B, int q, int mlen, int H) {
    (void)B; (void)q; (void)mlen; (void)H;
    return 0;
}

extern "C" int db1_relattn_mem_ring_fwd(const void* qu, const void* qv, const void* k_new, const void* v_new, int64_t new_row_stride,
                                        int64_t new_batch_stride, const void* base, int fp8, int M_base, int cap_base, const int32_t* state_base,
                                        const int32_t* base_rows, int32_t* status, const void* R, int nd, void* out, float* lse, int B, int q, int mlen,
                                        int H, int D, int shift, float scale, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    if (!db1_relattn_mem_ring_supported(B, q, mlen, cap_base, fp8, H, D, shift, DB1_BF16))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "relattn_mem_ring: needs bf16, d_head = 128, 1 <= q <= 8192, 1 <= mlen < cap_base, mlen + q <= 16384, shift >= 0, an even "
                                      "number of heads on an fp8 ring (got q=%d mlen=%d cap_base=%d fp8=%d H=%d D=%d shift=%d)", q, mlen, cap_base, fp8, H, D, shift);
    if (nd < 1 || !R || !qu || !qv || !k_new || !v_new || !base || !state_base || !status || !out)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem_ring: R rows (%d) or a null operand", nd);
    if (M_base < 1 || (!base_rows && B > M_base)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem_ring: %d call rows over a base ring of %d rows need base_rows", B, M_base);
    if (new_row_stride < (int64_t)H * DEC_D || new_batch_stride < 0) DB1_FAIL(DB1_ERR_BAD_SHAPE, "relattn_mem_ring: key / value row stride below H * D");
    if ((new_row_stride % 8) || (new_batch_stride % 8) || !db1_aligned16(qu) || !db1_aligned16(qv) || !db1_aligned16(k_new) || !db1_aligned16(v_new) ||
        !db1_aligned16(base) || !db1_aligned16(R) || !db1_aligned16(out) || (((uintptr_t)lse | (uintptr_t)state_base | (uintptr_t)base_rows | (uintptr_t)status) & 3))
        DB1_FAIL(DB1_ERR_BAD_ALIGN, "relattn_mem_ring: operands must be 16-byte aligned, strides multiples of 8 elements");
    MemArgs a;
    a.qu = (const bf16_t*)qu; a.qv = (const bf16_t*)qv; a.k = (const bf16_t*)k_new; a.v = (const bf16_t*)v_new; a.R = (const bf16_t*)R;
    a.out = (bf16_t*)out; a.lse = lse; a.kv_rs = new_row_stride; a.kv_bs = new_batch_stride;
    a.km = a.vm = nullptr; a.m_rs = a.m_bs = 0;
    a.base = (const unsigned char*)base; a.state_base = state_base; a.base_rows = base_rows; a.status = status; a.M_base = M_base; a.cap_base = cap_base;
    a.B = B; a.q = q; a.klen = mlen + q; a.mlen = mlen; a.H = H; a.shift = shift; a.nd = nd; a.scale = scale;
    const dim3 grid((unsigned)((q + MEM_QB - 1) / MEM_QB), (unsigned)H, (unsigned)B);
    if (fp8) {
        static Db1PerDeviceOnce attr_once;
        attr_once.run([] { hipFuncSetAttribute((const void*)relattn_mem_kernel<true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, MEM_LDS); });
        relattn_mem_kernel<true, 2><<<grid, 256, MEM_LDS, (hipStream_t)stream>>>(a);
    } else {
        static Db1PerDeviceOnce attr_once;
        attr_once.run([] { hipFuncSetAttribute((const void*)relattn_mem_kernel<true, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, MEM_LDS); });
        relattn_mem_kernel<true, 1><<<grid, 256, MEM_LDS, (hipStream_t)stream>>>(a);
    }
    DB1_CHECK_LAUNCH("relattn_mem_ring");
    return DB1_OK;
}
