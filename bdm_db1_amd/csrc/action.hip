// Action decoding on the device (db1_select_actions, db1_obs_tokens; include/db1_hip.h): the per-token work of the reference's RL evaluation
// (evaluate_rl.py:96-138,157-266: restrict the logits to the action vocabulary, subtract the environment's action mask, argmax, map the id back
// to a tokenizer bin, decode the bin, feed the id back) as ONE launch that can be captured behind the model call, and the tokenizer's
// observation ids written straight into the observation call's input.
//
// db1_select_actions: one workgroup of 256 threads per row; the window [act_lo, act_hi) is at most 4096 columns, i.e. at most 5 of the
// 1024-column blocks the row is cut into.  Thread `tid` owns the four consecutive columns 4 ((jb + j) * 256 + tid) + 0..3 of block jb + j,
// jb = act_lo / 1024, j < NG.  The choice is db1_select_tokens' (select.hip) over the same window, bit for bit:
//   - keys, arg-max, the top-k count and the thresholds are integer work: any order of reduction gives the same bits;
//   - a column's Philox counter and word depend on the column alone (column / 4, column % 4): the groups of four are aligned as select.hip's;
//   - the two fp32 sums of top-p (the kept mass and the mass above a threshold) are added in select.hip's order.  There thread T of 1024 adds
//     its groups T, T + 1024, ... in turn, wave T / 64 butterflies, and the 16 wave sums are added in order.  Block b of this kernel is that
//     kernel's threads 256 (b % 4) + tid, so (tid, b % 4) stands for thread T: the groups of blocks b and b + 4 are added in turn into one
//     partial sum (act_mass), each of the four partials goes through the butterfly of its own wave and lands in slot tid / 64 + 4 (b % 4) of 16,
//     and the 16 slots are added in order (act_block_sum_f).  A group outside the window adds +0.0f there and is left out here.
#include "select_common.h"
#include "mulaw.h"

#define ACT_THREADS 256
#define ACT_WAVES (ACT_THREADS / 64)
#define ACT_MAX_NG 5                       // a window of 4096 columns that starts inside a block touches 5 blocks
#define ACT_MAX_WINDOW 4096
#define ACT_MAX_LEN 64
#define ACT_SITE_SAMPLE 0xE0000100u        // db1_select_tokens' site: the same draws

typedef SelSharedT<ACT_WAVES> ActShared;

struct ActArgs {
    const void* logits;
    int64_t ld;
    int lo, hi;
    const uint8_t* mask;
    int n_mask;
    float inv_t;
    int top_k;
    float top_p;
    int greedy;
    unsigned k0, k1;
    int step_base;
    const int* ctr;
    const int* stream_id;
    int act_len, num_bins;
    int* bins;
    float* values;
    long long* next_ids;
    int64_t ids_stride;
    int* status;
};

// the 16 wave sums of select.hip's 1024 threads from the four partials of this block's 256 (part[v]: the groups of blocks jb + v, jb + v + 4)
__device__ __forceinline__ float act_block_sum_f(const float (&part)[4], int jb, float (&f)[2][16], int& ph) {
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const float x = wave_sum(part[v]);
        if ((threadIdx.x & 63) == 0) f[ph][(threadIdx.x >> 6) + 4 * ((jb + v) & 3)] = x;
    }
    __syncthreads();
    float r = f[ph][0];
#pragma unroll
    for (int w = 1; w < 16; w++) r += f[ph][w];
    ph ^= 1;
    return r;
}
template <int NG>
__device__ __forceinline__ int act_count_ge(const unsigned (&key)[NG][4], unsigned thr, ActShared& sh, int& ph) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < NG; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) c += (int)__popcll(__ballot(key[j][q] >= thr));
    return block_sum_i(c, sh, ph);
}
template <int NG>
__device__ __forceinline__ float act_mass_ge(const unsigned (&key)[NG][4], const float (&e)[NG][4], unsigned thr, int jb, float (&f)[2][16], int& ph) {
    float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NG; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) part[j & 3] += key[j][q] >= thr ? e[j][q] : 0.f;
    return act_block_sum_f(part, jb, f, ph);
}

template <typename T, int NG>
__global__ __launch_bounds__(ACT_THREADS) void select_actions_kernel(ActArgs a) {
    __shared__ ActShared sh;
    __shared__ float f16[2][16];
    const int tid = threadIdx.x, row = blockIdx.x;
    const int env_step = a.ctr[0], i = a.ctr[1];
    if (i == a.act_len) return;                       // (block-uniform) the memorising call: nothing is written
    if (i < 0 || i > a.act_len) {                     // (block-uniform)
        if (tid == 0) a.status[row] |= 2;
        return;
    }
    const T* lg = reinterpret_cast<const T*>(a.logits) + (int64_t)row * a.ld;
    const uint8_t* mk = a.mask ? a.mask + (int64_t)row * a.n_mask : nullptr;
    const int lo = a.lo, hi = a.hi, jb = lo >> 10;
    unsigned key[NG][4];
    unsigned long long best = 0;   // (key << 32) | ~column: max = largest key, lowest column on ties
    unsigned kmin = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < NG; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = 4 * ((jb + j) * ACT_THREADS + tid) + q;
            bool in = c >= lo && c < hi;
            if (in && mk && c - lo < a.n_mask) in = mk[c - lo] != 0;
            const unsigned k = in ? sel_key(ldf<T>(lg + c)) : 0u;
            key[j][q] = k;
            const unsigned long long p = ((unsigned long long)k << 32) | (unsigned)~c;
            best = (k && p > best) ? p : best;
            kmin = k ? min(kmin, k) : kmin;
        }
    int ph = 0;
    best = block_max_u64(best, sh, ph);
    int tok, bits = 0;
    const unsigned kmax = (unsigned)(best >> 32);
    if (kmax == 0) {                                  // no candidate: nothing finite and allowed in the window
        tok = lo;
        bits = 1;
    } else if (a.greedy || a.top_k == 1) {
        tok = (int)~(unsigned)best;
    } else {
        // top-k, top-p and the Gumbel-max draw of select.hip (bf16 logits: the bisections run over the high 16 bits of the keys)
        constexpr int S = sizeof(T) == 2 ? 16 : 0;
        unsigned thr = block_min_u32(kmin, sh, ph);
        if (a.top_k > 1)
            thr = sel_bisect_max(thr >> S, kmax >> S, [&](unsigned mid) { return act_count_ge<NG>(key, mid << S, sh, ph) >= a.top_k; }) << S;
        if (a.top_p < 1.f) {
            const float m = sel_unkey(kmax);
            float e[NG][4];
            float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NG; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    e[j][q] = key[j][q] >= thr ? expf((sel_unkey(key[j][q]) - m) * a.inv_t) : 0.f;
                    part[j & 3] += e[j][q];
                }
            const float target = a.top_p * act_block_sum_f(part, jb, f16, ph);
            thr = sel_bisect_max(thr >> S, kmax >> S, [&](unsigned mid) { return act_mass_ge<NG>(key, e, mid << S, jb, f16, ph) >= target; }) << S;
        }
        const unsigned sid = a.stream_id ? (unsigned)a.stream_id[row] : (unsigned)row;
        const unsigned step = (unsigned)a.step_base + (unsigned)env_step * (unsigned)a.act_len + (unsigned)i;
        unsigned long long sb = 0;
#pragma unroll
        for (int j = 0; j < NG; j++) {
            const bool any = key[j][0] >= thr || key[j][1] >= thr || key[j][2] >= thr || key[j][3] >= thr;
            if (any) {
                const int g = (jb + j) * ACT_THREADS + tid;
                unsigned o[4];
                db1_philox4x32_10((unsigned)g, sid, step, ACT_SITE_SAMPLE, a.k0, a.k1, o);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (key[j][q] < thr) continue;
                    const float u = ((float)(o[q] >> 8) + 0.5f) * 5.9604644775390625e-8f;   // ((x >> 8) + 0.5) * 2^-24: exact in fp32
                    const float s = sel_unkey(key[j][q]) * a.inv_t - logf(-logf(u));
                    const unsigned sk = sel_key(s);
                    const unsigned long long p = ((unsigned long long)sk << 32) | (unsigned)~(4 * g + q);
                    sb = p > sb ? p : sb;
                }
            }
        }
        sb = block_max_u64(sb, sh, ph);
        tok = (unsigned)(sb >> 32) ? (int)~(unsigned)sb : (int)~(unsigned)best;   // (a non-finite score cannot win: fall back to the arg-max)
    }
    if (tid == 0) {
        const int64_t at = (int64_t)row * a.act_len + i;
        const int bin = tok - lo;
        a.bins[at] = bin;
        if (a.values) {
            int bad = 0;
            a.values[at] = mulaw_decode_one(bin, 1, a.num_bins, 0.f, 0.f, bad);
        }
        a.next_ids[(int64_t)row * a.ids_stride] = tok;
        if (bits) a.status[row] |= bits;
    }
}

static int act_ng(int lo, int hi) { return ((hi + 1023) >> 10) - (lo >> 10); }

extern "C" int db1_select_actions_supported(int V, int64_t ld, int dt, int act_lo, int act_hi) {
    return db1_dt_ok(dt) && V > 0 && ld >= V && act_lo >= 0 && act_lo < act_hi && act_hi <= V && act_hi - act_lo <= ACT_MAX_WINDOW;
}

extern "C" int64_t db1_select_actions_workspace_bytes(int M, int V, int dt) {
    (void)M; (void)V; (void)dt;
    return 0;
}

extern "C" int db1_select_actions(const void* logits, int M, int V, int64_t ld, int dt, int act_lo, int act_hi, const uint8_t* mask, int n_mask,
                                  float temperature, int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int step_base,
                                  const int32_t* ctr, const int32_t* stream_id, int act_len, int num_bins, int32_t* bins, float* values,
                                  int64_t* next_ids, int64_t ids_stride, int32_t* status, void* stream) {
    const char* who = "select_actions";
    if (!db1_dt_ok(dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dt);
    if (M <= 0 || M > 65535 || V <= 0 || ld < V || ids_stride < 0 || num_bins <= 0)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d V=%d ld=%lld ids_stride=%lld num_bins=%d", who, M, V, (long long)ld, (long long)ids_stride, num_bins);
    if (act_len < 1 || act_len > ACT_MAX_LEN) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: act_len %d (1 .. %d)", who, act_len, ACT_MAX_LEN);
    if (!logits || !ctr || !bins || !next_ids || !status) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (act_lo < 0 || act_hi > V || act_lo >= act_hi)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: window [%d, %d) is empty or outside [0, %d)", who, act_lo, act_hi, V);
    if (act_hi - act_lo > ACT_MAX_WINDOW) DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: window [%d, %d) is wider than %d columns", who, act_lo, act_hi, ACT_MAX_WINDOW);
    if (n_mask < 0 || n_mask > act_hi - act_lo || (mask && n_mask == 0) || (!mask && n_mask != 0))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: n_mask %d for a window of %d columns (mask %s)", who, n_mask, act_hi - act_lo, mask ? "given" : "NULL");
    if (!greedy && !(temperature > 0.f && temperature < INFINITY)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: temperature %g", who, (double)temperature);
    if (!greedy && (top_k < 0 || !(top_p > 0.f && top_p <= 1.f))) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_k %d top_p %g", who, top_k, (double)top_p);
    ActArgs a = {};
    a.logits = logits; a.ld = ld; a.lo = act_lo; a.hi = act_hi; a.mask = mask; a.n_mask = n_mask;
    a.inv_t = greedy ? 1.f : 1.f / temperature; a.top_k = top_k; a.top_p = top_p; a.greedy = greedy;
    a.k0 = seed_lo; a.k1 = seed_hi; a.step_base = step_base; a.ctr = ctr; a.stream_id = stream_id;
    a.act_len = act_len; a.num_bins = num_bins; a.bins = bins; a.values = values;
    a.next_ids = reinterpret_cast<long long*>(next_ids); a.ids_stride = ids_stride; a.status = status;
    const int ng = act_ng(act_lo, act_hi);
    hipStream_t st = (hipStream_t)stream;
    DB1_DISPATCH_DT(dt, T, {
        if (ng == 1) select_actions_kernel<T, 1><<<M, ACT_THREADS, 0, st>>>(a);
        else if (ng == 2) select_actions_kernel<T, 2><<<M, ACT_THREADS, 0, st>>>(a);
        else select_actions_kernel<T, ACT_MAX_NG><<<M, ACT_THREADS, 0, st>>>(a);
    });
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}

// ------------------------------------------------------------------ observation tokens
__global__ __launch_bounds__(256) void obs_tokens_kernel(const float* __restrict__ x, long long* __restrict__ ids, int64_t ids_stride, int64_t n,
                                                         int obs_dim, int bin_base, int sep_id, int nb, float mu, float den) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / (obs_dim + 1);
        const int j = (int)(e - row * (obs_dim + 1));
        ids[row * ids_stride + j] = j < obs_dim ? bin_base + mulaw_discretize_one(x[row * obs_dim + j], 0, nb, mu, den) : sep_id;
    }
}

extern "C" int db1_obs_tokens(const float* x, int M, int obs_dim, int64_t* ids, int64_t ids_stride, int bin_base, int sep_id, int num_bins, float mu,
                              float Mm, void* stream) {
    const char* who = "obs_tokens";
    if (!x || !ids) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (M <= 0 || obs_dim <= 0 || ids_stride < (int64_t)obs_dim + 1 || num_bins <= 0 || bin_base < 0 || sep_id < 0)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d obs_dim=%d ids_stride=%lld num_bins=%d bin_base=%d sep_id=%d", who, M, obs_dim, (long long)ids_stride,
                 num_bins, bin_base, sep_id);
    const int64_t n = (int64_t)M * (obs_dim + 1);
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    obs_tokens_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, reinterpret_cast<long long*>(ids), ids_stride, n, obs_dim, bin_base, sep_id, num_bins,
                                                             mu, mulaw_den(mu, Mm));
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}
