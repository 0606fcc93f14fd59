// Beam search on the device (db1_beam_step, db1_beam_step_diverse, db1_ring_reorder; the rules are stated in include/db1_hip.h and restated
// in NumPy in tests/beam_rule.py).  The reference evaluates captions and answers by generating text (train.py:140-170, evaluate_ic /
// evaluate_vqa, not released); captioning is normally scored with beam search.
//
// Both steps are one launcher (beam_step_launch) and one group step (beam_group_step<DIVERSE>); the plain step is the case of one sub-group
// per prompt and no penalty.  Two launches, both only READ the token counter *t (the step can live in a captured graph):
//   1. rows:  (nb chunks of the vocabulary window) x (M rows), 256 threads.  A chunk computes its max logit m_c, sum exp(l - m_c) and its
//             top-K (K = 2W; diverse: W' + W) candidates by (logit desc, column asc) as packed (order-preserving key << 32 | ~column)
//             words: K rounds of a block arg-max; after each round only the thread that owned the winner rescans its own columns.  Done
//             groups and dead beams exit at once.
//   2. groups: one 256-thread workgroup per group (beam_group_kernel) or per prompt, walking its D sub-groups in turn
//             (beam_group_diverse_kernel).  A wave per beam row merges the nb chunk lists (K rounds of a wave arg-max over the nb list
//             heads) and the fp32 lse (wave max / butterfly sum over the chunks); every candidate gets s = beam_score + (l - lse) and a
//             group key (key(s) << 32 | ~(j << 16 | c); diverse: the key of sel = s - n(c) * lambda, s kept beside it); the group's top-2W
//             come from exact ranks (count of larger keys), so the order is (s desc, j asc, c asc) whatever the rounding did inside a row.
//             One thread walks them (pool offers, new beams), then the workgroup writes the histories (staged through the workspace: the
//             permutation is in place), the pool rows it touched, the beam scores, the parents and the next input ids.
// db1_ring_reorder, two launches (gather into the workspace, write back): the last t keys of every row whose parent is another row.
// Every reduction runs in a fixed order; no atomics, no communication between workgroups inside a launch.
#include <cfloat>

#include "select_common.h"

#define BEAM_THREADS 256
#define BEAM_WAVES (BEAM_THREADS / 64)
#define BEAM_MAX_W 16
#define BEAM_MAX_K (2 * BEAM_MAX_W)
#define BEAM_MAX_NB 16
#define BEAM_MAX_V 65536                   // the column goes into 16 bits of a group key

struct BeamArgs {
    const void* logits;
    int64_t ld;
    int G, W, K, M, V, vlo, vhi, nb, span;
    int eos, pad, max_new;
    float alpha;
    const int* t;
    float* beam_score;
    int* parent;
    int* tokens;
    int* pool_tokens;
    int* pool_len;
    float* pool_score;
    int* pool_slot;
    int* pool_count;
    int* done;
    int* switches;
    long long* next_ids;
    int64_t ids_stride;
    int* status;
    float2* ms;                 // [M, nb] (chunk max, chunk sum of exp(l - max))
    unsigned long long* cand;   // [M, nb, K]
    int* hist;                  // [M, max_new] staged histories
};

template <typename Args>      // (BeamArgs, by value or in the kernarg segment)
__device__ __forceinline__ bool beam_live(const Args& a, int t, int row, int j) {
    return t == 0 ? j == 0 : a.beam_score[row] > -INFINITY;
}

template <typename T>
__global__ __launch_bounds__(BEAM_THREADS) void beam_rows_kernel(BeamArgs a) {
    __shared__ SelSharedT<BEAM_WAVES> sh;
    const int ch = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
    const int g = row / a.W, j = row - g * a.W;
    const int t = *a.t;
    if (t < 0 || t >= a.max_new || a.done[g] || !beam_live(a, t, row, j)) return;   // (block-uniform; launch 2 skips the same rows)
    const T* lg = reinterpret_cast<const T*>(a.logits) + (int64_t)row * a.ld;
    const int c0 = a.vlo + ch * a.span, c1 = min(a.vhi, c0 + a.span);
    unsigned long long best = 0;
    for (int c = c0 + tid; c < c1; c += BEAM_THREADS) {
        const unsigned k = sel_key(ldf<T>(lg + c));
        const unsigned long long p = ((unsigned long long)k << 32) | (unsigned)~c;
        best = (k && p > best) ? p : best;
    }
    int ph = 0;
    unsigned long long win = block_max_u64(best, sh, ph);
    const unsigned kmax = (unsigned)(win >> 32);
    const float m = kmax ? sel_unkey(kmax) : -INFINITY;
    float s = 0.f;
    if (kmax) {
        for (int c = c0 + tid; c < c1; c += BEAM_THREADS) {
            const float l = ldf<T>(lg + c);
            s += sel_key(l) ? expf(l - m) : 0.f;
        }
        s = block_sum_f(s, sh, ph);
    }
    unsigned long long* out = a.cand + ((int64_t)row * a.nb + ch) * a.K;
    if (tid == 0) {
        a.ms[(int64_t)row * a.nb + ch] = make_float2(m, s);
        out[0] = win;
    }
    for (int r = 1; r < a.K; r++) {
        if (win != 0) {      // (block-uniform)
            if (best == win) {   // the one thread that owned the winner: its best column below it
                best = 0;
                for (int c = c0 + tid; c < c1; c += BEAM_THREADS) {
                    const unsigned k = sel_key(ldf<T>(lg + c));
                    const unsigned long long p = ((unsigned long long)k << 32) | (unsigned)~c;
                    best = (k && p < win && p > best) ? p : best;
                }
            }
            win = block_max_u64(best, sh, ph);
        }
        if (tid == 0) out[r] = win;
    }
}

// a hypothesis (score h, tokens: row `src`'s history, then `last` at position t) into the sorted pool (equal scores: the earlier stays ahead)
__device__ void beam_offer(float h, int src, int last, int n, int W, int& count, float* ps, int* pl, int* pslot, int* srow, int* slast) {
    int pos = count;
    while (pos > 0 && ps[pos - 1] < h) pos--;
    if (pos >= W) return;
    int slot;
    if (count < W) slot = count++;
    else slot = pslot[W - 1];
    for (int k = count - 1; k > pos; k--) {
        ps[k] = ps[k - 1];
        pl[k] = pl[k - 1];
        pslot[k] = pslot[k - 1];
    }
    ps[pos] = h;
    pl[pos] = n;
    pslot[pos] = slot;
    srow[slot] = src;
    slast[slot] = last;
}

// The LDS of one group step.  DIVERSE adds the unpenalised s beside every sel key (gs, tops) and the list of the tokens that the earlier
// sub-groups of the prompt chose; the plain step carries one element of each.
template <bool DIVERSE>
struct BeamGroupLds {
    unsigned long long gk[BEAM_MAX_W * BEAM_MAX_K];
    unsigned long long top[BEAM_MAX_K];
    float gs[DIVERSE ? BEAM_MAX_W * BEAM_MAX_K : 1];
    float tops[DIVERSE ? BEAM_MAX_K : 1];
    float ps[BEAM_MAX_W], nb_sc[BEAM_MAX_W];
    int pl[BEAM_MAX_W], pslot[BEAM_MAX_W], srow[BEAM_MAX_W], slast[BEAM_MAX_W], nb_par[BEAM_MAX_W], nb_tok[BEAM_MAX_W], nocand[BEAM_MAX_W];
    int chosen[DIVERSE ? BEAM_MAX_W : 1];
    int filled, done, n_chosen;
};

// One (sub-)group g of W = a.W beams at step t, by the whole workgroup.  The plain step: a.K = 2W candidates per row, ranked by s.  DIVERSE:
// a.K = W' + W per row; every candidate gets s and, ONCE, sel = s - n(c) * lam (n(c): one ballot over the at most 16 tokens in sh.chosen);
// the top-2W' come from exact ranks on the sel keys with s kept beside the key; the walk uses the unpenalised s and appends the new beams'
// tokens to sh.chosen.  Args: BeamArgs, by value or in the kernarg segment.
template <bool DIVERSE, typename Args>
__device__ __forceinline__ void beam_group_step(const Args& a, int g, float lam, BeamGroupLds<DIVERSE>& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = a.W, K = a.K, K2 = DIVERSE ? 2 * a.W : a.K, b0 = g * W, mx = a.max_new;
    const int t = *a.t;
    const int was_done = a.done[g];
    if (was_done || t < 0 || t >= mx) {      // (block-uniform)
        if (tid < W) a.next_ids[(int64_t)(b0 + tid) * a.ids_stride] = a.pad;
        if (tid == 0 && !was_done) a.status[g] |= 2;
        return;
    }
    const int nch = DIVERSE ? sh.n_chosen : 0;
    // 1. per beam row: lse over the chunks, the row's top-K as group keys (DIVERSE: sel keys, with their s)
    for (int j = wv; j < W; j += BEAM_WAVES) {
        const int row = b0 + j;
        if (lane < K) sh.gk[j * BEAM_MAX_K + lane] = 0ull;
        if (lane == 0) sh.nocand[j] = 0;
        if (!beam_live(a, t, row, j)) continue;
        const float base = t == 0 ? 0.f : a.beam_score[row];
        const float2 ms = lane < a.nb ? a.ms[(int64_t)row * a.nb + lane] : make_float2(-INFINITY, 0.f);
        const float m = wave_max(ms.x);
        if (!(m > -INFINITY)) {
            if (lane == 0) sh.nocand[j] = 1;
            continue;
        }
        const float lse = m + logf(wave_sum(ms.x > -INFINITY ? ms.y * expf(ms.x - m) : 0.f));
        const unsigned long long* lst = a.cand + ((int64_t)row * a.nb + lane) * K;
        int idx = 0;
        for (int r = 0; r < K; r++) {
            const unsigned long long h = (lane < a.nb && idx < K) ? lst[idx] : 0ull;
            const unsigned long long w = wave_max_u64(h);
            if (w == 0) break;
            if (h == w) idx++;
            const int c = (int)~(unsigned)w;
            const float s = base + (sel_unkey((unsigned)(w >> 32)) - lse);
            unsigned sk = sel_key(s);
            if constexpr (DIVERSE) {
                const int n = __popcll(__ballot(lane < nch && sh.chosen[lane & (BEAM_MAX_W - 1)] == c));   // (one lane per entry of the list)
                if (lane == 0) {
                    sk = sk ? sel_key(fmaxf(s - (float)n * lam, -FLT_MAX)) : 0u;
                    sh.gs[j * BEAM_MAX_K + r] = s;
                }
            }
            if (lane == 0) sh.gk[j * BEAM_MAX_K + r] = sk ? (((unsigned long long)sk << 32) | (unsigned)~(((unsigned)j << 16) | (unsigned)c)) : 0ull;
        }
    }
    if (tid < K2) sh.top[tid] = 0ull;
    if (tid < W) {
        sh.ps[tid] = a.pool_score[b0 + tid];
        sh.pl[tid] = a.pool_len[b0 + tid];
        sh.pslot[tid] = a.pool_slot[b0 + tid];
        sh.srow[tid] = -1;
    }
    __syncthreads();
    // 2. the group's top-K2 by exact rank (group keys are unique: (j, c) pairs differ)
    for (int e = tid; e < W * K; e += BEAM_THREADS) {
        const int at = (e / K) * BEAM_MAX_K + e % K;
        const unsigned long long x = sh.gk[at];
        if (x == 0) continue;
        int rank = 0;
        for (int f = 0; f < W * K && rank < K2; f++) rank += sh.gk[(f / K) * BEAM_MAX_K + f % K] > x;
        if (rank < K2) {
            sh.top[rank] = x;
            if constexpr (DIVERSE) sh.tops[rank] = sh.gs[at];
        }
    }
    __syncthreads();
    // 3. the walk (one thread, LDS only); DIVERSE: the order is sel's, every score is the unpenalised s
    if (tid == 0) {
        const float den = powf((float)(t + 1), a.alpha);
        int count = a.pool_count[g], filled = 0;
        for (int r = 0; r < K2 && filled < W; r++) {
            const unsigned long long p = sh.top[r];
            if (!p) break;
            const unsigned low = ~(unsigned)p;
            const int j = (int)(low >> 16), c = (int)(low & 0xffffu);
            float s;
            if constexpr (DIVERSE) s = sh.tops[r];
            else s = sel_unkey((unsigned)(p >> 32));
            if (c == a.eos) {
                if (r < W) beam_offer(s / den, b0 + j, c, t, W, count, sh.ps, sh.pl, sh.pslot, sh.srow, sh.slast);
                continue;
            }
            sh.nb_par[filled] = j;
            sh.nb_tok[filled] = c;
            sh.nb_sc[filled] = s;
            filled++;
        }
        if (t == mx - 1)
            for (int k = 0; k < filled; k++)
                beam_offer(sh.nb_sc[k] / den, b0 + sh.nb_par[k], sh.nb_tok[k], t + 1, W, count, sh.ps, sh.pl, sh.pslot, sh.srow, sh.slast);
        float best = -INFINITY;        // the largest new score: the first (the new beams are in s order), DIVERSE (sel order) the maximum
        if constexpr (DIVERSE)
            for (int k = 0; k < filled; k++) best = fmaxf(best, sh.nb_sc[k]);
        else best = sh.nb_sc[0];
        const int done = filled == 0 || (count == W && sh.ps[W - 1] >= best / den);
        int bits = 0, sw = 0;
        for (int j = 0; j < W; j++) bits |= sh.nocand[j];
        for (int k = 0; k < filled && t > 0; k++) sw += sh.nb_par[k] != k;   // (t = 0: every beam descends from beam 0 of one prefill)
        a.pool_count[g] = count;
        a.done[g] = done;
        a.switches[g] += sw;
        if (bits) a.status[g] |= bits;
        sh.filled = filled;
        sh.done = done;
        if constexpr (DIVERSE) {
            if (!done) {       // (nch + filled <= D * W' <= 16)
                for (int k = 0; k < filled && nch + k < BEAM_MAX_W; k++) sh.chosen[nch + k] = sh.nb_tok[k];
                sh.n_chosen = min(nch + filled, BEAM_MAX_W);
            }
        }
    }
    // 4. stage the histories (the new beams and the pool read the OLD rows)
    for (int e = tid; e < W * t; e += BEAM_THREADS) {
        const int64_t o = (int64_t)(b0 + e / t) * mx + e % t;
        a.hist[o] = a.tokens[o];
    }
    __syncthreads();
    const int filled = sh.filled;
    for (int e = tid; e < W * (t + 1); e += BEAM_THREADS) {
        const int j = e / (t + 1), i = e % (t + 1);
        const int64_t o = (int64_t)(b0 + j) * mx + i;
        if (j < filled) a.tokens[o] = i < t ? a.hist[(int64_t)(b0 + sh.nb_par[j]) * mx + i] : sh.nb_tok[j];
        else if (i == t) a.tokens[o] = a.pad;
    }
    for (int e = tid; e < W * mx; e += BEAM_THREADS) {
        const int k = e / mx, i = e % mx, src = sh.srow[k];
        if (src < 0) continue;
        a.pool_tokens[(int64_t)(b0 + k) * mx + i] = i < t ? a.hist[(int64_t)src * mx + i] : (i == t ? sh.slast[k] : a.pad);
    }
    if (tid < W) {
        const int b = b0 + tid;
        const bool alive = tid < filled;
        a.beam_score[b] = alive ? sh.nb_sc[tid] : -INFINITY;
        a.parent[b] = alive ? b0 + sh.nb_par[tid] : b;
        a.next_ids[(int64_t)b * a.ids_stride] = (alive && !sh.done) ? sh.nb_tok[tid] : a.pad;
        a.pool_score[b] = sh.ps[tid];
        a.pool_len[b] = sh.pl[tid];
        a.pool_slot[b] = sh.pslot[tid];
    }
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_group_kernel(BeamArgs a) {
    __shared__ BeamGroupLds<false> sh;
    beam_group_step<false>(a, blockIdx.x, 0.f, sh);
}

// Diverse beam search (db1_beam_step_diverse; the rule is stated in include/db1_hip.h and restated in tests/diverse_beam_rule.py): one
// workgroup per PROMPT walks its D sub-groups of W' = a.W beams in order (a.G = prompts * D sub-groups).  Barriers separate the sub-groups;
// nothing leaves the workgroup.
#define BEAM_KERNARG __attribute__((address_space(4)))      // the constant address space of the kernel's own arguments
struct BeamDivArgs {
    BeamArgs a;
    int D;
    float lam;
};

__global__ __launch_bounds__(BEAM_THREADS) void beam_group_diverse_kernel(BeamDivArgs) {
    __shared__ BeamGroupLds<true> sh;
    // The arguments (the kernel's only parameter: offset 0 of the kernarg segment) are read through a pointer that every trip of the
    // sub-group loop takes as new.  Read as a by-value parameter, all 15 pointers and every loop-invariant condition stay live across the
    // loop, which costs 52 SGPR spills; read again per trip they are scalar loads from the constant segment and nothing spills.
    const BEAM_KERNARG BeamDivArgs* kp = (const BEAM_KERNARG BeamDivArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int nD = kp->D;
    if (threadIdx.x == 0) sh.n_chosen = 0;
    __syncthreads();
#pragma unroll 1
    for (int d = 0; d < nD; d++) {
        asm volatile("" : "+s"(kp));
        beam_group_step<true>(kp->a, blockIdx.x * kp->D + d, kp->lam, sh);
        __syncthreads();     // (the next sub-group rewrites every LDS array)
    }
}

static int beam_nb(int M, int width) {
    int nb = (512 + M - 1) / M;
    nb = min(nb, (width + 1023) / 1024);
    return max(1, min(nb, BEAM_MAX_NB));
}
// K: the candidates a chunk keeps per row (W' + D W'; 2W for the plain step)
static int64_t beam_ws_layout_k(int M, int V, int K, int max_new, int64_t* off_cand, int64_t* off_hist) {
    const int nb = beam_nb(M, V);
    const int64_t ms = ((int64_t)M * nb * 8 + 15) / 16 * 16;
    const int64_t cand = (int64_t)M * nb * K * 8;
    if (off_cand) *off_cand = ms;
    if (off_hist) *off_hist = ms + cand;
    return ms + cand + (int64_t)M * max_new * 4;
}

// W: the beams of ONE sub-group (W'), D sub-groups per prompt
extern "C" int db1_beam_step_diverse_supported(int V, int64_t ld, int W, int D, int dt) {
    return db1_dt_ok(dt) && V > 0 && V <= BEAM_MAX_V && ld >= V && W >= 1 && D >= 1 && (int64_t)D * W <= BEAM_MAX_W;
}

extern "C" int64_t db1_beam_step_diverse_workspace_bytes(int M, int V, int W, int D, int max_new, int dt) {
    (void)dt;
    if (M <= 0 || V <= 0 || W <= 0 || D <= 0 || (int64_t)D * W > BEAM_MAX_W || max_new <= 0) return 0;
    return beam_ws_layout_k(M, V, W + D * W, max_new, nullptr, nullptr);
}

extern "C" int db1_beam_step_supported(int V, int64_t ld, int W, int dt) { return db1_beam_step_diverse_supported(V, ld, W, 1, dt); }

extern "C" int64_t db1_beam_step_workspace_bytes(int M, int V, int W, int max_new, int dt) {
    (void)dt;
    if (M <= 0 || V <= 0 || W <= 0 || max_new <= 0) return 0;
    return beam_ws_layout_k(M, V, 2 * W, max_new, nullptr, nullptr);
}

// Both steps: G prompts of D sub-groups of W beams (the plain step: D = 1, lam = 0, `diverse` false: beam_group_kernel on G workgroups).
static int beam_step_launch(const char* who, bool diverse, const void* logits, int G, int D, int W, float lam, int V, int64_t ld, int dt, int vocab_lo,
                            int vocab_hi, int eos_id, int pad_id, float length_penalty, const int32_t* t, int max_new, float* beam_score,
                            int32_t* parent, int32_t* tokens, int32_t* pool_tokens, int32_t* pool_len, float* pool_score, int32_t* pool_slot,
                            int32_t* pool_count, int32_t* done, int32_t* switches, int64_t* next_ids, int64_t ids_stride, int32_t* status, void* ws,
                            int64_t ws_bytes, void* stream) {
    if (!db1_beam_step_diverse_supported(V, ld, W, D, dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: V=%d ld=%lld W=%d D=%d dt=%d", who, V, (long long)ld, W, D, dt);
    if (G <= 0 || (int64_t)G * D * W > 65535 || max_new <= 0 || ids_stride < 0)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: G=%d D=%d W=%d max_new=%d ids_stride=%lld", who, G, D, W, max_new, (long long)ids_stride);
    if (vocab_lo < 0 || vocab_hi > V || vocab_lo >= vocab_hi)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: window [%d, %d) is empty or outside [0, %d)", who, vocab_lo, vocab_hi, V);
    if (!(length_penalty > -INFINITY && length_penalty < INFINITY)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: length_penalty %g", who, (double)length_penalty);
    if (!(lam >= 0.f && lam < INFINITY)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: diversity_penalty %g must be finite and >= 0", who, (double)lam);
    if (!logits || !t || !beam_score || !parent || !tokens || !pool_tokens || !pool_len || !pool_score || !pool_slot || !pool_count || !done ||
        !switches || !next_ids || !status)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    const int M = G * D * W;
    int64_t off_cand = 0, off_hist = 0;
    const int64_t need = beam_ws_layout_k(M, V, W + D * W, max_new, &off_cand, &off_hist);
    DB1_NEED_WS(ws, ws_bytes, need, who);
    BeamDivArgs da;
    BeamArgs& a = da.a;
    da.D = D; da.lam = lam;
    a.logits = logits; a.ld = ld; a.G = G * D; a.W = W; a.K = W + D * W; a.M = M; a.V = V; a.vlo = vocab_lo; a.vhi = vocab_hi;
    a.nb = beam_nb(M, vocab_hi - vocab_lo);
    a.span = (vocab_hi - vocab_lo + a.nb - 1) / a.nb;
    a.eos = eos_id; a.pad = pad_id; a.max_new = max_new; a.alpha = length_penalty; a.t = t;
    a.beam_score = beam_score; a.parent = parent; a.tokens = tokens; a.pool_tokens = pool_tokens; a.pool_len = pool_len; a.pool_score = pool_score;
    a.pool_slot = pool_slot; a.pool_count = pool_count; a.done = done; a.switches = switches;
    a.next_ids = reinterpret_cast<long long*>(next_ids); a.ids_stride = ids_stride; a.status = status;
    char* w = static_cast<char*>(ws);
    a.ms = reinterpret_cast<float2*>(w);
    a.cand = reinterpret_cast<unsigned long long*>(w + off_cand);
    a.hist = reinterpret_cast<int*>(w + off_hist);
    hipStream_t st = (hipStream_t)stream;
    DB1_DISPATCH_DT(dt, T, { beam_rows_kernel<T><<<dim3(a.nb, M), BEAM_THREADS, 0, st>>>(a); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) DB1_FAIL(DB1_ERR_HIP, "%s rows: %s", who, hipGetErrorString(e));
    if (diverse) beam_group_diverse_kernel<<<G, BEAM_THREADS, 0, st>>>(da);
    else beam_group_kernel<<<G, BEAM_THREADS, 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) DB1_FAIL(DB1_ERR_HIP, "%s groups: %s", who, hipGetErrorString(e));
    return DB1_OK;
}

extern "C" int db1_beam_step(const void* logits, int G, int W, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, int eos_id, int pad_id,
                             float length_penalty, const int32_t* t, int max_new, float* beam_score, int32_t* parent, int32_t* tokens,
                             int32_t* pool_tokens, int32_t* pool_len, float* pool_score, int32_t* pool_slot, int32_t* pool_count, int32_t* done,
                             int32_t* switches, int64_t* next_ids, int64_t ids_stride, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
    return beam_step_launch("beam_step", false, logits, G, 1, W, 0.f, V, ld, dt, vocab_lo, vocab_hi, eos_id, pad_id, length_penalty, t, max_new,
                            beam_score, parent, tokens, pool_tokens, pool_len, pool_score, pool_slot, pool_count, done, switches, next_ids,
                            ids_stride, status, ws, ws_bytes, stream);
}

extern "C" int db1_beam_step_diverse(const void* logits, int G, int D, int W, float diversity_penalty, int V, int64_t ld, int dt, int vocab_lo,
                                     int vocab_hi, int eos_id, int pad_id, float length_penalty, const int32_t* t, int max_new, float* beam_score,
                                     int32_t* parent, int32_t* tokens, int32_t* pool_tokens, int32_t* pool_len, float* pool_score,
                                     int32_t* pool_slot, int32_t* pool_count, int32_t* done, int32_t* switches, int64_t* next_ids,
                                     int64_t ids_stride, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
    return beam_step_launch("beam_step_diverse", true, logits, G, D, W, diversity_penalty, V, ld, dt, vocab_lo, vocab_hi, eos_id, pad_id,
                            length_penalty, t, max_new, beam_score, parent, tokens, pool_tokens, pool_len, pool_score, pool_slot, pool_count, done,
                            switches, next_ids, ids_stride, status, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------ ring reorder
#define REORDER_THREADS 256
#define REORDER_MAX_Z 4

struct ReorderArgs {
    const long long* rings;
    int L, M, W, cap, mlen, max_t;
    int64_t slot16;             // slot size in 16-byte words
    const int* state;
    const int* t;
    const int* parent;
    const int* done;
    uint4* ws;                  // [L, M, max_t, slot]
};

// grid (M, L, z): row b, layer, every z-th of the t slots.  Rows that keep their own history, rows of done groups, parents outside the row's
// group and a counter outside [0, min(max_t, mlen)] copy nothing.
template <bool GATHER>
__global__ __launch_bounds__(REORDER_THREADS) void ring_reorder_kernel(ReorderArgs a) {
    const int b = blockIdx.x, layer = blockIdx.y;
    const int g = b / a.W;
    const int p = a.parent[b], t = *a.t;
    if (p == b || p < g * a.W || p >= (g + 1) * a.W || (a.done && a.done[g]) || t <= 0 || t > a.max_t || t > a.mlen) return;
    const int s0 = *a.state;
    if (s0 < 0 || s0 >= a.cap) return;
    uint4* ring = reinterpret_cast<uint4*>(a.rings[layer]);
    for (int i = blockIdx.z; i < t; i += gridDim.z) {
        const int slot = (s0 + a.mlen - t + i) % a.cap;
        uint4* stage = a.ws + (((int64_t)layer * a.M + b) * a.max_t + i) * a.slot16;
        if (GATHER) {
            const uint4* src = ring + ((int64_t)p * a.cap + slot) * a.slot16;
            for (int64_t e = threadIdx.x; e < a.slot16; e += REORDER_THREADS) stage[e] = src[e];
        } else {
            uint4* dst = ring + ((int64_t)b * a.cap + slot) * a.slot16;
            for (int64_t e = threadIdx.x; e < a.slot16; e += REORDER_THREADS) dst[e] = stage[e];
        }
    }
}

extern "C" int db1_ring_reorder_supported(int64_t slot_bytes) { return slot_bytes > 0 && slot_bytes % 16 == 0; }

extern "C" int64_t db1_ring_reorder_workspace_bytes(int n_layers, int M, int max_t, int64_t slot_bytes) {
    if (n_layers <= 0 || M <= 0 || max_t <= 0 || slot_bytes <= 0) return 0;
    return (int64_t)n_layers * M * max_t * slot_bytes;
}

extern "C" int db1_ring_reorder(const void* const* rings, int n_layers, int M, int W, int cap, int64_t slot_bytes, const int32_t* state, int mlen,
                                const int32_t* t, int max_t, const int32_t* parent, const int32_t* done, void* ws, int64_t ws_bytes, void* stream) {
    if (!db1_ring_reorder_supported(slot_bytes)) DB1_FAIL(DB1_ERR_UNSUPPORTED, "ring_reorder: slot of %lld bytes", (long long)slot_bytes);
    if (n_layers <= 0 || n_layers > 65535 || M <= 0 || W <= 0 || M % W != 0 || max_t <= 0 || mlen < 0 || max_t > mlen || cap < mlen + 1)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_reorder: L=%d M=%d W=%d cap=%d mlen=%d max_t=%d", n_layers, M, W, cap, mlen, max_t);
    if (!rings || !state || !t || !parent) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_reorder: null buffer");
    DB1_NEED_WS(ws, ws_bytes, db1_ring_reorder_workspace_bytes(n_layers, M, max_t, slot_bytes), "ring_reorder");
    ReorderArgs a;
    a.rings = reinterpret_cast<const long long*>(rings);
    a.L = n_layers; a.M = M; a.W = W; a.cap = cap; a.mlen = mlen; a.max_t = max_t; a.slot16 = slot_bytes / 16;
    a.state = state; a.t = t; a.parent = parent; a.done = done; a.ws = static_cast<uint4*>(ws);
    const dim3 grid(M, n_layers, min(max_t, REORDER_MAX_Z));
    hipStream_t st = (hipStream_t)stream;
    ring_reorder_kernel<true><<<grid, REORDER_THREADS, 0, st>>>(a);
    DB1_CHECK_LAUNCH("ring_reorder gather");
    ring_reorder_kernel<false><<<grid, REORDER_THREADS, 0, st>>>(a);
    DB1_CHECK_LAUNCH("ring_reorder write-back");
    return DB1_OK;
}

// ------------------------------------------------------------------ ring load (continuous batching: a new request takes over a row)
// db1_ring_load_rows, one launch: the mlen projected keys / values of n new requests (src [n, mlen, slot] per layer) go to rows rows[i] of
// every ring, logical key j to slot (state + j) % cap.  A source row is contiguous and so is its target but for the one wrap at the ring's
// end: workgroup (chunk, i, layer) streams LOAD_CHUNK 16-byte words, four loads in flight per thread before the four stores.
#define LOAD_THREADS 256
#define LOAD_UNROLL 4
#define LOAD_CHUNK (LOAD_THREADS * LOAD_UNROLL * 4)

struct LoadArgs {
    const long long* rings;
    const long long* src;
    int M, cap, mlen;
    int64_t slot16;
    const int* rows;
    const int* state;
    int* status;
};

__global__ __launch_bounds__(LOAD_THREADS) void ring_load_rows_kernel(LoadArgs a) {
    const int i = blockIdx.y, layer = blockIdx.z;
    const int row = a.rows[i], s0 = *a.state;
    const bool bad_row = row < 0 || row >= a.M, bad_origin = s0 < 0 || s0 >= a.cap;
    if (bad_row || bad_origin) {     // (block-uniform) never written through: reported once per entry
        if (blockIdx.x == 0 && layer == 0 && threadIdx.x == 0) atomicOr(a.status, (bad_row ? 1 : 0) | (bad_origin ? 2 : 0));
        return;
    }
    const int64_t words = (int64_t)a.mlen * a.slot16, ring_words = (int64_t)a.cap * a.slot16;
    const uint4* src = reinterpret_cast<const uint4*>(a.src[layer]) + (int64_t)i * words;
    uint4* dst = reinterpret_cast<uint4*>(a.rings[layer]) + (int64_t)row * ring_words;
    const int64_t first = (int64_t)s0 * a.slot16;          // (first + e < 2 * ring_words: one wrap at most)
    const int64_t c0 = (int64_t)blockIdx.x * LOAD_CHUNK, c1 = min(c0 + LOAD_CHUNK, words);
    for (int64_t e0 = c0 + threadIdx.x; e0 < c1; e0 += LOAD_THREADS * LOAD_UNROLL) {
        uint4 v[LOAD_UNROLL];
#pragma unroll
        for (int q = 0; q < LOAD_UNROLL; q++) {
            const int64_t e = e0 + q * LOAD_THREADS;
            if (e < c1) v[q] = src[e];
        }
#pragma unroll
        for (int q = 0; q < LOAD_UNROLL; q++) {
            const int64_t e = e0 + q * LOAD_THREADS;
            if (e < c1) {
                int64_t o = first + e;
                o = o >= ring_words ? o - ring_words : o;
                dst[o] = v[q];
            }
        }
    }
}

extern "C" int db1_ring_load_rows_supported(int64_t slot_bytes, int mlen, int cap) {
    return slot_bytes > 0 && slot_bytes % 16 == 0 && mlen > 0 && mlen < cap;
}

extern "C" int db1_ring_load_rows(const void* const* rings, const void* const* src, int n_layers, int M, int n, int cap, int64_t slot_bytes,
                                  const int32_t* state, int mlen, const int32_t* rows, int32_t* status, void* stream) {
    if (!db1_ring_load_rows_supported(slot_bytes, mlen, cap))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "ring_load_rows: slot of %lld bytes, mlen=%d, cap=%d", (long long)slot_bytes, mlen, cap);
    if (n_layers <= 0 || n_layers > 65535 || M <= 0 || n < 0 || n > 65535 || n > M)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_load_rows: L=%d M=%d n=%d", n_layers, M, n);
    if (n == 0) return DB1_OK;
    if (!rings || !src || !state || !rows || !status) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_load_rows: null buffer");
    LoadArgs a;
    a.rings = reinterpret_cast<const long long*>(rings);
    a.src = reinterpret_cast<const long long*>(src);
    a.M = M; a.cap = cap; a.mlen = mlen; a.slot16 = slot_bytes / 16;
    a.rows = rows; a.state = state; a.status = status;
    const int64_t words = (int64_t)mlen * a.slot16;
    const int64_t chunks = (words + LOAD_CHUNK - 1) / LOAD_CHUNK;
    if (chunks > 0x7fffffff) DB1_FAIL(DB1_ERR_BAD_SHAPE, "ring_load_rows: a row of %lld bytes", (long long)(words * 16));
    ring_load_rows_kernel<<<dim3((unsigned)chunks, n, n_layers), LOAD_THREADS, 0, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH("ring_load_rows");
    return DB1_OK;
}
