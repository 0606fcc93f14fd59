// Speculative decoding on the device (db1_spec_accept, db1_spec_commit; include/db1_hip.h states the rule, tests/spec_rule.py restates it in
// NumPy).  A step feeds every row one real token and k guessed ones; db1_spec_pick (csrc/select.hip) has chosen, for every position, the token
// the plain selection would have chosen there.  db1_spec_accept counts how many of those choices the step may keep (a position's choice is
// only valid if every guess before it was right), commits that many tokens of every row, and proposes the next k guesses; db1_spec_commit
// advances the token counter and takes the ring's origin back over the positions that were not kept.
//
// db1_spec_accept: one workgroup of 256 threads per row.  EVERY workgroup derives the step's accepted count n_acc from sel, hit and *t
// alone -- arrays no workgroup of this launch writes -- so the workgroups need not talk: thread i walks rows i, i + 256, ..., one fixed-order
// block minimum follows.  Thread 0 then keeps its row's books (at most 16 tokens), all threads stage the row's history (the prompt's text
// and the output up to the new counter, at most 4096 tokens) in LDS -- the tokens of this step from sel, not from the global stores thread 0
// has just issued -- and the draft lookup tests the candidate positions 256 at a time, longest n-gram first, with one fixed-order block maximum
// per n-gram length.  No atomics, no workspace; nothing is read back: both launches can be captured and replayed.
#include "db1_common.h"

#define SPEC_THREADS 256
#define SPEC_WAVES (SPEC_THREADS / 64)
#define SPEC_MAX_Q 16
#define SPEC_MAX_HIST 4096
#define SPEC_MAX_NGRAM 8
#define SPEC_NONE (-1)
#define SPEC_SKIP (-2)

struct SpecArgs {
    int M, q_in, Q, eos, pad, V, max_new, ctx_cap, ng_min, ng_max;
    const int* t;
    const int* sel;
    const int* hit;
    const float* lp;
    int* finished;
    int* lengths;
    int* out;
    int* status;
    float* logprob;
    float* sum_logprob;
    long long* ids;
    const int* ctx;
    const int* ctx_len;
    const int* script;
    int* n_acc;
};

// fixed order: the wave butterflies, then the four wave results read in order; `ph` alternates between two slot sets (one barrier each)
__device__ __forceinline__ int spec_block_max(int x, int (&red)[2][SPEC_WAVES], int& ph) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
    if ((threadIdx.x & 63) == 0) red[ph][threadIdx.x >> 6] = x;
    __syncthreads();
    int r = red[ph][0];
#pragma unroll
    for (int w = 1; w < SPEC_WAVES; w++) r = max(r, red[ph][w]);
    ph ^= 1;
    return r;
}

// the emissions of a live row: it stops after position i when the row ends there (no candidate, EOS), at the last token index, at the last
// position of the call, or when the next column's guess was not the pick
__device__ __forceinline__ int spec_row_emits(const SpecArgs& a, int row, int t) {
    const int* s = a.sel + (int64_t)row * a.Q;
    const int* h = a.hit + (int64_t)row * a.Q;
    int i = 0;
    for (;; i++) {
        const int v = s[i];
        if (v == SPEC_NONE || v == a.eos || t + i + 1 == a.max_new || i == a.q_in - 1 || h[i] == 0) break;
    }
    return i + 1;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_accept_kernel(SpecArgs a) {
    __shared__ int h[SPEC_MAX_HIST];
    __shared__ int red[2][SPEC_WAVES];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int t = *a.t;
    if (t < 0 || t > a.max_new) {                    // (block-uniform) the counter left its range: reported on every row, nothing committed
        if (tid == 0) {
            a.status[r] |= 2;
            if (r == 0) *a.n_acc = 0;
        }
        return;
    }
    if (t == a.max_new) {                            // a replay past the end, before the host's next look: nothing at all
        if (tid == 0 && r == 0) *a.n_acc = 0;
        return;
    }
    int ph = 0;
    // n_acc = the fewest emissions among the rows that were live on entry (sel[row, 0] is SKIP exactly for the others, as t < max_new)
    int mine = -0x7fffffff;                          // (the maximum of the negated counts)
    for (int row = tid; row < a.M; row += SPEC_THREADS)
        if (a.sel[(int64_t)row * a.Q] != SPEC_SKIP) mine = max(mine, -spec_row_emits(a, row, t));
    const int m = spec_block_max(mine, red, ph);
    const int n_acc = m == -0x7fffffff ? 0 : -m;     // 1 .. q_in, and t + n_acc <= max_new; 0: no live row
    const int* s = a.sel + (int64_t)r * a.Q;
    const bool live = s[0] != SPEC_SKIP;
    const int last = n_acc > 0 && live ? s[n_acc - 1] : 0;
    const bool fin = !live || (n_acc > 0 && (last == SPEC_NONE || last == a.eos));
    if (tid == 0) {
        if (r == 0) *a.n_acc = n_acc;
        const int64_t row = (int64_t)r * a.max_new + t;
        if (!live) {
            for (int i = 0; i < n_acc; i++) {
                a.out[row + i] = a.pad;
                if (a.logprob) a.logprob[row + i] = 0.f;
            }
        } else if (n_acc > 0) {
            int len = a.lengths[r];
            float sum = a.logprob ? a.sum_logprob[r] : 0.f;
            for (int i = 0; i < n_acc; i++) {
                const int v = s[i];
                if (v == SPEC_NONE) {
                    a.out[row + i] = a.pad;
                    if (a.logprob) a.logprob[row + i] = 0.f;
                    a.status[r] |= 1;
                } else {
                    a.out[row + i] = v;
                    if (a.logprob) {
                        const float l = a.lp[(int64_t)r * a.Q + i];
                        a.logprob[row + i] = l;
                        sum += l;                    // (one fp32 add per token, in token order: the plain form's running sum)
                    }
                    if (v != a.eos) len++;
                }
            }
            a.lengths[r] = len;
            if (a.logprob) a.sum_logprob[r] = sum;
            if (fin) a.finished[r] = 1;
        }
        if (n_acc > 0) a.ids[(int64_t)r * a.Q] = fin ? a.pad : last;
    }
    // the drafts for token indices t2 .. t2 + Q - 2 over the history h = [the prompt's text, out[r, :t2]]
    const int k = a.Q - 1, t2 = t + n_acc;
    long long* d = a.ids + (int64_t)r * a.Q + 1;
    if (fin) {                                       // (block-uniform)
        if (tid < k) d[tid] = a.pad;
        return;
    }
    int nc = a.ctx ? a.ctx_len[r] : 0;
    nc = min(max(nc, 0), a.ctx_cap);
    const int n = nc + t2;                           // <= ctx_cap + max_new <= 4096 (the launch checked)
    for (int j = tid; j < nc; j += SPEC_THREADS) h[j] = a.ctx[(int64_t)r * a.ctx_cap + j];
    for (int j = tid; j < t; j += SPEC_THREADS) h[nc + j] = a.out[(int64_t)r * a.max_new + j];
    if (tid < n_acc) h[nc + t + tid] = s[tid];       // (a live row that has not ended: every committed pick is a token)
    __syncthreads();
    if (n == 0) {                                    // (only with n_acc == 0 at t == 0: nothing to look at)
        if (tid < k) d[tid] = a.pad;
        return;
    }
    if (a.script) {
        if (tid < k) {
            const int c = t2 + tid;
            const int v = c < a.max_new ? a.script[(int64_t)r * a.max_new + c] : -1;
            d[tid] = (v >= 0 && v < a.V) ? v : h[n - 1];
        }
        return;
    }
    int bp = -1, bg = 0;
    for (int g = a.ng_max; g >= a.ng_min; g--) {
        if (n <= g) continue;                        // (block-uniform)
        int p_best = -1;
        for (int p = tid; p <= n - g - 1; p += SPEC_THREADS) {
            bool same = true;
            for (int x = 0; x < g; x++) same = same && h[p + x] == h[n - g + x];
            if (same) p_best = p;                    // (ascending p: the thread's latest)
        }
        bp = spec_block_max(p_best, red, ph);
        if (bp >= 0) {
            bg = g;
            break;
        }
    }
    if (tid < k) {
        if (bp < 0) d[tid] = h[n - 1];
        else {
            const int from = bp + bg, L = n - from;  // L >= 1; a continuation that reaches the end of the history wraps: a loop goes on
            d[tid] = h[from + tid % L];
        }
    }
}

__global__ void spec_commit_kernel(int* t, const int* n_acc, int* hist, int q_in, int* ring_state, int cap) {
    int n = *n_acc;
    n = min(max(n, 0), q_in);
    *t += n;
    if (ring_state) *ring_state = (*ring_state + cap - (q_in - n)) % cap;
    if (hist) hist[n] += 1;
}

extern "C" int db1_spec_accept_supported(int Q, int ctx_cap, int max_new, int ngram_min, int ngram_max) {
    return Q >= 2 && Q <= SPEC_MAX_Q && ctx_cap >= 0 && max_new >= 1 && (int64_t)ctx_cap + max_new <= SPEC_MAX_HIST && ngram_min >= 1 &&
           ngram_min <= ngram_max && ngram_max <= SPEC_MAX_NGRAM;
}

extern "C" int db1_spec_accept(int M, int q_in, int Q, int eos_id, int pad_id, int V, int max_new, const int32_t* t, const int32_t* sel,
                               const int32_t* hit, const float* lp, int32_t* finished, int32_t* lengths, int32_t* out, int32_t* status,
                               float* logprob, float* sum_logprob, int64_t* ids, const int32_t* ctx, const int32_t* ctx_len, int ctx_cap,
                               const int32_t* script, int ngram_min, int ngram_max, int32_t* n_acc, void* stream) {
    const char* who = "spec_accept";
    if (M <= 0 || Q < 2 || Q > SPEC_MAX_Q || q_in < 1 || q_in > Q || (int64_t)M * Q > 65535 || V <= 0 || max_new <= 0 || ctx_cap < 0)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d q_in=%d Q=%d V=%d max_new=%d ctx_cap=%d (1 <= q_in <= Q, 2 <= Q <= %d, M * Q <= 65535)", who, M, q_in, Q,
                 V, max_new, ctx_cap, SPEC_MAX_Q);
    if (ngram_min < 1 || ngram_max > SPEC_MAX_NGRAM || ngram_min > ngram_max)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: n-gram range [%d, %d] (1 <= min <= max <= %d)", who, ngram_min, ngram_max, SPEC_MAX_NGRAM);
    if (!db1_spec_accept_supported(Q, ctx_cap, max_new, ngram_min, ngram_max))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: ctx_cap %d + max_new %d exceeds the %d tokens of history a row can stage", who, ctx_cap, max_new, SPEC_MAX_HIST);
    if (!t || !sel || !hit || !finished || !lengths || !out || !status || !ids || !n_acc) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if ((lp == nullptr) != (logprob == nullptr) || (logprob == nullptr) != (sum_logprob == nullptr))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: lp, logprob and sum_logprob go together", who);
    if ((ctx == nullptr) != (ctx_len == nullptr) || (ctx != nullptr && ctx_cap < 1))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: ctx and ctx_len go together, with ctx_cap >= 1", who);
    SpecArgs a = {};
    a.M = M; a.q_in = q_in; a.Q = Q; a.eos = eos_id; a.pad = pad_id; a.V = V; a.max_new = max_new; a.ctx_cap = ctx ? ctx_cap : 0;
    a.ng_min = ngram_min; a.ng_max = ngram_max; a.t = t; a.sel = sel; a.hit = hit; a.lp = lp; a.finished = finished; a.lengths = lengths;
    a.out = out; a.status = status; a.logprob = logprob; a.sum_logprob = sum_logprob; a.ids = reinterpret_cast<long long*>(ids);
    a.ctx = ctx; a.ctx_len = ctx_len; a.script = script; a.n_acc = n_acc;
    spec_accept_kernel<<<M, SPEC_THREADS, 0, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}

extern "C" int db1_spec_commit_supported(int Q, int cap) { return Q >= 2 && Q <= SPEC_MAX_Q && cap > 0; }

extern "C" int db1_spec_commit(int32_t* t, const int32_t* n_acc, int32_t* hist, int q_in, int Q, int32_t* ring_state, int cap, void* stream) {
    const char* who = "spec_commit";
    if (Q < 2 || Q > SPEC_MAX_Q || q_in < 1 || q_in > Q) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: q_in=%d Q=%d (1 <= q_in <= Q, 2 <= Q <= %d)", who, q_in, Q, SPEC_MAX_Q);
    if (!t || !n_acc) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (ring_state && (cap <= 0 || cap < q_in)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: cap %d (a ring of at least q_in = %d slots)", who, cap, q_in);
    spec_commit_kernel<<<1, 1, 0, (hipStream_t)stream>>>(t, n_acc, hist, q_in, ring_state, cap);
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}
