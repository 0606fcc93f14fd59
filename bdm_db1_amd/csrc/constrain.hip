// Decoding constraints on the device (db1_constrain_logits, include/db1_hip.h; tests/constraint_rule.py restates the rule in NumPy): the
// repetition penalty, the no-repeat n-gram ban, the banned-id list and the minimum length, applied IN PLACE to the step's logits before
// db1_select_tokens / db1_select_tokens_slots / db1_beam_step read them.  Those kernels take only finite logits as candidates, so a ban is
// a -inf store and nothing in them changes.
//
// One workgroup of 256 threads per logits row.  The row's history (the t tokens it has generated, t < max_new <= 4096) is staged in LDS;
// every history position i belongs to thread i % 256.  Only O(t + n_bad) columns of the row are touched: the vocabulary is never swept.
// The first-occurrence test of position i scans the i positions before it (16 per trip, leaving at the first copy): up to t^2 / 512
// tokens per thread, nothing at caption lengths, the dominant term for a long history of distinct tokens (profiles/constraints_caption_1p3b.txt).
// No atomics: position i penalises its column only if no earlier position holds the same token (decided from the LDS copy: all lanes read
// the same word, a broadcast), so every penalised column has exactly one reader and one writer; after a barrier the bans store -inf, and
// duplicate bans write the same bits.  t, hist, finished and row_map are only read: the launch can be captured and replayed.
#include "db1_common.h"

#define CON_THREADS 256
#define CON_MAX_NEW 4096                   // the LDS staging: 16 KB of history per workgroup (the models' mem_len is far below)
#define CON_MAX_BAD 1024

struct ConArgs {
    void* logits;
    int64_t ld;
    int V, max_new, n_slots, t_per_slot;
    const int* t;
    const int* hist;
    const int* finished;
    const int* row_map;
    float theta, inv_theta;
    int ngram;
    const int* bad;
    int n_bad, eos, min_new;
};

template <typename T>
__global__ __launch_bounds__(CON_THREADS) void constrain_logits_kernel(ConArgs a) {
    __shared__ __attribute__((aligned(16))) int h[CON_MAX_NEW];
    const int4* h4 = reinterpret_cast<const int4*>(h);
    const int tid = threadIdx.x;
    // the guard (block-uniform): a slot that does not exist, a finished / vacant row, a counter outside [0, max_new)
    const int slot = a.row_map ? a.row_map[blockIdx.x] : (int)blockIdx.x;
    if (slot < 0 || slot >= a.n_slots) return;
    if (a.finished && a.finished[slot]) return;
    const int t = a.t_per_slot ? a.t[slot] : a.t[0];
    if (t < 0 || t >= a.max_new) return;
    T* lg = reinterpret_cast<T*>(a.logits) + (int64_t)blockIdx.x * a.ld;
    const int* hs = a.hist + (int64_t)slot * a.max_new;
    for (int i = tid; i < t; i += CON_THREADS) h[i] = hs[i];
    __syncthreads();
    // repetition penalty: the first occurrence of every distinct token rescales its column (a single fp32 multiplication, rounded to T)
    if (a.theta != 1.f) {
        for (int i = tid; i < t; i += CON_THREADS) {
            const int c = h[i];
            if (c < 0 || c >= a.V) continue;
            // an earlier copy?  16 tokens per trip (four 16-byte LDS reads, all lanes the same address), leaving at the first trip with a hit
            bool dup = false;
            const int quads = i >> 2;
            for (int q = 0; q < quads && !dup; q += 4) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (q + u < quads) {
                        const int4 v = h4[q + u];
                        dup = dup || v.x == c || v.y == c || v.z == c || v.w == c;
                    }
                }
            }
            for (int j = quads * 4; j < i; j++) dup = dup || h[j] == c;
            if (dup) continue;
            const float l = ldf<T>(lg + c);
            if ((__float_as_uint(l) & 0x7f800000u) == 0x7f800000u) continue;      // NaN, +-inf: left as stored
            stf<T>(lg + c, l > 0.f ? l * a.inv_theta : l * a.theta);
        }
    }
    __syncthreads();      // the penalised values are in memory before a ban of the same column overwrites them
    const float ninf = -INFINITY;
    // no-repeat n-gram: position i ends an earlier copy of the last n - 1 tokens -> its token would repeat that n-gram
    if (a.ngram > 0 && a.ngram <= t) {      // (n - 1 tokens before position i >= n - 1, and i < t)
        const int n1 = a.ngram - 1;
        for (int i = n1 + tid; i < t; i += CON_THREADS) {
            bool same = true;
            for (int k = 1; k <= n1; k++) same = same && h[i - k] == h[t - k];
            const int c = h[i];
            if (same && c >= 0 && c < a.V) stf<T>(lg + c, ninf);
        }
    }
    for (int i = tid; i < a.n_bad; i += CON_THREADS) {
        const int c = a.bad[i];
        if (c >= 0 && c < a.V) stf<T>(lg + c, ninf);
    }
    if (tid == 0 && a.eos >= 0 && a.eos < a.V && t < a.min_new) stf<T>(lg + a.eos, ninf);
}

extern "C" int db1_constrain_logits_supported(int V, int64_t ld, int max_new, int n_bad, int dt) {
    return db1_dt_ok(dt) && V > 0 && ld >= V && max_new >= 1 && max_new <= CON_MAX_NEW && n_bad >= 0 && n_bad <= CON_MAX_BAD;
}

extern "C" int64_t db1_constrain_logits_workspace_bytes(int M, int V, int max_new, int n_bad, int dt) {
    (void)M; (void)V; (void)max_new; (void)n_bad; (void)dt;
    return 0;
}

extern "C" int db1_constrain_logits(void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, int t_per_slot, const int32_t* hist,
                                    int max_new, const int32_t* finished, const int32_t* row_map, int n_slots, float theta, float inv_theta,
                                    int ngram, const int32_t* bad, int n_bad, int eos_id, int min_new, void* ws, int64_t ws_bytes,
                                    void* stream) {
    (void)ws; (void)ws_bytes;
    const char* who = "constrain_logits";
    if (!db1_dt_ok(dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dt);
    if (M <= 0 || M > 65535 || V <= 0 || ld < V || max_new <= 0 || n_bad < 0 || n_slots <= 0 || (!row_map && n_slots != M))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d V=%d ld=%lld max_new=%d n_bad=%d n_slots=%d%s", who, M, V, (long long)ld, max_new, n_bad, n_slots,
                 !row_map ? " (no row_map: n_slots must equal M)" : "");
    if (!db1_constrain_logits_supported(V, ld, max_new, n_bad, dt))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: max_new=%d (at most %d) n_bad=%d (at most %d)", who, max_new, CON_MAX_NEW, n_bad, CON_MAX_BAD);
    if (!logits || !t || !hist || (n_bad > 0 && !bad)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (!(theta > 0.f && theta < INFINITY) || !(inv_theta > 0.f && inv_theta < INFINITY))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: theta %g (1 / theta %g) must be finite and > 0", who, (double)theta, (double)inv_theta);
    if (ngram < 0 || min_new < 0) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: ngram %d min_new %d must be >= 0", who, ngram, min_new);
    if (theta == 1.f && ngram == 0 && n_bad == 0 && (eos_id < 0 || min_new == 0)) return DB1_OK;      // no constraint: no launch
    ConArgs a = {};
    a.logits = logits; a.ld = ld; a.V = V; a.max_new = max_new; a.n_slots = n_slots; a.t_per_slot = t_per_slot != 0;
    a.t = t; a.hist = hist; a.finished = finished; a.row_map = row_map;
    a.theta = theta; a.inv_theta = inv_theta; a.ngram = ngram; a.bad = bad; a.n_bad = n_bad; a.eos = eos_id; a.min_new = min_new;
    hipStream_t st = (hipStream_t)stream;
    DB1_DISPATCH_DT(dt, T, { constrain_logits_kernel<T><<<M, CON_THREADS, 0, st>>>(a); });
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}
