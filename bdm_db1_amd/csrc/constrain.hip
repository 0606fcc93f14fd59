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
//
// db1_constrain_logits_pen (tests/penalty_rule.py) is the PEN instantiation of the same kernel: the thread that holds a token's first
// occurrence also counts its later copies in the staged history (n_c) and takes freq * n_c + pres off the rescaled value before its single
// store -- three fp32 operations that must each round, hence ``rounded`` below: the build contracts a * b + c into one fma --; then,
// between two barriers of its own, the bias list adds to the STORED values (one writer per column in each phase, so still no atomics); the
// bans come last.  The count scan reads the t - i - 1 tokens after position i, 16 bytes at a time: about t^2 / 512 tokens per thread for a
// history of distinct tokens, as much again as the first-occurrence test.  The plain instantiation holds none of this.
//
// db1_constrain_logits_slots_per (tests/slot_constraints_rule.py) is the PER instantiation of the PEN kernel: what the other two take as
// launch scalars and one shared list each is read per SLOT from a 32-byte record and the slot's own rows of the list tables, after the
// guard and before the history is staged (all of it block-uniform).  A launch cannot validate device data, so the kernel does: an invalid
// record ends the slot (status bit 3, finished = 1, written by one thread) with its logits untouched; a record that edits nothing leaves
// before the staging.  From there on the code is the PEN code over locals, so a valid slot's bits are db1_constrain_logits_pen's.
#include "db1_common.h"
#include <type_traits>

#define CON_THREADS 256
#define CON_MAX_NEW 4096                   // the LDS staging: 16 KB of history per workgroup (the models' mem_len is far below)
#define CON_MAX_BAD 1024
#define CON_MAX_BIAS 1024

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

struct ConPerArgs {                        // the PER instantiation: the record and the list tables instead of the scalars
    void* logits;
    int64_t ld;
    int V, max_new, n_slots;
    const int* t;
    const int* hist;
    int* finished;
    int* status;
    const int* row_map;
    const int* cons;                       // [n_slots, 8], 32-byte aligned: the record of include/db1_hip.h
    const int* bad;                        // [n_slots, bad_cap]
    const int* bias_ids;                   // [n_slots, bias_cap]
    const float* bias_val;
    int bad_cap, bias_cap, eos;
};

struct ConPenArgs : ConArgs {              // what the PEN instantiation reads on top
    float freq, pres;
    const int* bias_ids;
    const float* bias_val;
    int n_bias;
};

// The build's -ffp-contract=fast lets the backend fuse a multiplication into the addition that follows whatever the source says (a
// contract(off) pragma only keeps the front end from doing it).  A value that has passed through an empty asm statement is opaque to that
// combiner: the product is rounded before it is used.
__device__ __forceinline__ float rounded(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

template <typename T, bool PEN, bool PER = false>
__global__ __launch_bounds__(CON_THREADS) void constrain_logits_kernel(
    typename std::conditional<PER, ConPerArgs, typename std::conditional<PEN, ConPenArgs, ConArgs>::type>::type a) {
    static_assert(PEN || !PER, "PER is a mode of the PEN kernel");
    __shared__ __attribute__((aligned(16))) int h[CON_MAX_NEW];
    const int4* h4 = reinterpret_cast<const int4*>(h);
    const int tid = threadIdx.x;
    // the guard (block-uniform): a slot that does not exist, a finished / vacant row, a counter outside [0, max_new)
    const int slot = a.row_map ? a.row_map[blockIdx.x] : (int)blockIdx.x;
    if (slot < 0 || slot >= a.n_slots) return;
    if (a.finished && a.finished[slot]) return;
    int t;
    if constexpr (PER) t = a.t[slot];
    else t = a.t_per_slot ? a.t[slot] : a.t[0];
    if (t < 0 || t >= a.max_new) return;
    // what the phases below read: the launch's scalars and lists, or (PER) the slot's record and its rows of the list tables
    float theta, inv_theta, freq = 0.f, pres = 0.f;
    int ngram, n_bad, min_new, n_bias = 0;
    const int* bad;
    const int* bias_ids = nullptr;
    const float* bias_val = nullptr;
    if constexpr (PER) {
        const int4* rec = reinterpret_cast<const int4*>(a.cons + (int64_t)slot * 8);
        const int4 w0 = rec[0], w1 = rec[1];
        theta = __int_as_float(w0.x); inv_theta = __int_as_float(w0.y); ngram = w0.z; min_new = w0.w;
        freq = __int_as_float(w1.x); pres = __int_as_float(w1.y); n_bad = w1.z; n_bias = w1.w;
        const bool ok = theta > 0.f && theta < INFINITY && inv_theta > 0.f && inv_theta < INFINITY && ngram >= 0 && min_new >= 0 &&
                        fabsf(freq) < INFINITY && fabsf(pres) < INFINITY && n_bad >= 0 && n_bad <= a.bad_cap && n_bias >= 0 && n_bias <= a.bias_cap;
        if (!ok) {      // the slot ends here, its logits as they are: the selection that follows feeds pad_id forward
            if (tid == 0) {
                a.status[slot] |= 8;
                a.finished[slot] = 1;
            }
            return;
        }
        if (theta == 1.f && freq == 0.f && pres == 0.f && ngram == 0 && n_bad == 0 && n_bias == 0 && (a.eos < 0 || min_new == 0)) return;
        bad = a.bad + (int64_t)slot * a.bad_cap;             // (a capacity of 0: never read)
        bias_ids = a.bias_ids + (int64_t)slot * a.bias_cap;
        bias_val = a.bias_val + (int64_t)slot * a.bias_cap;
    } else {
        theta = a.theta; inv_theta = a.inv_theta; ngram = a.ngram; n_bad = a.n_bad; min_new = a.min_new; bad = a.bad;
        if constexpr (PEN) {
            freq = a.freq; pres = a.pres; n_bias = a.n_bias; bias_ids = a.bias_ids; bias_val = a.bias_val;
        }
    }
    T* lg = reinterpret_cast<T*>(a.logits) + (int64_t)blockIdx.x * a.ld;
    const int* hs = a.hist + (int64_t)slot * a.max_new;
    for (int i = tid; i < t; i += CON_THREADS) h[i] = hs[i];
    __syncthreads();
    // repetition penalty: the first occurrence of every distinct token rescales its column (a single fp32 multiplication, rounded to T)
    bool edit = theta != 1.f;
    if constexpr (PEN) edit = edit || freq != 0.f || pres != 0.f;
    if (edit) {
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
            if constexpr (!PEN) {
                stf<T>(lg + c, l > 0.f ? l * inv_theta : l * theta);
            } else {
                // n_c: this copy and those after it (none before: it is the first).  Single tokens up to the next 16-byte boundary, 16-byte
                // reads up to the last whole one below t (the words past t in LDS were never written), single tokens again
                int n = 1, j = i + 1;
                const int j4 = min((j + 3) & ~3, t), qend = t >> 2;
                for (; j < j4; j++) n += h[j] == c;
                for (int q = j >> 2; q < qend; q++) {
                    const int4 v = h4[q];
                    n += (v.x == c) + (v.y == c) + (v.z == c) + (v.w == c);
                }
                for (j = max(j4, qend << 2); j < t; j++) n += h[j] == c;
                // three roundings, not two: the products pass through ``rounded`` before anything is added to them
                float v = l;
                if (theta != 1.f) v = rounded(l > 0.f ? v * inv_theta : v * theta);
                if (freq != 0.f || pres != 0.f) {
                    float p = rounded((float)n * freq);
                    p = p + pres;
                    v = v - p;
                }
                stf<T>(lg + c, v);
            }
        }
    }
    __syncthreads();      // the penalised values are in memory before a ban of the same column overwrites them
    if constexpr (PEN) {
        // the bias: distinct ids, so one reader and one writer per column; it reads what the penalties stored
        for (int i = tid; i < n_bias; i += CON_THREADS) {
            const int c = bias_ids[i];
            if (c < 0 || c >= a.V) continue;
            const float l = ldf<T>(lg + c);
            if ((__float_as_uint(l) & 0x7f800000u) == 0x7f800000u) continue;
            stf<T>(lg + c, l + bias_val[i]);
        }
        __syncthreads();  // ... and the biased values before a ban
    }
    const float ninf = -INFINITY;
    // no-repeat n-gram: position i ends an earlier copy of the last n - 1 tokens -> its token would repeat that n-gram
    if (ngram > 0 && ngram <= t) {      // (n - 1 tokens before position i >= n - 1, and i < t)
        const int n1 = ngram - 1;
        for (int i = n1 + tid; i < t; i += CON_THREADS) {
            bool same = true;
            for (int k = 1; k <= n1; k++) same = same && h[i - k] == h[t - k];
            const int c = h[i];
            if (same && c >= 0 && c < a.V) stf<T>(lg + c, ninf);
        }
    }
    for (int i = tid; i < n_bad; i += CON_THREADS) {
        const int c = bad[i];
        if (c >= 0 && c < a.V) stf<T>(lg + c, ninf);
    }
    if (tid == 0 && a.eos >= 0 && a.eos < a.V && t < min_new) stf<T>(lg + a.eos, ninf);
}

extern "C" int db1_constrain_logits_supported(int V, int64_t ld, int max_new, int n_bad, int dt) {
    return db1_dt_ok(dt) && V > 0 && ld >= V && max_new >= 1 && max_new <= CON_MAX_NEW && n_bad >= 0 && n_bad <= CON_MAX_BAD;
}

extern "C" int64_t db1_constrain_logits_workspace_bytes(int M, int V, int max_new, int n_bad, int dt) {
    (void)M; (void)V; (void)max_new; (void)n_bad; (void)dt;
    return 0;
}

static int constrain_launch(const char* who, void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, int t_per_slot, const int32_t* hist,
                            int max_new, const int32_t* finished, const int32_t* row_map, int n_slots, float theta, float inv_theta, int ngram,
                            const int32_t* bad, int n_bad, int eos_id, int min_new, bool pen, float freq, float pres, const int32_t* bias_ids,
                            const float* bias_val, int n_bias, void* stream);

extern "C" int db1_constrain_logits(void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, int t_per_slot, const int32_t* hist,
                                    int max_new, const int32_t* finished, const int32_t* row_map, int n_slots, float theta, float inv_theta,
                                    int ngram, const int32_t* bad, int n_bad, int eos_id, int min_new, void* ws, int64_t ws_bytes,
                                    void* stream) {
    (void)ws; (void)ws_bytes;
    return constrain_launch("constrain_logits", logits, M, V, ld, dt, t, t_per_slot, hist, max_new, finished, row_map, n_slots, theta, inv_theta, ngram,
                            bad, n_bad, eos_id, min_new, false, 0.f, 0.f, nullptr, nullptr, 0, stream);
}

extern "C" int db1_constrain_logits_pen_supported(int V, int64_t ld, int max_new, int n_bad, int n_bias, int dt) {
    return db1_constrain_logits_supported(V, ld, max_new, n_bad, dt) && n_bias >= 0 && n_bias <= CON_MAX_BIAS;
}

extern "C" int64_t db1_constrain_logits_pen_workspace_bytes(int M, int V, int max_new, int n_bad, int n_bias, int dt) {
    (void)M; (void)V; (void)max_new; (void)n_bad; (void)n_bias; (void)dt;
    return 0;
}

extern "C" int db1_constrain_logits_pen(void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, int t_per_slot, const int32_t* hist,
                                        int max_new, const int32_t* finished, const int32_t* row_map, int n_slots, float theta, float inv_theta,
                                        int ngram, const int32_t* bad, int n_bad, int eos_id, int min_new, float freq, float pres,
                                        const int32_t* bias_ids, const float* bias_val, int n_bias, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    return constrain_launch("constrain_logits_pen", logits, M, V, ld, dt, t, t_per_slot, hist, max_new, finished, row_map, n_slots, theta, inv_theta,
                            ngram, bad, n_bad, eos_id, min_new, true, freq, pres, bias_ids, bias_val, n_bias, stream);
}

// the checks and the launch of both entry points.  ``pen`` with freq == pres == 0 and no bias is the plain rule and launches the plain
// instantiation: the bits of db1_constrain_logits by construction
static int constrain_launch(const char* who, void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, int t_per_slot, const int32_t* hist,
                            int max_new, const int32_t* finished, const int32_t* row_map, int n_slots, float theta, float inv_theta, int ngram,
                            const int32_t* bad, int n_bad, int eos_id, int min_new, bool pen, float freq, float pres, const int32_t* bias_ids,
                            const float* bias_val, int n_bias, void* stream) {
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
    if (pen) {
        if (n_bias < 0) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: n_bias=%d", who, n_bias);
        if (n_bias > CON_MAX_BIAS) DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: n_bias=%d (at most %d)", who, n_bias, CON_MAX_BIAS);
        if (n_bias > 0 && (!bias_ids || !bias_val)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null bias buffer", who);
        if (!(fabsf(freq) < INFINITY) || !(fabsf(pres) < INFINITY))
            DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: freq %g pres %g must be finite", who, (double)freq, (double)pres);
        pen = freq != 0.f || pres != 0.f || n_bias > 0;
    }
    if (!pen && theta == 1.f && ngram == 0 && n_bad == 0 && (eos_id < 0 || min_new == 0)) return DB1_OK;      // no constraint: no launch
    ConPenArgs a = {};
    a.logits = logits; a.ld = ld; a.V = V; a.max_new = max_new; a.n_slots = n_slots; a.t_per_slot = t_per_slot != 0;
    a.t = t; a.hist = hist; a.finished = finished; a.row_map = row_map;
    a.theta = theta; a.inv_theta = inv_theta; a.ngram = ngram; a.bad = bad; a.n_bad = n_bad; a.eos = eos_id; a.min_new = min_new;
    a.freq = freq; a.pres = pres; a.bias_ids = bias_ids; a.bias_val = bias_val; a.n_bias = n_bias;
    hipStream_t st = (hipStream_t)stream;
    if (pen) DB1_DISPATCH_DT(dt, T, { constrain_logits_kernel<T, true><<<M, CON_THREADS, 0, st>>>(a); });
    else DB1_DISPATCH_DT(dt, T, { constrain_logits_kernel<T, false><<<M, CON_THREADS, 0, st>>>(static_cast<const ConArgs&>(a)); });
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}

extern "C" int db1_constrain_logits_slots_supported(int V, int64_t ld, int max_new, int bad_cap, int bias_cap, int dt) {
    return db1_constrain_logits_pen_supported(V, ld, max_new, bad_cap, bias_cap, dt);
}

extern "C" int64_t db1_constrain_logits_slots_workspace_bytes(int M, int V, int max_new, int bad_cap, int bias_cap, int dt) {
    (void)M; (void)V; (void)max_new; (void)bad_cap; (void)bias_cap; (void)dt;
    return 0;
}

// the per-slot form: what can be checked at a launch is checked here in the manner of constrain_launch; the records are the kernel's to check
extern "C" int db1_constrain_logits_slots_per(void* logits, int M, int V, int64_t ld, int dt, const int32_t* t, const int32_t* hist, int max_new,
                                              int32_t* finished, int32_t* status, const int32_t* row_map, int n_slots, const int32_t* cons,
                                              const int32_t* bad, int bad_cap, const int32_t* bias_ids, const float* bias_val, int bias_cap,
                                              int eos_id, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    const char* who = "constrain_logits_slots_per";
    if (!db1_dt_ok(dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dt);
    if (M <= 0 || M > 65535 || V <= 0 || ld < V || max_new <= 0 || bad_cap < 0 || bias_cap < 0 || n_slots <= 0 || (!row_map && n_slots != M))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d V=%d ld=%lld max_new=%d bad_cap=%d bias_cap=%d n_slots=%d%s", who, M, V, (long long)ld, max_new,
                 bad_cap, bias_cap, n_slots, !row_map ? " (no row_map: n_slots must equal M)" : "");
    if (!db1_constrain_logits_slots_supported(V, ld, max_new, bad_cap, bias_cap, dt))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: max_new=%d (at most %d) bad_cap=%d (at most %d) bias_cap=%d (at most %d)", who, max_new, CON_MAX_NEW,
                 bad_cap, CON_MAX_BAD, bias_cap, CON_MAX_BIAS);
    if (!logits || !t || !hist || !finished || !status || !cons || (bad_cap > 0 && !bad) || (bias_cap > 0 && (!bias_ids || !bias_val)))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if ((uintptr_t)cons % 32) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: cons must be 32-byte aligned", who);
    ConPerArgs a = {};
    a.logits = logits; a.ld = ld; a.V = V; a.max_new = max_new; a.n_slots = n_slots; a.t = t; a.hist = hist; a.finished = finished;
    a.status = status; a.row_map = row_map; a.cons = cons; a.bad = bad; a.bias_ids = bias_ids; a.bias_val = bias_val; a.bad_cap = bad_cap;
    a.bias_cap = bias_cap; a.eos = eos_id;
    DB1_DISPATCH_DT(dt, T, { constrain_logits_kernel<T, true, true><<<M, CON_THREADS, 0, (hipStream_t)stream>>>(a); });
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}
