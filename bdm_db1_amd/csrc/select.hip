// Next-token selection on the device (db1_select_tokens, include/db1_hip.h): greedy / temperature / top-k / top-p sampling over a vocabulary
// window, EOS bookkeeping and the hand-back of the chosen token into the next call's input ids -- so a generation loop is N graph replays with no
// host round trip in between.  The reference picks tokens with torch (logits.argmax(-1) and a host copy per token, evaluate_rl.py:157-266); its
// caption / VQA evaluation (train.py:146-170, text_decoder.py:42-62) keeps the tokens up to the first EOS.
//
// One workgroup of 1024 threads per row; the row lives in registers: thread `tid` owns the four consecutive columns 4 (j * 1024 + tid) + 0..3,
// j < NG (NG * 4096 >= V).  Every logit becomes an order-preserving uint32 key (0 = not a candidate: outside the window, NaN or +-inf), so
// max / arg-max are integer reductions (ties: lowest column) and the top-k / top-p thresholds are found by a bisection over the key range --
// no sort, no histogram atomics.  All reductions run in a fixed order (wave butterflies, then the 16 wave results read in order from LDS):
// the same inputs give the same bits.
#include "select_common.h"

#define SEL_THREADS 1024
#define SEL_WAVES (SEL_THREADS / 64)
#define SEL_MAX_NG 9                       // V <= 36 864 (DB1-1.3B: 33 025)
#define SEL_MAX_TOP 16                     // alternatives per token of the _top forms
#define SEL_SITE_SAMPLE 0xE0000100u        // Philox site of the sampling draws (dropout sites: layer * 4 + {0, 1, 2}, 0xE0000000, 0xE0000001)

typedef SelSharedT<SEL_WAVES> SelShared;

template <int NG>
__device__ __forceinline__ int sel_count_ge(const unsigned (&key)[NG][4], unsigned thr, SelShared& sh, int& ph) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < NG; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) c += (int)__popcll(__ballot(key[j][q] >= thr));
    return block_sum_i(c, sh, ph);
}
template <int NG>
__device__ __forceinline__ float sel_mass_ge(const unsigned (&key)[NG][4], const float (&e)[NG][4], unsigned thr, SelShared& sh, int& ph) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NG; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) s += key[j][q] >= thr ? e[j][q] : 0.f;
    return block_sum_f(s, sh, ph);
}

struct SelArgs {
    const void* logits;
    int64_t ld;
    int V, vlo, vhi;
    float inv_t;
    int top_k;
    float top_p;
    int greedy;
    unsigned k0, k1;
    int eos, pad, step_base, max_new;
    const int* t;
    const int* stream_id;
    int* t_slot;                // the slot form (db1_select_tokens_slots): per-slot counters (read and advanced), limits, the rows' slots
    const int* limit;
    const int* row_map;
    int n_slots;
    int* finished;
    int* lengths;
    int* out;
    long long* next_ids;
    int64_t ids_stride;
    int* status;
    float* logprob;             // the _lp forms (LP): [rows | n_slots, max_new] and [rows | n_slots]; NULL otherwise
    float* sum_logprob;
    int top_n;                  // the _top forms (TOP): [rows | n_slots, max_new, top_n] each; 0 and NULL otherwise
    int* top_ids;
    float* top_logprob;
    const int* params;          // the per-slot form (PER, db1_select_tokens_slots_per): [n_slots, 8], the record of include/db1_hip.h; NULL otherwise
    int q_in, Q;                // the verify form (SPEC, db1_spec_pick): positions per row in this launch, row stride of the four arrays below
    const long long* spec_ids;  // [rows, Q] the step's input ids (column i + 1: the draft for position i), READ only
    int* spec_sel;              // [rows, Q] the pick of every position (-1: no candidate, -2: skipped)
    int* spec_hit;              // [rows, Q] 1 where the next column's draft is the pick
    float* spec_lp;             // [rows, Q] the pick's log-probability (LP); NULL otherwise
};

// the unused entries [from, top_n) of one (row, t) of the _top buffers: -1 / -inf
__device__ __forceinline__ void sel_top_fill(const SelArgs& a, int64_t at, int from) {
    for (int i = from; i < a.top_n; i++) {
        a.top_ids[at * a.top_n + i] = -1;
        a.top_logprob[at * a.top_n + i] = -INFINITY;
    }
}

// SLOTS (db1_select_tokens_slots): logits row blockIdx.x belongs to slot `row` (row_map), which keeps its own counter t_slot[row] below
// limit[row]; a vacant slot (finished) only hands pad_id on; the selection itself is the same code.
// LP (db1_select_tokens_lp, db1_select_tokens_slots_lp): after the token is chosen, one more sweep over the keys forms the log-sum-exp of the
// row's candidates (the raw logits: no temperature, no top-k / top-p) and the owner of the row writes the token's log-probability next to it.
// TOP (db1_select_tokens_top, db1_select_tokens_slots_top; LP as well): after that, top_n rounds over the same keys (sel_top_rounds) give the
// row's best candidates in the arg-max's own order, and the owner of the row writes their columns and (l - max) - lz, the token's expression.
// PER (db1_select_tokens_slots_per; SLOTS only, with or without LP / TOP): the window, greedy, top-k, top-p, 1 / temperature and the seed are
// the slot's own, eight block-uniform words read from params[slot] once the slot is known to be live and its counter in range; a record no
// launch would have accepted as scalars closes the slot with status bit 2 the way a counter out of range closes it with bit 1.  The other
// instantiations take the same values from SelArgs and hold no trace of this mode.
// SPEC (db1_spec_pick; lockstep only, with or without LP): the verify launch of speculative decoding.  Workgroup blockIdx.x looks at
// position i = blockIdx.x % q_in of row blockIdx.x / q_in, i.e. at token index *t + i, and chooses exactly as the plain form chooses there
// (the code from the keys to `tok` is shared, the Philox step is step_base + *t + i); it keeps NO books: the owner thread writes the pick,
// whether the next column's draft equals it and (LP) its log-probability into [row, i] of the scratch arrays and nothing else, so that
// db1_spec_accept can derive the accepted count from those arrays alone.  The other instantiations hold no trace of this mode either.
template <typename T, int NG, bool SLOTS, bool LP, bool TOP, bool PER, bool SPEC>
__global__ __launch_bounds__(SEL_THREADS) void select_tokens_kernel(SelArgs a) {
    static_assert(SLOTS || !PER, "the per-slot parameters belong to the slot form");
    static_assert(!SPEC || (!SLOTS && !TOP), "the verify form is a lockstep form without alternatives");
    __shared__ SelShared sh;
    const int tid = threadIdx.x;
    int row = blockIdx.x, t;
    bool t_ok;
    int vlo = a.vlo, vhi = a.vhi, top_k = a.top_k, greedy = a.greedy;
    float inv_t = a.inv_t, top_p = a.top_p;
    unsigned k0 = a.k0, k1 = a.k1;
    if constexpr (SLOTS) {
        if (a.row_map) row = a.row_map[blockIdx.x];
        if (row < 0 || row >= a.n_slots) return;     // (a slot that does not exist: nothing to write to)
        if (a.finished[row]) {     // (block-uniform) vacant: out, t and lengths stay as they are
            if (tid == 0) a.next_ids[(int64_t)row * a.ids_stride] = a.pad;
            return;
        }
        t = a.t_slot[row];
        const int lim = a.limit[row];
        t_ok = t >= 0 && t < lim && lim <= a.max_new;
        if (!t_ok) {
            if (tid == 0) {
                a.status[row] |= 2;
                a.finished[row] = 1;
                a.next_ids[(int64_t)row * a.ids_stride] = a.pad;
            }
            return;
        }
        if constexpr (PER) {
            const int* p = a.params + (int64_t)row * 8;     // (every thread reads the same 32 bytes)
            greedy = p[0]; top_k = p[1]; vlo = p[2]; vhi = p[3];
            k0 = (unsigned)p[4]; k1 = (unsigned)p[5];
            inv_t = __int_as_float(p[6]); top_p = __int_as_float(p[7]);
            // what sel_launch refuses for the scalar forms (1 / temperature finite and positive <=> temperature is); a greedy slot's
            // words 1 and 4 .. 7 are never looked at
            const bool bad = !(vlo >= 0 && vlo < vhi && vhi <= a.V) ||
                             (!greedy && (!(inv_t > 0.f && inv_t < INFINITY) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f)));
            if (bad) {     // (block-uniform) out, t, lengths and the log-prob / top-n buffers stay as they are
                if (tid == 0) {
                    a.status[row] |= 4;
                    a.finished[row] = 1;
                    a.next_ids[(int64_t)row * a.ids_stride] = a.pad;
                }
                return;
            }
        }
    } else if constexpr (SPEC) {
        const int i = (int)(blockIdx.x % (unsigned)a.q_in);
        row = (int)(blockIdx.x / (unsigned)a.q_in);
        t = *a.t + i;
        t_ok = true;
        if (a.finished[row] || t < 0 || t >= a.max_new) {     // (block-uniform) nothing to verify here: SKIP
            if (tid == 0) {
                const int64_t at = (int64_t)row * a.Q + i;
                a.spec_sel[at] = -2;
                a.spec_hit[at] = 0;
                if constexpr (LP) a.spec_lp[at] = 0.f;
            }
            return;
        }
    } else {
        t = *a.t;
        t_ok = t >= 0 && t < a.max_new;
        if (a.finished[row]) {     // (block-uniform)
            if (tid == 0) {
                if (t_ok) {
                    a.out[(int64_t)row * a.max_new + t] = a.pad;
                    if constexpr (LP) a.logprob[(int64_t)row * a.max_new + t] = 0.f;
                    if constexpr (TOP) sel_top_fill(a, (int64_t)row * a.max_new + t, 0);
                } else a.status[row] |= 2;
                a.next_ids[(int64_t)row * a.ids_stride] = a.pad;
            }
            return;
        }
    }
    const T* lg = reinterpret_cast<const T*>(a.logits) + (int64_t)blockIdx.x * a.ld;
    const int lo = max(vlo, 0), hi = min(vhi, a.V);
    unsigned key[NG][4];
    unsigned long long best = 0;   // (key << 32) | ~column: max = largest key, lowest column on ties
    unsigned kmin = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < NG; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = 4 * (j * SEL_THREADS + tid) + q;
            const unsigned k = (c >= lo && c < hi) ? sel_key(ldf<T>(lg + c)) : 0u;
            key[j][q] = k;
            const unsigned long long p = ((unsigned long long)k << 32) | (unsigned)~c;
            best = (k && p > best) ? p : best;
            kmin = k ? min(kmin, k) : kmin;
        }
    int ph = 0;
    best = block_max_u64(best, sh, ph);
    int tok, bits = 0;
    const unsigned kmax = (unsigned)(best >> 32);
    if (kmax == 0) {                                  // nothing finite in the window
        tok = a.pad;
        bits = 1;
    } else if (greedy || top_k == 1) {
        tok = (int)~(unsigned)best;
    } else {
        // top-k: thr_k = the k-th largest key = the largest x with #{key >= x} >= k (bisection over [smallest key, largest key])
        // (bf16 logits: the low 16 bits of every key are 0, the bisection runs over the high 16)
        constexpr int S = sizeof(T) == 2 ? 16 : 0;
        unsigned thr = block_min_u32(kmin, sh, ph);
        if (top_k > 1) {
            unsigned l = thr >> S, h = kmax >> S;
            while (l < h) {
                const unsigned mid = l + ((h - l) >> 1) + ((h - l) & 1);
                if (sel_count_ge<NG>(key, mid << S, sh, ph) >= top_k) l = mid; else h = mid - 1;
            }
            thr = l << S;
        }
        // top-p: p = softmax(l / T) over {key >= thr_k}; thr_p = the largest key x with mass{key >= x} >= top_p (ties at x kept)
        if (top_p < 1.f) {
            const float m = sel_unkey(kmax);
            float e[NG][4];
            float z = 0.f;
#pragma unroll
            for (int j = 0; j < NG; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    e[j][q] = key[j][q] >= thr ? expf((sel_unkey(key[j][q]) - m) * inv_t) : 0.f;
                    z += e[j][q];
                }
            z = block_sum_f(z, sh, ph);
            const float target = top_p * z;
            unsigned l = thr >> S, h = kmax >> S;
            while (l < h) {
                const unsigned mid = l + ((h - l) >> 1) + ((h - l) & 1);
                if (sel_mass_ge<NG>(key, e, mid << S, sh, ph) >= target) l = mid; else h = mid - 1;
            }
            thr = l << S;
        }
        // Gumbel-max over the kept set: argmax l / T - log(-log u), u from Philox (column / 4, stream id, step, SITE_SAMPLE; seed)
        const unsigned sid = a.stream_id ? (unsigned)a.stream_id[row] : (unsigned)row;
        const unsigned step = (unsigned)(a.step_base + t);
        unsigned long long sb = 0;
#pragma unroll
        for (int j = 0; j < NG; j++) {
            const bool any = key[j][0] >= thr || key[j][1] >= thr || key[j][2] >= thr || key[j][3] >= thr;
            if (any) {
                const int g = j * SEL_THREADS + tid;
                unsigned o[4];
                db1_philox4x32_10((unsigned)g, sid, step, SEL_SITE_SAMPLE, k0, k1, o);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (key[j][q] < thr) continue;
                    const float u = ((float)(o[q] >> 8) + 0.5f) * 5.9604644775390625e-8f;   // ((x >> 8) + 0.5) * 2^-24: exact in fp32
                    const float s = sel_unkey(key[j][q]) * inv_t - logf(-logf(u));
                    const unsigned sk = sel_key(s);
                    const unsigned long long p = ((unsigned long long)sk << 32) | (unsigned)~(4 * g + q);
                    sb = p > sb ? p : sb;
                }
            }
        }
        sb = block_max_u64(sb, sh, ph);
        tok = (unsigned)(sb >> 32) ? (int)~(unsigned)sb : (int)~(unsigned)best;   // (a non-finite score cannot win: fall back to the arg-max)
    }
    // LP: lp = (l[tok] - max) - log(sum exp(l - max)) over the candidates (key != 0), the sum in the fixed order of every reduction here.  The e
    // of the top-p branch is exp((l - max) / T) over the top-k set: another quantity, dead by now.
    float lz = 0.f;
    if constexpr (LP) {
        if (kmax != 0 && t_ok) {                      // (block-uniform)
            const float m = sel_unkey(kmax);
            float z = 0.f;
#pragma unroll
            for (int j = 0; j < NG; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) z += key[j][q] ? expf(sel_unkey(key[j][q]) - m) : 0.f;
            lz = logf(block_sum_f(z, sh, ph));
        }
    }
    if constexpr (TOP) {
        if (t_ok) {                                   // (block-uniform)
            const int64_t at = (int64_t)row * a.max_new + t;
            const float m = sel_unkey(kmax);
            auto scan = [&](unsigned long long below) {
                const unsigned wk = (unsigned)(below >> 32);
                const int d = (int)~(unsigned)below - 4 * tid;
                const int z = sel_opaque_zero();
                unsigned bk = 0;
                int bo = 0;
#pragma unroll
                for (int j = 0; j < NG; j++)
#pragma unroll
                    for (int q = 0; q < 4; q++) sel_scan_step(key[j][q], z + (4 * j * SEL_THREADS + q), wk, d, bk, bo);
                return sel_pair(bk, 4 * tid + bo);
            };
            auto emit = [&](int i, unsigned long long w, bool) {
                if (tid == 0) {
                    a.top_ids[at * a.top_n + i] = (int)~(unsigned)w;
                    a.top_logprob[at * a.top_n + i] = (sel_unkey((unsigned)(w >> 32)) - m) - lz;   // (the key gives the logit back bit for bit)
                }
            };
            const int got = kmax ? sel_top_rounds(a.top_n, best, scan, emit, sh, ph) : 0;
            if (tid == 0) sel_top_fill(a, at, got);
        }
    }
    if constexpr (SPEC) {
        if (tid == 0) {
            const int i = (int)(blockIdx.x % (unsigned)a.q_in);
            const int64_t at = (int64_t)row * a.Q + i;
            const int s = (bits & 1) ? -1 : tok;
            a.spec_sel[at] = s;
            a.spec_hit[at] = (i + 1 < a.q_in && a.spec_ids[at + 1] == (long long)s) ? 1 : 0;
            if constexpr (LP) a.spec_lp[at] = kmax != 0 ? (ldf<T>(lg + tok) - sel_unkey(kmax)) - lz : 0.f;
        }
        return;
    }
    if (tid == 0) {
        int fin = 0;
        if (bits & 1) fin = 1;
        else if (tok == a.eos) fin = 1;
        else a.lengths[row] += 1;
        if constexpr (SLOTS) {      // this workgroup owns the slot: it advances the slot's counter itself and closes the slot at its limit
            a.t_slot[row] = t + 1;
            if (t + 1 == a.limit[row]) fin = 1;
        }
        if (fin) a.finished[row] = 1;
        if (t_ok) {
            a.out[(int64_t)row * a.max_new + t] = tok;
            if constexpr (LP) {
                float lp = 0.f;
                if (kmax != 0) {                      // (a row without a candidate: 0, and the sum stays)
                    lp = (ldf<T>(lg + tok) - sel_unkey(kmax)) - lz;
                    a.sum_logprob[row] += lp;
                }
                a.logprob[(int64_t)row * a.max_new + t] = lp;
            }
        } else bits |= 2;
        if (bits) a.status[row] |= bits;
        a.next_ids[(int64_t)row * a.ids_stride] = tok;
    }
}

static int sel_ng(int V) { return V <= 4096 ? 1 : (V <= 3 * 4096 ? 3 : (V <= SEL_MAX_NG * 4096 ? SEL_MAX_NG : 0)); }

extern "C" int db1_select_tokens_supported(int V, int64_t ld, int dt) {
    return db1_dt_ok(dt) && V > 0 && ld >= V && sel_ng(V) > 0;
}

extern "C" int64_t db1_select_tokens_workspace_bytes(int M, int V, int dt) {
    (void)M; (void)V; (void)dt;
    return 0;
}

template <typename T, bool SLOTS, bool LP, bool TOP, bool PER = false, bool SPEC = false>
static void sel_dispatch(int ng, const SelArgs& a, int M, hipStream_t st) {
    if (ng == 1) select_tokens_kernel<T, 1, SLOTS, LP, TOP, PER, SPEC><<<M, SEL_THREADS, 0, st>>>(a);
    else if (ng == 3) select_tokens_kernel<T, 3, SLOTS, LP, TOP, PER, SPEC><<<M, SEL_THREADS, 0, st>>>(a);
    else select_tokens_kernel<T, SEL_MAX_NG, SLOTS, LP, TOP, PER, SPEC><<<M, SEL_THREADS, 0, st>>>(a);
}

// The host side both entry points share: `a` arrives filled; validation (in one order for both, so an argument list that is wrong in two ways
// fails with the same code as ever), 1 / temperature, the NG / SLOTS / LP dispatch over M workgroups, the launch check.  `lp`: the _lp
// forms, which need both log-prob buffers; the others leave them NULL and launch the instantiations without that code.  `top`: the _top
// forms (lp as well), which need 1 <= top_n <= SEL_MAX_TOP and both of their buffers; a.top_n == 0 otherwise.  `per`: the per-slot form
// (slots as well): a.params, non-NULL and 32-byte aligned, stands in for the window, the temperature, top-k / top-p and the seed, which the
// kernel checks slot by slot (device data cannot be checked here).
static int sel_launch(const char* who, bool slots, bool lp, bool top, bool per, SelArgs& a, int M, int dt, float temperature, void* stream) {
    if (!db1_dt_ok(dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dt);
    if (M <= 0 || M > 65535 || a.V <= 0 || a.ld < a.V || a.max_new <= 0 || a.ids_stride < 0 || a.n_slots <= 0 || (!a.row_map && a.n_slots != M))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d V=%d ld=%lld max_new=%d ids_stride=%lld n_slots=%d%s", who, M, a.V, (long long)a.ld, a.max_new,
                 (long long)a.ids_stride, a.n_slots, slots && !a.row_map ? " (no row_map: n_slots must equal M)" : "");
    if (top && (a.top_n < 1 || a.top_n > SEL_MAX_TOP)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_n %d (1 .. %d)", who, a.top_n, SEL_MAX_TOP);
    const int ng = sel_ng(a.V);
    if (!ng) DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: V=%d (at most %d)", who, a.V, SEL_MAX_NG * 4096);
    if (!a.logits || !(slots ? a.t_slot && a.limit : a.t != nullptr) || !a.finished || !a.lengths || !a.out || !a.next_ids || !a.status ||
        (lp && (!a.logprob || !a.sum_logprob)) || (top && (!a.top_ids || !a.top_logprob)) || (per && !a.params))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (per) {
        if (reinterpret_cast<uintptr_t>(a.params) % 32) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: params %p is not 32-byte aligned", who, (const void*)a.params);
    } else {
        if (a.vlo < 0 || a.vhi > a.V || a.vlo >= a.vhi)
            DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: window [%d, %d) is empty or outside [0, %d)", who, a.vlo, a.vhi, a.V);
        if (!a.greedy && !(temperature > 0.f && temperature < INFINITY))
            DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: temperature %g", who, (double)temperature);
        if (!a.greedy && (a.top_k < 0 || !(a.top_p > 0.f && a.top_p <= 1.f)))
            DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_k %d top_p %g", who, a.top_k, (double)a.top_p);
        a.inv_t = a.greedy ? 1.f : 1.f / temperature;
    }
    hipStream_t st = (hipStream_t)stream;
    DB1_DISPATCH_DT(dt, T, {
        if (per) {
            if (top) sel_dispatch<T, true, true, true, true>(ng, a, M, st);
            else if (lp) sel_dispatch<T, true, true, false, true>(ng, a, M, st);
            else sel_dispatch<T, true, false, false, true>(ng, a, M, st);
        } else if (slots) {
            if (top) sel_dispatch<T, true, true, true>(ng, a, M, st);
            else if (lp) sel_dispatch<T, true, true, false>(ng, a, M, st);
            else sel_dispatch<T, true, false, false>(ng, a, M, st);
        } else {
            if (top) sel_dispatch<T, false, true, true>(ng, a, M, st);
            else if (lp) sel_dispatch<T, false, true, false>(ng, a, M, st);
            else sel_dispatch<T, false, false, false>(ng, a, M, st);
        }
    });
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}

// every field but inv_t (sel_launch) and the counters (t | t_slot, limit, row_map, n_slots: the entry points)
static SelArgs sel_args(const void* logits, int V, int64_t ld, int vocab_lo, int vocab_hi, int top_k, float top_p, int greedy, uint32_t seed_lo,
                        uint32_t seed_hi, int eos_id, int pad_id, int step_base, const int32_t* stream_id, int32_t* finished, int32_t* lengths,
                        int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride, int32_t* status) {
    SelArgs a = {};
    a.logits = logits; a.ld = ld; a.V = V; a.vlo = vocab_lo; a.vhi = vocab_hi;
    a.top_k = top_k; a.top_p = top_p; a.greedy = greedy;
    a.k0 = seed_lo; a.k1 = seed_hi; a.eos = eos_id; a.pad = pad_id; a.step_base = step_base; a.max_new = max_new;
    a.stream_id = stream_id; a.finished = finished; a.lengths = lengths; a.out = out;
    a.next_ids = reinterpret_cast<long long*>(next_ids); a.ids_stride = ids_stride; a.status = status;
    return a;
}

// db1_select_tokens (logprob == NULL), db1_select_tokens_lp (top_ids == NULL, top_n 0) and db1_select_tokens_top
static int sel_tokens(const char* who, bool lp, bool top, const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature,
                      int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base,
                      const int32_t* t, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                      int64_t* next_ids, int64_t ids_stride, int32_t* status, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids,
                      float* top_logprob, void* stream) {
    SelArgs a = sel_args(logits, V, ld, vocab_lo, vocab_hi, top_k, top_p, greedy, seed_lo, seed_hi, eos_id, pad_id, step_base, stream_id, finished,
                         lengths, out, max_new, next_ids, ids_stride, status);
    a.t = t; a.n_slots = M; a.logprob = logprob; a.sum_logprob = sum_logprob;
    a.top_n = top_n; a.top_ids = top_ids; a.top_logprob = top_logprob;
    return sel_launch(who, false, lp, top, false, a, M, dt, temperature, stream);
}

extern "C" int db1_select_tokens(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                                 float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base,
                                 const int32_t* t, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                                 int64_t* next_ids, int64_t ids_stride, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    return sel_tokens("select_tokens", false, false, logits, M, V, ld, dt, vocab_lo, vocab_hi, temperature, top_k, top_p, greedy, seed_lo, seed_hi, eos_id,
                      pad_id, step_base, t, stream_id, finished, lengths, out, max_new, next_ids, ids_stride, status, nullptr, nullptr, 0, nullptr,
                      nullptr, stream);
}

extern "C" int db1_select_tokens_lp(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                                    float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base,
                                    const int32_t* t, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                                    int64_t* next_ids, int64_t ids_stride, int32_t* status, float* logprob, float* sum_logprob, void* ws,
                                    int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    return sel_tokens("select_tokens_lp", true, false, logits, M, V, ld, dt, vocab_lo, vocab_hi, temperature, top_k, top_p, greedy, seed_lo,
                      seed_hi, eos_id, pad_id, step_base, t, stream_id, finished, lengths, out, max_new, next_ids, ids_stride, status, logprob,
                      sum_logprob, 0, nullptr, nullptr, stream);
}

extern "C" int db1_select_tokens_top(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature, int top_k,
                                     float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base,
                                     const int32_t* t, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                                     int64_t* next_ids, int64_t ids_stride, int32_t* status, float* logprob, float* sum_logprob, int top_n,
                                     int32_t* top_ids, float* top_logprob, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    return sel_tokens("select_tokens_top", true, true, logits, M, V, ld, dt, vocab_lo, vocab_hi, temperature, top_k, top_p, greedy, seed_lo,
                      seed_hi, eos_id, pad_id, step_base, t, stream_id, finished, lengths, out, max_new, next_ids, ids_stride, status, logprob,
                      sum_logprob, top_n, top_ids, top_logprob, stream);
}

// ------------------------------------------------------------------ the slot form (continuous batching, serving.py)
extern "C" int db1_select_tokens_slots_supported(int V, int64_t ld, int dt) { return db1_select_tokens_supported(V, ld, dt); }

extern "C" int64_t db1_select_tokens_slots_workspace_bytes(int M, int V, int dt) {
    (void)M; (void)V; (void)dt;
    return 0;
}

// db1_select_tokens_slots (logprob == NULL), db1_select_tokens_slots_lp (top_ids == NULL, top_n 0) and db1_select_tokens_slots_top
static int sel_slots(const char* who, bool lp, bool top, const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature,
                     int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id, int step_base, int32_t* t,
                     const int32_t* limit, const int32_t* stream_id, int32_t* finished, int32_t* lengths, int32_t* out, int max_new,
                     int64_t* next_ids, int64_t ids_stride, int32_t* status, const int32_t* row_map, int n_slots, float* logprob,
                     float* sum_logprob, int top_n, int32_t* top_ids, float* top_logprob, void* stream) {
    SelArgs a = sel_args(logits, V, ld, vocab_lo, vocab_hi, top_k, top_p, greedy, seed_lo, seed_hi, eos_id, pad_id, step_base, stream_id, finished,
                         lengths, out, max_new, next_ids, ids_stride, status);
    a.t_slot = t; a.limit = limit; a.row_map = row_map; a.n_slots = n_slots; a.logprob = logprob; a.sum_logprob = sum_logprob;
    a.top_n = top_n; a.top_ids = top_ids; a.top_logprob = top_logprob;
    return sel_launch(who, true, lp, top, false, a, M, dt, temperature, stream);
}

extern "C" int db1_select_tokens_slots(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature,
                                       int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id,
                                       int step_base, int32_t* t, const int32_t* limit, const int32_t* stream_id, int32_t* finished,
                                       int32_t* lengths, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride, int32_t* status,
                                       const int32_t* row_map, int n_slots, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    return sel_slots("select_tokens_slots", false, false, logits, M, V, ld, dt, vocab_lo, vocab_hi, temperature, top_k, top_p, greedy, seed_lo, seed_hi,
                     eos_id, pad_id, step_base, t, limit, stream_id, finished, lengths, out, max_new, next_ids, ids_stride, status, row_map, n_slots,
                     nullptr, nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int db1_select_tokens_slots_lp(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature,
                                          int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id,
                                          int step_base, int32_t* t, const int32_t* limit, const int32_t* stream_id, int32_t* finished,
                                          int32_t* lengths, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride, int32_t* status,
                                          const int32_t* row_map, int n_slots, float* logprob, float* sum_logprob, void* ws, int64_t ws_bytes,
                                          void* stream) {
    (void)ws; (void)ws_bytes;
    return sel_slots("select_tokens_slots_lp", true, false, logits, M, V, ld, dt, vocab_lo, vocab_hi, temperature, top_k, top_p, greedy, seed_lo,
                     seed_hi, eos_id, pad_id, step_base, t, limit, stream_id, finished, lengths, out, max_new, next_ids, ids_stride, status, row_map,
                     n_slots, logprob, sum_logprob, 0, nullptr, nullptr, stream);
}

extern "C" int db1_select_tokens_slots_top(const void* logits, int M, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature,
                                           int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int eos_id, int pad_id,
                                           int step_base, int32_t* t, const int32_t* limit, const int32_t* stream_id, int32_t* finished,
                                           int32_t* lengths, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride, int32_t* status,
                                           const int32_t* row_map, int n_slots, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids,
                                           float* top_logprob, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    return sel_slots("select_tokens_slots_top", true, true, logits, M, V, ld, dt, vocab_lo, vocab_hi, temperature, top_k, top_p, greedy, seed_lo,
                     seed_hi, eos_id, pad_id, step_base, t, limit, stream_id, finished, lengths, out, max_new, next_ids, ids_stride, status, row_map,
                     n_slots, logprob, sum_logprob, top_n, top_ids, top_logprob, stream);
}

// The per-slot form: db1_select_tokens_slots[_lp|_top] with the window, greedy, temperature, top-k, top-p and the seed read per slot from
// params [n_slots, 8] (include/db1_hip.h).  ONE entry point: the log-prob and top-n arguments say which instantiation runs -- none of them
// (plain), both log-prob buffers (LP), those and top_n with both top-n buffers (TOP); any other combination fails sel_launch's own checks.
extern "C" int db1_select_tokens_slots_per(const void* logits, int M, int V, int64_t ld, int dt, const int32_t* params, int eos_id, int pad_id,
                                           int step_base, int32_t* t, const int32_t* limit, const int32_t* stream_id, int32_t* finished,
                                           int32_t* lengths, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride, int32_t* status,
                                           const int32_t* row_map, int n_slots, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids,
                                           float* top_logprob, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    const bool top = top_n != 0 || top_ids || top_logprob, lp = top || logprob || sum_logprob;
    SelArgs a = sel_args(logits, V, ld, 0, V, 0, 1.f, 1, 0, 0, eos_id, pad_id, step_base, stream_id, finished, lengths, out, max_new, next_ids,
                         ids_stride, status);
    a.t_slot = t; a.limit = limit; a.row_map = row_map; a.n_slots = n_slots; a.logprob = logprob; a.sum_logprob = sum_logprob;
    a.top_n = top_n; a.top_ids = top_ids; a.top_logprob = top_logprob; a.params = params;
    return sel_launch("select_tokens_slots_per", true, lp, top, true, a, M, dt, 1.f, stream);
}

// ------------------------------------------------------------------ the verify form (speculative decoding, generation.py; csrc/spec.hip)
#define SPEC_MAX_Q 16

extern "C" int db1_spec_pick_supported(int V, int64_t ld, int dt, int Q) {
    return db1_select_tokens_supported(V, ld, dt) && Q >= 2 && Q <= SPEC_MAX_Q;
}

// db1_spec_pick: the SPEC instantiations over M * q_in workgroups (lp == NULL: without the log-prob sweep).  Its refusals are sel_launch's,
// in sel_launch's order and with its codes, for the arguments the two share; nothing is launched after one.
extern "C" int db1_spec_pick(const void* logits, int M, int q_in, int Q, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, float temperature,
                             int top_k, float top_p, int greedy, uint32_t seed_lo, uint32_t seed_hi, int pad_id, int step_base, const int32_t* t,
                             const int32_t* stream_id, const int32_t* finished, int max_new, const int64_t* ids, int32_t* sel, int32_t* hit,
                             float* lp, void* stream) {
    const char* who = "spec_pick";
    if (!db1_dt_ok(dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dt);
    if (M <= 0 || Q < 2 || Q > SPEC_MAX_Q || q_in < 1 || q_in > Q || (int64_t)M * Q > 65535 || V <= 0 || ld < V || max_new <= 0)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d q_in=%d Q=%d V=%d ld=%lld max_new=%d (1 <= q_in <= Q, 2 <= Q <= %d, M * Q <= 65535)", who, M, q_in, Q, V,
                 (long long)ld, max_new, SPEC_MAX_Q);
    const int ng = sel_ng(V);
    if (!ng) DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: V=%d (at most %d)", who, V, SEL_MAX_NG * 4096);
    if (!logits || !t || !finished || !ids || !sel || !hit) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (vocab_lo < 0 || vocab_hi > V || vocab_lo >= vocab_hi)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: window [%d, %d) is empty or outside [0, %d)", who, vocab_lo, vocab_hi, V);
    if (!greedy && !(temperature > 0.f && temperature < INFINITY)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: temperature %g", who, (double)temperature);
    if (!greedy && (top_k < 0 || !(top_p > 0.f && top_p <= 1.f))) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_k %d top_p %g", who, top_k, (double)top_p);
    SelArgs a = sel_args(logits, V, ld, vocab_lo, vocab_hi, top_k, top_p, greedy, seed_lo, seed_hi, -1, pad_id, step_base, stream_id,
                         const_cast<int32_t*>(finished), nullptr, nullptr, max_new, nullptr, 0, nullptr);     // (the SPEC code only reads finished)
    a.inv_t = greedy ? 1.f : 1.f / temperature;
    a.t = t; a.n_slots = M; a.q_in = q_in; a.Q = Q;
    a.spec_ids = reinterpret_cast<const long long*>(ids); a.spec_sel = sel; a.spec_hit = hit; a.spec_lp = lp;
    hipStream_t st = (hipStream_t)stream;
    DB1_DISPATCH_DT(dt, T, {
        if (lp) sel_dispatch<T, false, true, false, false, true>(ng, a, M * q_in, st);
        else sel_dispatch<T, false, false, false, false, true>(ng, a, M * q_in, st);
    });
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}
