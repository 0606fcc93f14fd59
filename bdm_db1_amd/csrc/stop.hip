// Stop sequences on the device (db1_stop_match, include/db1_hip.h; tests/stop_rule.py restates the rule in NumPy): after the selection has
// written a row's token, the row's output is compared with up to 16 token sequences of up to 16 tokens each; a row whose last tokens spell
// one of them loses those tokens (pad_id), ends (finished = 1) and feeds pad_id forward, and its log-prob sum is rebuilt over what is kept.
//
// One wave of 64 threads per logits row, no LDS.  ``lengths[slot] != checked[slot]`` says that the selection has just added a token (it grows
// ``lengths`` exactly then), so vacant slots, rows that finished earlier and rows that just wrote EOS cost two loads.  Lane k compares
// sequence k with the row's tail (at most 16 dependent-free loads of each); one butterfly maximum over (length, 63 - k) names the longest
// match, the lowest k among equals, in every lane; the lanes then clear the matched range (at most 16 tokens, 16 x 16 alternatives) and lane 0
// writes the row's scalars and re-adds the kept log-probs one by one from 0.0f: the order, and so the bits, of the selection's own running
// sum.  A workgroup owns its slot (row_map entries are distinct): no atomics, no workspace; every argument is a pointer or a launch scalar
// and nothing is read back: the launch can be captured and replayed.
//
// db1_stop_match_per (tests/slot_constraints_rule.py) is the PER instantiation: every slot has its own list, stop_tok [n_slots, 16, 16] and
// stop_len [n_slots, 16], and all 16 lanes look (an unused entry has length 0, which matches nothing).  Nothing else differs.
#include "db1_common.h"

#define STOP_THREADS 64
#define STOP_MAX_SEQ 16
#define STOP_MAX_LEN 16

struct StopArgs {
    const int* stop_tok;
    const int* stop_len;
    int n_stop, pad_id, max_new, n_slots, top_n;
    int* lengths;
    int* checked;
    int* finished;
    int* stop_hit;
    int* out;
    int64_t* next_ids;
    int64_t ids_stride;
    const int* row_map;
    float* logprob;
    float* sum_logprob;
    int* top_ids;
    float* top_logprob;
};

template <bool PER>
__global__ __launch_bounds__(STOP_THREADS) void stop_match_kernel(StopArgs a) {
    const int lane = threadIdx.x;
    const int s = a.row_map ? a.row_map[blockIdx.x] : (int)blockIdx.x;
    if (s < 0 || s >= a.n_slots) return;
    const int n = a.lengths[s];
    if (n == a.checked[s]) return;                       // no new token since the last look: nothing of the slot is touched
    if (lane == 0) a.checked[s] = n;
    if (n < 1 || n > a.max_new) return;
    int* o = a.out + (int64_t)s * a.max_new;
    // lane k: does sequence k end the row?  (a length outside 1 .. 16 in the device list matches nothing: nothing is read through it)
    int key = 0;
    if (lane < (PER ? STOP_MAX_SEQ : a.n_stop)) {
        const int e = PER ? s * STOP_MAX_SEQ + lane : lane;      // (PER: the slot's own list)
        const int len = a.stop_len[e];
        if (len >= 1 && len <= STOP_MAX_LEN && len <= n) {
            const int* q = a.stop_tok + e * STOP_MAX_LEN;
            bool same = true;
            for (int j = 0; j < len; j++) same = same && o[n - len + j] == q[j];
            if (same) key = (len << 6) | (63 - lane);    // longest first, then the lowest k
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off, STOP_THREADS));
    if (key == 0) return;
    const int L = key >> 6, k = 63 - (key & 63), m = n - L;
    const int64_t row = (int64_t)s * a.max_new;
    if (lane < L) {
        o[m + lane] = a.pad_id;
        if (a.logprob) a.logprob[row + m + lane] = 0.f;
    }
    if (a.top_ids) {
        const int64_t base = (row + m) * a.top_n;
        for (int e = lane; e < L * a.top_n; e += STOP_THREADS) {
            a.top_ids[base + e] = -1;
            a.top_logprob[base + e] = -INFINITY;
        }
    }
    if (lane == 0) {
        a.lengths[s] = m;
        a.checked[s] = m;
        a.finished[s] = 1;
        a.stop_hit[s] = k + 1;
        a.next_ids[(int64_t)s * a.ids_stride] = a.pad_id;
        if (a.logprob) {
            float sum = 0.f;
            for (int j = 0; j < m; j++) sum += a.logprob[row + j];
            a.sum_logprob[s] = sum;
        }
    }
}

extern "C" int db1_stop_match_supported(int n_stop, int max_new) {
    return n_stop >= 1 && n_stop <= STOP_MAX_SEQ && max_new >= 1;
}

extern "C" int db1_stop_match(const int32_t* stop_tok, const int32_t* stop_len, int n_stop, int pad_id, int32_t* lengths, int32_t* checked,
                              int32_t* finished, int32_t* stop_hit, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride,
                              const int32_t* row_map, int M, int n_slots, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids,
                              float* top_logprob, void* stream) {
    const char* who = "stop_match";
    if (M <= 0 || M > 65535 || n_slots <= 0 || max_new <= 0 || n_stop <= 0 || (!row_map && n_slots != M))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d n_slots=%d max_new=%d n_stop=%d%s", who, M, n_slots, max_new, n_stop,
                 !row_map ? " (no row_map: n_slots must equal M)" : "");
    if (!db1_stop_match_supported(n_stop, max_new)) DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: n_stop=%d (at most %d)", who, n_stop, STOP_MAX_SEQ);
    if (!stop_tok || !stop_len || !lengths || !checked || !finished || !stop_hit || !out || !next_ids)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if ((logprob == nullptr) != (sum_logprob == nullptr)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: logprob and sum_logprob go together", who);
    const bool top = top_n != 0 || top_ids || top_logprob;
    if (top && (top_n < 1 || top_n > 16 || !top_ids || !top_logprob || !logprob))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_n=%d needs 1 <= top_n <= 16, top_ids, top_logprob and the log-prob buffers", who, top_n);
    StopArgs a = {};
    a.stop_tok = stop_tok; a.stop_len = stop_len; a.n_stop = n_stop; a.pad_id = pad_id; a.max_new = max_new; a.n_slots = n_slots; a.top_n = top_n;
    a.lengths = lengths; a.checked = checked; a.finished = finished; a.stop_hit = stop_hit; a.out = out; a.next_ids = next_ids;
    a.ids_stride = ids_stride; a.row_map = row_map; a.logprob = logprob; a.sum_logprob = sum_logprob; a.top_ids = top_ids;
    a.top_logprob = top_logprob;
    stop_match_kernel<false><<<M, STOP_THREADS, 0, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}

extern "C" int db1_stop_match_per(const int32_t* stop_tok, const int32_t* stop_len, int pad_id, int32_t* lengths, int32_t* checked,
                                  int32_t* finished, int32_t* stop_hit, int32_t* out, int max_new, int64_t* next_ids, int64_t ids_stride,
                                  const int32_t* row_map, int M, int n_slots, float* logprob, float* sum_logprob, int top_n, int32_t* top_ids,
                                  float* top_logprob, void* stream) {
    const char* who = "stop_match_per";
    if (M <= 0 || M > 65535 || n_slots <= 0 || max_new <= 0 || (!row_map && n_slots != M))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: M=%d n_slots=%d max_new=%d%s", who, M, n_slots, max_new,
                 !row_map ? " (no row_map: n_slots must equal M)" : "");
    if (!stop_tok || !stop_len || !lengths || !checked || !finished || !stop_hit || !out || !next_ids)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if ((logprob == nullptr) != (sum_logprob == nullptr)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: logprob and sum_logprob go together", who);
    const bool top = top_n != 0 || top_ids || top_logprob;
    if (top && (top_n < 1 || top_n > 16 || !top_ids || !top_logprob || !logprob))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_n=%d needs 1 <= top_n <= 16, top_ids, top_logprob and the log-prob buffers", who, top_n);
    StopArgs a = {};
    a.stop_tok = stop_tok; a.stop_len = stop_len; a.n_stop = STOP_MAX_SEQ; a.pad_id = pad_id; a.max_new = max_new; a.n_slots = n_slots;
    a.top_n = top_n; a.lengths = lengths; a.checked = checked; a.finished = finished; a.stop_hit = stop_hit; a.out = out; a.next_ids = next_ids;
    a.ids_stride = ids_stride; a.row_map = row_map; a.logprob = logprob; a.sum_logprob = sum_logprob; a.top_ids = top_ids;
    a.top_logprob = top_logprob;
    stop_match_kernel<true><<<M, STOP_THREADS, 0, (hipStream_t)stream>>>(a);
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}
