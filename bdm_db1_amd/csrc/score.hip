// Scoring given text (db1_score_rows / db1_lmhead_score / db1_score_segments, include/db1_hip.h): the log-probability, arg-max and rank of a
// label under every row of logits, over a vocabulary window.  The reference has no such path: its validation prints one mean loss and leaves
// the per-task `sub_loss` dictionary empty (train.py:86-138).
//
// db1_score_rows: one workgroup per row, the row lives in registers as loaded (16 bytes per piece, like ce_fwd_bwd_kernel in
// elementwise.hip): thread `tid` owns the pieces (k * NT + tid) * VN + 0..VN-1, k < SC_NP.  Pass 1 over the registers: the maximum of the
// candidates (finite, inside the window; everything else reads as -inf).  Pass 2: sum-exp, the count of candidates above the label's logit
// and the lowest column that holds the maximum.  Three reductions share one barrier; every reduction runs in a fixed order (wave butterfly,
// then the wave results read in order from LDS): the same inputs give the same bits.  Nothing is written to the logits.
//
// db1_score_rows_top (TOP, an instantiation of its own): after pass 2 every thread holds lse, and top_n rounds over the same registers
// (sel_top_rounds, select_common.h) give the row's best candidates, logit descending, ties by the lower column; the thread that holds a
// round's winner writes its column and x - lse, the expression of logprob.  The rounds rank -0.0 and +0.0 as one value, as the float
// comparisons of top1 and rank do.
#include "select_common.h"

#define SC_NP 17                            // 16-byte pieces per thread: 256 x 8 x 17 = 34 816 bf16, 512 x 4 x 17 = 34 816 fp32 elements
#define SC_MAX_ROW (256 * 8 * SC_NP)
#define SC_MAX_TOP 16                       // alternatives per row of db1_score_rows_top

__device__ __forceinline__ bool sc_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

struct ScoreArgs {
    const void* logits;
    const int64_t* labels;
    float* lse;
    float* logprob;
    int* top1;
    int* rank;
    int* status;
    int64_t ld;
    int V, lo, hi;
    int top_n;                  // db1_score_rows_top (TOP): [T, top_n] each; 0 and NULL otherwise
    int* top_ids;
    float* top_logprob;
};

// (TOP: held to the 4 waves per SIMD of the plain form)
template <typename T, int NT, bool TOP>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(TOP ? 4 : 1))) void score_rows_kernel(ScoreArgs a) {
    constexpr int VN = Vec16<T>::N, NW = NT / 64;
    __shared__ float sh_m[NW];
    __shared__ float sh_s[NW];
    __shared__ int sh_c[NW];
    __shared__ unsigned sh_a[NW];
    const int64_t t = blockIdx.x;
    const T* row = reinterpret_cast<const T*>(a.logits) + t * a.ld;
    const int tid = threadIdx.x, ld = (int)a.ld, lo = a.lo, hi = a.hi;
    const int64_t yl = a.labels[t];
    const bool y_in = yl >= 0 && yl < a.V;
    const int y = y_in ? (int)yl : 0;
    uint4 raw[SC_NP];
#pragma unroll
    for (int k = 0; k < SC_NP; k++) {   // (unconditional, at a clamped address: loads inside a branch are waited for one by one)
        const int c = (k * NT + tid) * VN;
        raw[k] = *reinterpret_cast<const uint4*>(row + (c < ld ? c : ld - VN));
    }
    const float ly_raw = ldf<T>(row + y);
    const bool y_cand = y_in && y >= lo && y < hi && sc_finite(ly_raw);
    // the VN values of piece k with everything that is not a candidate replaced by -inf
    auto unpack = [&](int k, int c, float (&x)[VN]) {
        Vec16<T> v;
        v.load(reinterpret_cast<const T*>(&raw[k]));
        const bool inside = c >= lo && c + VN <= hi;
#pragma unroll
        for (int j = 0; j < VN; j++) {
            const bool ok = sc_finite(v.v[j]) && (inside || (c + j >= lo && c + j < hi));
            x[j] = ok ? v.v[j] : -INFINITY;
        }
    };
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < SC_NP; k++) {
        const int c = (k * NT + tid) * VN;
        if (c < hi && c + VN > lo) {
            float x[VN];
            unpack(k, c, x);
#pragma unroll
            for (int j = 0; j < VN; j++) m = fmaxf(m, x[j]);
        }
    }
    m = wave_max(m);
    if ((tid & 63) == 0) sh_m[tid >> 6] = m;
    __syncthreads();
    float M = sh_m[0];
#pragma unroll
    for (int w = 1; w < NW; w++) M = fmaxf(M, sh_m[w]);
    if (M == -INFINITY) {     // (block-uniform) no candidate in the window
        if (tid == 0) {
            a.lse[t] = -INFINITY;
            a.top1[t] = -1;
            a.rank[t] = -1;
            a.logprob[t] = y_in ? -INFINITY : 0.f;
            a.status[t] = 2 | (y_in ? 1 : 0);
            if constexpr (TOP)
                for (int i = 0; i < a.top_n; i++) {
                    a.top_ids[t * a.top_n + i] = -1;
                    a.top_logprob[t * a.top_n + i] = -INFINITY;
                }
        }
        return;
    }
    const float ly = y_cand ? ly_raw : INFINITY;   // (nothing is above +inf: the count of a label that is no candidate is not used)
    float s = 0.f;
    int cnt = 0;
    unsigned arg = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < SC_NP; k++) {
        const int c = (k * NT + tid) * VN;
        if (c < hi && c + VN > lo) {
            float x[VN];
            unpack(k, c, x);
#pragma unroll
            for (int j = 0; j < VN; j++) {
                s += __expf(x[j] - M);                       // (-inf - M = -inf: a non-candidate adds exactly 0)
                cnt += x[j] > ly ? 1 : 0;
                arg = x[j] == M ? min(arg, (unsigned)(c + j)) : arg;
            }
        }
    }
    s = wave_sum(s);
    arg = wave_min_u32(arg);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) { sh_s[tid >> 6] = s; sh_c[tid >> 6] = cnt; sh_a[tid >> 6] = arg; }
    __syncthreads();
    float l = 0.f;
    if (TOP || tid == 0) {     // (TOP: every thread forms lse, from the same slots in the same order)
        float S = sh_s[0];
        int C = sh_c[0];
        unsigned A = sh_a[0];
#pragma unroll
        for (int w = 1; w < NW; w++) { S += sh_s[w]; C += sh_c[w]; A = min(A, sh_a[w]); }
        l = M + logf(S);
        if (tid == 0) {
            a.lse[t] = l;
            a.top1[t] = (int)A;
            a.logprob[t] = y_cand ? ly_raw - l : (y_in ? -INFINITY : 0.f);
            a.rank[t] = y_cand ? C : -1;
            a.status[t] = (y_in && !y_cand) ? 1 : 0;
        }
    }
    if constexpr (TOP) {
        __shared__ SelSharedT<NW> sh;
        // The row once more, in place and without a branch: every element becomes its order-preserving key (sel_key; bf16: the upper half,
        // which orders bf16 values just as well), 0 for what is no candidate, so that a round reads a piece without the window or a test.
        // -0.0 and +0.0 keep their own keys in the row (NEG0 + 1 == POS0), so that a winner's logit comes back with its sign; the rounds
        // rank them as one value.
        constexpr int KS = VN == 8 ? 16 : 0;
        constexpr unsigned NEG0 = 0x7fffffffu >> KS;
#pragma unroll
        for (int k = 0; k < SC_NP; k++) {
            const int c = (k * NT + tid) * VN;
            Vec16<T> v;
            v.load(reinterpret_cast<const T*>(&raw[k]));
            unsigned kk[VN];
#pragma unroll
            for (int j = 0; j < VN; j++) kk[j] = (sel_key(v.v[j]) >> KS) & (0u - (unsigned)((c + j >= lo) & (c + j < hi)));
            if constexpr (VN == 8) raw[k] = make_uint4(kk[0] | kk[1] << 16, kk[2] | kk[3] << 16, kk[4] | kk[5] << 16, kk[6] | kk[7] << 16);
            else raw[k] = make_uint4(kk[0], kk[1], kk[2], kk[3]);
        }
        unsigned mk = 0, bk = 0;  // mk: the key of this thread's best pair as stored
        int bo = 0;
        auto step = [&](unsigned ks, int off, unsigned wk, int d) {
            const unsigned before = bk;
            sel_scan_step(ks + (unsigned)(ks == NEG0), off, wk, d, bk, bo);
            mk = bk != before ? ks : mk;     // (a step that takes the element raises bk)
        };
        // z: an opaque zero folded into every word, so that what a round computes from the row is computed there, in every round, and
        // not carried in 8 x 17 registers across the rounds
        auto scan = [&](unsigned long long below) {
            const unsigned wk = (unsigned)(below >> 32);
            const int d = (int)~(unsigned)below - tid * VN;
            const int z = sel_opaque_zero();
            bk = 0;
            bo = 0;
#pragma unroll
            for (int k = 0; k < SC_NP; k++) {
                const unsigned w[4] = {raw[k].x ^ (unsigned)z, raw[k].y ^ (unsigned)z, raw[k].z ^ (unsigned)z, raw[k].w ^ (unsigned)z};
#pragma unroll
                for (int j = 0; j < VN; j++)
                    step(VN == 8 ? ((j & 1) ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu) : w[j & 3], z + (k * NT * VN + j), wk, d);
            }
            return sel_pair(bk, tid * VN + bo);
        };
        // the logit a stored key stands for, bit for bit (bf16: the lower half of sel_key comes back from the sign)
        auto value = [&](unsigned ks) { return sel_unkey(VN == 8 ? (ks << 16) | ((ks & 0x8000u) ? 0u : 0xffffu) : ks); };
        auto emit = [&](int i, unsigned long long w, bool own) {
            if (own) {
                a.top_ids[t * a.top_n + i] = (int)~(unsigned)w;
                a.top_logprob[t * a.top_n + i] = value(mk) - l;
            }
        };
        int ph = 0;
        const int got = sel_top_rounds(a.top_n, 0ull, scan, emit, sh, ph);
        if (tid == 0)
            for (int i = got; i < a.top_n; i++) {
                a.top_ids[t * a.top_n + i] = -1;
                a.top_logprob[t * a.top_n + i] = -INFINITY;
            }
    }
}

extern "C" int db1_score_rows_supported(int V, int64_t ld, int dt) {
    const int VN = dt == DB1_F32 ? 4 : 8;
    return (db1_dt_ok(dt) && V > 0 && ld >= V && ld % VN == 0 && ld <= (int64_t)SC_MAX_ROW) ? 1 : 0;
}

template <bool TOP>
static void sc_dispatch(const ScoreArgs& a, int64_t T_, int64_t ld, int dt, hipStream_t st) {
    if (dt == DB1_BF16) score_rows_kernel<bf16_t, 256, TOP><<<(unsigned)T_, 256, 0, st>>>(a);
    else if (ld <= 256 * 4 * SC_NP) score_rows_kernel<float, 256, TOP><<<(unsigned)T_, 256, 0, st>>>(a);
    else score_rows_kernel<float, 512, TOP><<<(unsigned)T_, 512, 0, st>>>(a);
}

// db1_score_rows (top == false: top_n 0, no buffers) and db1_score_rows_top: one validation order, then the instantiation with or without the rounds
static int sc_rows(const char* who, bool top, const void* logits, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank,
                   int32_t* status, int64_t T_, int V, int64_t ld, int dt, int top_n, int32_t* top_ids, float* top_logprob, int vocab_lo,
                   int vocab_hi, void* stream) {
    if (!db1_dt_ok(dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dt);
    if (T_ <= 0 || T_ > 0x7fffffff || V <= 0 || ld < V) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: T=%lld V=%d ld=%lld", who, (long long)T_, V, (long long)ld);
    if (top && (top_n < 1 || top_n > SC_MAX_TOP)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_n %d (1 .. %d)", who, top_n, SC_MAX_TOP);
    if (!logits || !labels || !lse || !logprob || !top1 || !rank || !status || (top && (!top_ids || !top_logprob)))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (vocab_lo < 0 || vocab_hi > V || vocab_lo >= vocab_hi)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: window [%d, %d) is empty or outside [0, %d)", who, vocab_lo, vocab_hi, V);
    if (!db1_score_rows_supported(V, ld, dt))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: V=%d ld=%lld (rows of at most %d elements, a multiple of 16 bytes)", who, V, (long long)ld, SC_MAX_ROW);
    if (!db1_aligned16(logits)) DB1_FAIL(DB1_ERR_BAD_ALIGN, "%s: logits must be 16-byte aligned", who);
    ScoreArgs a;
    a.logits = logits; a.labels = labels; a.lse = lse; a.logprob = logprob; a.top1 = top1; a.rank = rank; a.status = status;
    a.ld = ld; a.V = V; a.lo = vocab_lo; a.hi = vocab_hi;
    a.top_n = top_n; a.top_ids = top_ids; a.top_logprob = top_logprob;
    hipStream_t st = (hipStream_t)stream;
    if (top) sc_dispatch<true>(a, T_, ld, dt, st); else sc_dispatch<false>(a, T_, ld, dt, st);
    DB1_CHECK_LAUNCH(who);
    return DB1_OK;
}

extern "C" int db1_score_rows(const void* logits, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank, int32_t* status,
                              int64_t T_, int V, int64_t ld, int dt, int vocab_lo, int vocab_hi, void* stream) {
    return sc_rows("score_rows", false, logits, labels, lse, logprob, top1, rank, status, T_, V, ld, dt, 0, nullptr, nullptr, vocab_lo, vocab_hi,
                   stream);
}

extern "C" int db1_score_rows_top(const void* logits, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank,
                                  int32_t* status, int64_t T_, int V, int64_t ld, int dt, int top_n, int32_t* top_ids, float* top_logprob,
                                  int vocab_lo, int vocab_hi, void* stream) {
    return sc_rows("score_rows_top", true, logits, labels, lse, logprob, top1, rank, status, T_, V, ld, dt, top_n, top_ids, top_logprob, vocab_lo,
                   vocab_hi, stream);
}

// ---- the chunked sweep of lmhead_ce.hip with db1_score_rows on every chunk of logits
static inline int64_t sc_al256(int64_t x) { return (x + 255) & ~(int64_t)255; }
struct ScorePlan { int64_t chunk, logits_b, gemm_b, total; };
static ScorePlan score_plan(int64_t T_, int n_w_rows, int d, int chunk_rows, int dt) {
    ScorePlan p;
    p.chunk = chunk_rows > 0 ? chunk_rows : 16384;
    if (p.chunk > T_) p.chunk = T_;
    p.logits_b = sc_al256(p.chunk * (int64_t)n_w_rows * db1_elt_size(dt));
    p.gemm_b = sc_al256(db1_gemm_workspace_bytes((int)p.chunk, n_w_rows, d, dt, dt, dt, d, 1, 1, d, n_w_rows, 1, 1, 1));   // logits = h W^T
    p.total = p.logits_b + p.gemm_b;
    return p;
}

extern "C" int64_t db1_lmhead_score_workspace_bytes(int64_t T_, int n_w_rows, int d, int chunk_rows, int dt) {
    if (T_ <= 0 || n_w_rows <= 0 || d <= 0 || !db1_dt_ok(dt)) return 0;
    return score_plan(T_, n_w_rows, d, chunk_rows, dt).total;
}

// db1_lmhead_score (top == false) and db1_lmhead_score_top: the same sweep (and workspace), db1_score_rows or db1_score_rows_top on every chunk
static int sc_lmhead(const char* who, bool top, const void* h, const void* W, const int64_t* labels, float* lse, float* logprob, int32_t* top1,
                     int32_t* rank, int32_t* status, int64_t T_, int V, int n_w_rows, int d, int vocab_lo, int vocab_hi, int chunk_rows, int dt,
                     int top_n, int32_t* top_ids, float* top_logprob, void* ws, int64_t ws_bytes, void* stream) {
    if (!db1_dt_ok(dt)) DB1_FAIL(DB1_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dt);
    if (T_ <= 0 || V <= 0 || n_w_rows < V || d <= 0 || chunk_rows < 0)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: T=%lld V=%d rows=%d d=%d chunk_rows=%d", who, (long long)T_, V, n_w_rows, d, chunk_rows);
    if (top && (top_n < 1 || top_n > SC_MAX_TOP)) DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: top_n %d (1 .. %d)", who, top_n, SC_MAX_TOP);
    if (!h || !W || !labels || !lse || !logprob || !top1 || !rank || !status || (top && (!top_ids || !top_logprob)))
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: null buffer", who);
    if (vocab_lo < 0 || vocab_hi > V || vocab_lo >= vocab_hi)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "%s: window [%d, %d) is empty or outside [0, %d)", who, vocab_lo, vocab_hi, V);
    if (!db1_score_rows_supported(V, n_w_rows, dt))
        DB1_FAIL(DB1_ERR_UNSUPPORTED, "%s: V=%d rows=%d (rows of at most %d elements, a multiple of 16 bytes)", who, V, n_w_rows, SC_MAX_ROW);
    const ScorePlan p = score_plan(T_, n_w_rows, d, chunk_rows, dt);
    DB1_NEED_WS(ws, ws_bytes, p.total, who);
    const int es = db1_elt_size(dt);
    char* logits = (char*)ws;
    void* gws = logits + p.logits_b;
    for (int64_t r0 = 0; r0 < T_; r0 += p.chunk) {
        const int rows = (int)((T_ - r0 < p.chunk) ? (T_ - r0) : p.chunk);
        int rc = db1_gemm_strided((const char*)h + r0 * d * es, W, logits, nullptr, rows, n_w_rows, d, dt, dt, dt, 0, d, 1, 1, d, n_w_rows, 1, 1, 1, 0, 0,
                                  0, 0, 0, 0, 1.f, 0.f, gws, p.gemm_b, stream);                                   // logits = h W^T
        if (rc) return rc;
        rc = top ? db1_score_rows_top(logits, labels + r0, lse + r0, logprob + r0, top1 + r0, rank + r0, status + r0, rows, V, n_w_rows, dt, top_n,
                                      top_ids + r0 * top_n, top_logprob + r0 * top_n, vocab_lo, vocab_hi, stream)
                 : db1_score_rows(logits, labels + r0, lse + r0, logprob + r0, top1 + r0, rank + r0, status + r0, rows, V, n_w_rows, dt, vocab_lo,
                                  vocab_hi, stream);
        if (rc) return rc;
    }
    return DB1_OK;
}

extern "C" int db1_lmhead_score(const void* h, const void* W, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank,
                                int32_t* status, int64_t T_, int V, int n_w_rows, int d, int vocab_lo, int vocab_hi, int chunk_rows, int dt,
                                void* ws, int64_t ws_bytes, void* stream) {
    return sc_lmhead("lmhead_score", false, h, W, labels, lse, logprob, top1, rank, status, T_, V, n_w_rows, d, vocab_lo, vocab_hi, chunk_rows, dt, 0,
                     nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int db1_lmhead_score_top(const void* h, const void* W, const int64_t* labels, float* lse, float* logprob, int32_t* top1, int32_t* rank,
                                    int32_t* status, int64_t T_, int V, int n_w_rows, int d, int vocab_lo, int vocab_hi, int chunk_rows, int dt,
                                    int top_n, int32_t* top_ids, float* top_logprob, void* ws, int64_t ws_bytes, void* stream) {
    return sc_lmhead("lmhead_score_top", true, h, W, labels, lse, logprob, top1, rank, status, T_, V, n_w_rows, d, vocab_lo, vocab_hi, chunk_rows, dt,
                     top_n, top_ids, top_logprob, ws, ws_bytes, stream);
}

// ---- per-sequence sums: one workgroup per segment, double accumulators, fixed order
__global__ __launch_bounds__(256) void score_segments_kernel(const float* __restrict__ logprob, const int* __restrict__ rank,
                                                             const int64_t* __restrict__ labels, const float* __restrict__ mask,
                                                             float* __restrict__ out, int64_t seg_len, int V) {
    __shared__ double red[3][256];
    const int64_t base = (int64_t)blockIdx.x * seg_len;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t i = threadIdx.x; i < seg_len; i += 256) {
        const int64_t y = labels[base + i];
        const float mk = (y >= 0 && y < V) ? mask[base + i] : 0.f;
        if (mk != 0.f) {                 // (0 * -inf would be NaN: a row that is masked out adds nothing, whatever its log-prob)
            s0 += (double)mk * (double)logprob[base + i];
            s1 += (double)mk;
            s2 += rank[base + i] == 0 ? (double)mk : 0.0;
        }
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int q = 0; q < 3; q++) red[q][threadIdx.x] += red[q][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 3) out[(int64_t)blockIdx.x * 3 + threadIdx.x] = (float)red[threadIdx.x][0];
}

extern "C" int db1_score_segments(const float* logprob, const int32_t* rank, const int64_t* labels, const float* mask, float* out, int64_t n_seg,
                                  int64_t seg_len, int V, void* stream) {
    if (n_seg <= 0 || n_seg > 0x7fffffff || seg_len <= 0 || V <= 0)
        DB1_FAIL(DB1_ERR_BAD_SHAPE, "score_segments: n_seg=%lld seg_len=%lld V=%d", (long long)n_seg, (long long)seg_len, V);
    if (!logprob || !rank || !labels || !mask || !out) DB1_FAIL(DB1_ERR_BAD_SHAPE, "score_segments: null buffer");
    score_segments_kernel<<<(unsigned)n_seg, 256, 0, (hipStream_t)stream>>>(logprob, rank, labels, mask, out, seg_len, V);
    DB1_CHECK_LAUNCH("score_segments");
    return DB1_OK;
}
