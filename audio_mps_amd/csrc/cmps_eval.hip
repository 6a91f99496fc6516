// Held-out evaluation: the per-clip losses of a pass over a dataset reduced where they are (include/cmps.h states the record and the contract;
// tests/_eval_ref.py restates both in numpy).
//
// k_loss_stats (cmps_loss_stats): folds loss[0 .. B) -- clip ids first_id .. first_id + B - 1 -- into ONE 64-byte record in device memory:
// sum and sum of squares of the finite losses in double (a float32 squared in double is exact), the counts of finite and non-finite values,
// minimum and maximum with the ids that hold them (the lowest id on ties) and the lowest id of a non-finite value.  A pass over thousands of
// clips then downloads 64 bytes once instead of every batch's losses.
// ONE workgroup of STATS_NT threads, no atomics: thread t folds elements t, t + STATS_NT, ... in that order into a record in registers, the
// STATS_NT records are merged by a binary tree in LDS (t takes t + w for w = STATS_NT / 2, ..., 1), and thread 0 merges the result behind
// what the record held (reset == 0) or in its place, and writes it with plain stores.  Assignment and tree are fixed, and the update is
// ordered by the stream, so the same sequence of calls gives the same bits on every run.  A batch is a few thousand floats: one workgroup
// reads it in a few microseconds, and more of them would need the second pass or the atomics this kernel does without.
// k_classify_stats (cmps_bank_classify_stats), further down: the [M][B] losses of a bank of one model per class judged as a classifier.
// k_classify_weights (cmps_bank_classify_weights), behind it: the same losses turned into the per-clip, per-member cotangents of a cross-entropy step.
// k_bank_posterior (cmps_bank_posterior), behind that: the per-step losses of a scored bank stream folded into a posterior over the members after every step.
// k_calib_pass, k_calib_update (cmps_bank_calibrate), last: the [M][N] losses of a held-out set fitted for the temperature and the prior.
#include "cmps_internal.h"

namespace cmps {

namespace {

constexpr int STATS_NT = 256;

struct alignas(8) LossStats {          // the record of include/cmps.h (cmps_loss_stats), field for field
    double sum, sumsq;
    long long n_finite, n_nonfinite, argmin, argmax, first_nonfinite;
    float min, max;
};
static_assert(sizeof(LossStats) == 64, "the record of cmps_loss_stats is 64 bytes");

__device__ __forceinline__ LossStats stats_empty() {
    return LossStats{0.0, 0.0, 0ll, 0ll, -1ll, -1ll, -1ll, __uint_as_float(0x7f800000u), __uint_as_float(0xff800000u)};
}

// One value of a thread's own sequence: its ids arrive in increasing order, so a tie keeps what is there
__device__ __forceinline__ void stats_add(LossStats& r, float x, long long id) {
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {                        // NaN, +Inf, -Inf
        r.n_nonfinite += 1;
        if (r.first_nonfinite < 0) r.first_nonfinite = id;
        return;
    }
    const double d = (double)x;
    r.sum += d;
    r.sumsq += d * d;
    if (r.n_finite == 0 || x < r.min) { r.min = x; r.argmin = id; }
    if (r.n_finite == 0 || x > r.max) { r.max = x; r.argmax = id; }
    r.n_finite += 1;
}

// a <- a merged with b, whatever ids either holds: a tie goes to the lower id
__device__ __forceinline__ void stats_merge(LossStats& a, const LossStats& b) {
    a.sum += b.sum;
    a.sumsq += b.sumsq;
    if (b.n_finite > 0) {
        if (a.n_finite == 0 || b.min < a.min || (b.min == a.min && b.argmin < a.argmin)) { a.min = b.min; a.argmin = b.argmin; }
        if (a.n_finite == 0 || b.max > a.max || (b.max == a.max && b.argmax < a.argmax)) { a.max = b.max; a.argmax = b.argmax; }
    }
    a.n_finite += b.n_finite;
    a.n_nonfinite += b.n_nonfinite;
    if (b.first_nonfinite >= 0 && (a.first_nonfinite < 0 || b.first_nonfinite < a.first_nonfinite)) a.first_nonfinite = b.first_nonfinite;
}

// grid 1
__global__ __launch_bounds__(STATS_NT) void k_loss_stats(const float* __restrict__ loss, int B, long long first_id, int reset,
                                                         LossStats* __restrict__ out) {
    __shared__ LossStats part[STATS_NT];
    const int tid = threadIdx.x;
    LossStats r = stats_empty();
    for (int b = tid; b < B; b += STATS_NT) stats_add(r, loss[b], first_id + (long long)b);
    part[tid] = r;
    __syncthreads();
    for (int w = STATS_NT / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            LossStats a = part[tid];
            stats_merge(a, part[tid + w]);
            part[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) {
        LossStats total = part[0];
        if (!reset) {
            LossStats before = *out;
            stats_merge(before, total);
            total = before;
        }
        *out = total;
    }
}

// k_classify_stats (cmps_bank_classify_stats): the [M][B] losses of a bank forward judged as a classifier, into the record of include/cmps.h
// (tests/_classify_ref.py restates it).  ONE workgroup of STATS_NT threads, as k_loss_stats: thread t takes clips t, t + STATS_NT, ... in that
// order and walks the M losses of each (loss[m * ld + b]: neighbouring threads read neighbouring floats, every load of a member's row is
// coalesced); its two double sums and seven integers go through the same binary tree in LDS, and thread 0 merges the result behind (or in
// place of) the header.  The confusion matrix and unlabelled_best are integer counts: every thread adds its own clips with vector atomic
// adds -- an integer sum does not depend on the order -- after all threads have zeroed them where reset says so.
struct alignas(8) ClassifyHead {       // the header of the record of include/cmps.h (cmps_bank_classify_stats), field for field
    double sum_xent, sum_margin;
    long long n_decided, n_undecided, n_unlabelled, n_correct, n_xent, n_margin, first_undecided;
};
static_assert(sizeof(ClassifyHead) == 72, "the header of cmps_bank_classify_stats is 72 bytes");

__device__ __forceinline__ void classify_merge(ClassifyHead& a, const ClassifyHead& b) {
    a.sum_xent += b.sum_xent;
    a.sum_margin += b.sum_margin;
    a.n_decided += b.n_decided;
    a.n_undecided += b.n_undecided;
    a.n_unlabelled += b.n_unlabelled;
    a.n_correct += b.n_correct;
    a.n_xent += b.n_xent;
    a.n_margin += b.n_margin;
    if (b.first_undecided >= 0 && (a.first_undecided < 0 || b.first_undecided < a.first_undecided)) a.first_undecided = b.first_undecided;
}

__device__ __forceinline__ bool is_finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// grid 1
__global__ __launch_bounds__(STATS_NT) void k_classify_stats(const float* __restrict__ loss, int M, int B, long long ld,
                                                             const int* __restrict__ label, long long first_id, int reset,
                                                             ClassifyHead* __restrict__ head, int* __restrict__ best_out) {
    __shared__ ClassifyHead part[STATS_NT];
    const int tid = threadIdx.x;
    unsigned long long* confusion = reinterpret_cast<unsigned long long*>(head + 1);          // [M][M], then unlabelled_best [M]
    unsigned long long* unlabelled_best = confusion + (size_t)M * (size_t)M;
    if (reset) {
        const size_t n = (size_t)M * (size_t)M + (size_t)M;
        for (size_t i = tid; i < n; i += STATS_NT) confusion[i] = 0ull;
        __threadfence();              // the zeros are in place before any thread of the workgroup adds to them
        __syncthreads();
    }
    ClassifyHead r{0.0, 0.0, 0ll, 0ll, 0ll, 0ll, 0ll, 0ll, -1ll};
    for (int b = tid; b < B; b += STATS_NT) {
        const float* col = loss + b;
        float l1 = __uint_as_float(0x7f800000u), l2 = l1;                                     // smallest and second-smallest finite loss
        int best = -1, n_finite = 0;
#pragma unroll 8
        for (int m = 0; m < M; ++m) {
            const float x = col[(long long)m * ld];
            if (is_finite_f32(x)) {
                ++n_finite;
                if (x < l1) { l2 = l1; l1 = x; best = m; }                                    // (strict: the lowest m keeps a tie)
                else if (x < l2) l2 = x;
            }
        }
        if (best_out) best_out[b] = best;
        if (n_finite == 0) {
            r.n_undecided += 1;
            if (r.first_undecided < 0) r.first_undecided = first_id + (long long)b;           // (a thread's ids arrive in increasing order)
            continue;
        }
        r.n_decided += 1;
        if (n_finite >= 2) {
            r.sum_margin += (double)l2 - (double)l1;
            r.n_margin += 1;
        }
        const int y = label ? label[b] : -1;
        if (y < 0 || y >= M) {
            r.n_unlabelled += 1;
            atomicAdd(unlabelled_best + best, 1ull);
            continue;
        }
        atomicAdd(confusion + (size_t)y * (size_t)M + (size_t)best, 1ull);
        if (y == best) r.n_correct += 1;
        const float xl = col[(long long)y * ld];
        if (!is_finite_f32(xl)) continue;
        double S = 0.0;                                                                       // sum over the finite members, in member order,
#pragma unroll 4
        for (int m = 0; m < M; ++m) {                                                         // of exp(-(loss_m - min)): 1 <= S <= M
            const float x = col[(long long)m * ld];
            if (is_finite_f32(x)) S += exp(-((double)x - (double)l1));
        }
        r.sum_xent += ((double)xl - (double)l1) + log(S);
        r.n_xent += 1;
    }
    part[tid] = r;
    __syncthreads();
    for (int w = STATS_NT / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            ClassifyHead a = part[tid];
            classify_merge(a, part[tid + w]);
            part[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) {
        ClassifyHead total = part[0];
        if (!reset) {
            ClassifyHead before = *head;
            classify_merge(before, total);
            total = before;
        }
        *head = total;
    }
}

// k_classify_weights (cmps_bank_classify_weights): the same [M][B] losses and the labels turned into the [M][B] cotangents of the
// cross-entropy objective of include/cmps.h (tests/_disc_ref.py restates it), w[m][b] = d J_b / d loss[m][b] with
// J_b = alpha loss[y][b] + beta xent_b, and into a 40-byte record.  ONE workgroup of STATS_NT threads, as k_classify_stats: thread t takes
// clips t, t + STATS_NT, ... in that order and walks the M losses of each three times (smallest present loss; S; the weights), every
// pass's loads and the stores coalesced over neighbouring clips.  Every weight[m * ldw + b], m < M, b < B, is written exactly once, a
// skipped clip's and an absent member's with +0.  The record's two double sums and three counts go through the binary tree in LDS.
struct alignas(8) ClassifyWeightsRec {   // the record of include/cmps.h (cmps_bank_classify_weights), field for field
    double sum_xent, sum_own_loss;
    long long n_used, n_unlabelled, n_own_absent;
};
static_assert(sizeof(ClassifyWeightsRec) == 40, "the record of cmps_bank_classify_weights is 40 bytes");

__device__ __forceinline__ void weights_merge(ClassifyWeightsRec& a, const ClassifyWeightsRec& b) {
    a.sum_xent += b.sum_xent;
    a.sum_own_loss += b.sum_own_loss;
    a.n_used += b.n_used;
    a.n_unlabelled += b.n_unlabelled;
    a.n_own_absent += b.n_own_absent;
}

// grid 1
__global__ __launch_bounds__(STATS_NT) void k_classify_weights(const float* __restrict__ loss, int M, int B, long long ld,
                                                               const int* __restrict__ label, double kappa, double alpha, double beta,
                                                               int reset, float* __restrict__ weight, long long ldw,
                                                               ClassifyWeightsRec* __restrict__ rec) {
    __shared__ ClassifyWeightsRec part[STATS_NT];
    const int tid = threadIdx.x;
    const double bk = beta * kappa;
    ClassifyWeightsRec r{0.0, 0.0, 0ll, 0ll, 0ll};
    for (int b = tid; b < B; b += STATS_NT) {
        const float* col = loss + b;
        float* wcol = weight + b;
        const int y = label[b];
        const bool labelled = y >= 0 && y < M;
        const float xl = labelled ? col[(long long)y * ld] : 0.f;
        if (!labelled || !is_finite_f32(xl)) {                                                // skipped: every weight of the clip is +0
            if (!labelled) r.n_unlabelled += 1; else r.n_own_absent += 1;
            for (int m = 0; m < M; ++m) wcol[(long long)m * ldw] = 0.f;
            continue;
        }
        float l1 = xl;                                                                        // smallest present loss (the own one is present)
#pragma unroll 8
        for (int m = 0; m < M; ++m) {
            const float x = col[(long long)m * ld];
            if (is_finite_f32(x) && x < l1) l1 = x;
        }
        double S = 0.0;                                                                       // in member order: 1 <= S <= M
#pragma unroll 4
        for (int m = 0; m < M; ++m) {
            const float x = col[(long long)m * ld];
            if (is_finite_f32(x)) S += exp(-(kappa * ((double)x - (double)l1)));
        }
#pragma unroll 4
        for (int m = 0; m < M; ++m) {
            const float x = col[(long long)m * ld];
            float w = 0.f;
            if (is_finite_f32(x)) {
                const double d = m == y ? 1.0 : 0.0;
                const double p = exp(-(kappa * ((double)x - (double)l1))) / S;
                w = (float)(alpha * d + bk * (d - p));
            }
            wcol[(long long)m * ldw] = w;
        }
        r.sum_xent += kappa * ((double)xl - (double)l1) + log(S);
        r.sum_own_loss += (double)xl;
        r.n_used += 1;
    }
    part[tid] = r;
    __syncthreads();
    for (int w = STATS_NT / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            ClassifyWeightsRec a = part[tid];
            weights_merge(a, part[tid + w]);
            part[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) {
        ClassifyWeightsRec total = part[0];
        if (!reset) {
            ClassifyWeightsRec before = *rec;
            weights_merge(before, total);
            total = before;
        }
        *rec = total;
    }
}

// k_bank_posterior (cmps_bank_posterior): the per-step losses nll[M][n][steps] of a scored bank stream folded into the running totals and,
// after EVERY step, the posterior over the members, the best member, its probability and the first step at which the bank was sure
// (include/cmps.h states it; tests/_posterior_ref.py restates it).  Two shapes of work: per row (m, g) a chain of `steps` dependent float32
// additions -- the fold of the score kernels, bit for bit, so no tree scan -- and per (g, k) a soft-max over the M members in double.
// ONE workgroup of POST_NT threads per path g; the steps go by in chunks of C (64; 32 above 512 members, where the tile has to fit the LDS):
//   load    thread (part, k) = (t / C, t % C) holds step k of the rows part, part + P, ... (P = POST_NT / C) of the chunk in R registers --
//           every load is C consecutive floats of one row -- and puts them into tile[m][C + 1]; the NEXT chunk's loads are issued right
//           behind, so they are in flight while this chunk is folded and judged (R = the rows a thread holds, a template parameter)
//   fold    thread t walks rows t, t + POST_NT, ... of the tile with the total in a register and leaves the running totals in place
//           (the odd row pitch spreads the lanes of a wave over the banks)
//   judge   thread (part, k) takes step k and the members part, part + P, ...: the smallest a and its member, then the sum of
//           exp(-(a - amin)), each merged over the P parts through LDS in part order; post, best and conf from there
//   decide  wave 0 holds the path's decision record in registers: one ballot over the chunk's steps, the lowest set bit is the first
// nll is read once, the only scratch is LDS, nothing is atomic, and the assignment of work to threads is fixed: the same bits on every run.
constexpr int POST_NT = 512;
constexpr int POST_ROWS = CLASSIFY_MAX_M / POST_NT;      // rows of the tile a thread folds, at most

struct alignas(8) BankDecision {       // the record of include/cmps.h (cmps_bank_decision), field for field
    long long step;
    int member, reserved;
};
static_assert(sizeof(BankDecision) == 16, "the record of cmps_bank_posterior is 16 bytes");

// grid n; dynamic LDS posterior_lds_bytes(M, C); R > 0: M <= R * POST_NT / C, the next chunk prefetched; R == 0: any M, no prefetch
template <int C, int R>
__global__ __launch_bounds__(POST_NT) void k_bank_posterior(const float* __restrict__ nll, int M, int n, int steps, const float* total_in,
                                                            const double* __restrict__ log_prior, double kappa, float* total_out,
                                                            float* __restrict__ post, int* __restrict__ best_out,
                                                            float* __restrict__ conf_out, double threshold, long long first_step, int reset,
                                                            BankDecision* __restrict__ decision) {
    constexpr int P = POST_NT / C, LD = C + 1;
    extern __shared__ __attribute__((aligned(8))) unsigned char post_lds[];
    __shared__ double s_min[POST_NT], s_sum[POST_NT];
    __shared__ int s_arg[POST_NT];
    double* lp = reinterpret_cast<double*>(post_lds);                                        // [M]
    float* tile = reinterpret_cast<float*>(lp + M);                                           // [M][LD]
    const int tid = threadIdx.x, k = tid % C, part = tid / C;
    const size_t g = blockIdx.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int m = tid; m < M; m += POST_NT) lp[m] = log_prior ? log_prior[m] : 0.0;
    float tot[POST_ROWS];
#pragma unroll
    for (int j = 0; j < POST_ROWS; ++j) {
        const int m = tid + j * POST_NT;
        tot[j] = (m < M && total_in) ? total_in[(size_t)m * n + g] : 0.f;
    }
    long long d_step = -1ll;                                                                  // (wave 0: the path's record)
    int d_member = -1, d_reserved = 0;
    if (decision && !reset && tid < 64) {
        const BankDecision r = decision[g];
        d_step = r.step, d_member = r.member, d_reserved = r.reserved;
    }
    float pre[R > 0 ? R : 1];                                                                 // this thread's part of the chunk to come
    auto fetch = [&](int k0) {
        const bool in = k0 + k < steps;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int m = part + i * P;
            pre[i] = (in && m < M) ? nll[((size_t)m * n + g) * steps + k0 + k] : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < steps; k0 += C) {
        const int len = steps - k0 < C ? steps - k0 : C;
        if constexpr (R > 0) {
            if (k < len) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int m = part + i * P;
                    if (m < M) tile[m * LD + k] = pre[i];
                }
            }
            if (k0 + C < steps) fetch(k0 + C);     // in flight while this chunk is folded and judged
        } else if (k < len) {                      // R == 0, the banks too wide to hold a chunk in registers: dozens of loads a thread anyway
#pragma unroll 8
            for (int m = part; m < M; m += P) tile[m * LD + k] = nll[((size_t)m * n + g) * steps + k0 + k];
        }
        __syncthreads();                          // (also: lp is in place before the first chunk is judged)
#pragma unroll
        for (int j = 0; j < POST_ROWS; ++j) {
            const int m = tid + j * POST_NT;
            if (m < M) {
                float* row = tile + m * LD;
                float c = tot[j];
                if (len == C) {                   // a whole chunk: the offsets are constants, the row's reads go out ahead of the chain
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        c += row[i];              // ONE float32 addition per step, in step order
                        row[i] = c;
                    }
                } else {
#pragma unroll 8
                    for (int i = 0; i < len; ++i) {
                        c += row[i];
                        row[i] = c;
                    }
                }
                tot[j] = c;
            }
        }
        __syncthreads();
        double amin = inf;
        int arg = -1;
        if (k < len)
            for (int m = part; m < M; m += P) {
                const float c = tile[m * LD + k];
                if (is_finite_f32(c)) {
                    const double a = kappa * (double)c - lp[m];
                    if (a < amin) { amin = a; arg = m; }          // (strict, m ascending: the lowest m keeps a tie; a = +inf never wins)
                }
            }
        s_min[tid] = amin;
        s_arg[tid] = arg;
        __syncthreads();
        amin = inf, arg = -1;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const double a = s_min[p * C + k];
            const int r = s_arg[p * C + k];
            if (r >= 0 && (arg < 0 || a < amin || (a == amin && r < arg))) { amin = a; arg = r; }
        }
        double S = 0.0;
        if (k < len && arg >= 0) {
#pragma unroll 4
            for (int m = part; m < M; m += P) {   // (no branch around the exp: the members' terms can overlap; exp(-inf) = +0)
                const float c = tile[m * LD + k];
                S += exp(is_finite_f32(c) ? -((kappa * (double)c - lp[m]) - amin) : -inf);
            }
        }
        s_sum[tid] = S;
        __syncthreads();
        S = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) S += s_sum[p * C + k];
        const double inv_S = arg >= 0 ? 1.0 / S : 0.0;
        if (k < len) {
            const size_t at = g * steps + k0 + k;
            if (post)
                for (int m = part; m < M; m += P) {
                    const float c = tile[m * LD + k];
                    float p = 0.f;
                    if (arg >= 0 && is_finite_f32(c)) p = (float)(exp(-((kappa * (double)c - lp[m]) - amin)) / S);
                    post[(size_t)m * n * steps + at] = p;
                }
            if (part == 0) {
                if (best_out) best_out[at] = arg;
                if (conf_out) conf_out[at] = (float)inv_S;
            }
        }
        if (decision && tid < 64) {                // part 0 sits in wave 0's lanes 0 .. C - 1: lane k is step k0 + k
            const unsigned long long sure = __ballot(part == 0 && k < len && arg >= 0 && inv_S >= threshold);
            if (d_step < 0 && sure != 0ull) {
                const int first = __ffsll((long long)sure) - 1;
                d_step = first_step + (long long)(k0 + first);
                d_member = __shfl(arg, first);
            }
        }
        if (post) __syncthreads();                // post was the tile's last reader; without it the barrier behind the partial sums was,
                                                  // and the three arrays are rewritten only behind two barriers of the next chunk
    }
    if (total_out) {
#pragma unroll
        for (int j = 0; j < POST_ROWS; ++j) {
            const int m = tid + j * POST_NT;
            if (m < M) total_out[(size_t)m * n + g] = tot[j];
        }
    }
    if (decision && tid == 0) decision[g] = BankDecision{d_step, d_member, d_reserved};
}

inline size_t posterior_lds_bytes(int M, int C) { return (size_t)M * (sizeof(double) + sizeof(float) * (size_t)(C + 1)); }

// k_calib_pass, k_calib_update (cmps_bank_calibrate): the temperature and the prior of a class bank fitted on the [M][N] losses of a held-out
// set where they lie (include/cmps.h states the model, the objective and the contract; tests/_calib_ref.py restates them).  One iteration
// is two launches, so an iteration boundary is a kernel boundary and no workgroup ever waits for another:
//   k_calib_pass    G = calib_groups(N) workgroups of ONE wave; workgroup w takes the tiles w, w + G, ... of CALIB_TILE consecutive clips,
//                   thread t clip t of the tile, and walks the M losses of its clip (loss[m * ld + b]: the lanes read consecutive floats):
//                   smallest present loss; smallest a; S and the two moments; then, CALIB_TILE members at a time, p_m into a tile in LDS
//                   that thread j walks for member j in clip order and adds to the workgroup's q[m].  J, g, h and the three counts go
//                   through a binary tree in LDS; n_m is an integer count (LDS integer adds: no order to depend on).  The workgroup's sums
//                   go to its own row of the scratch buffer.
//   k_calib_update  ONE workgroup: adds the G rows in row order (thread per quantity, thread per member), takes the maximum residual through
//                   a tree, and thread 0 decides: converged, out of iterations, a kappa step or a prior sweep.  The state of the solver
//                   (CalibState), the best theta seen and a `done` word live at the head of the scratch buffer.
// The entry enqueues max_iter + 1 such pairs without looking; once `done` is set every later launch leaves at its first branch.  The
// assignment of clips to threads and every order of summation are fixed: the same call gives the same bits on every run.
constexpr int CALIB_TILE = 64;         // clips of a tile = threads of a pass workgroup = members of a p-tile
constexpr int CALIB_MAX_G = 1024;      // workgroups of a pass, at most: the update kernel adds that many rows per quantity
constexpr int CALIB_UPD_NT = 256;
constexpr int CALIB_UPD_ROWS = CLASSIFY_MAX_M / CALIB_UPD_NT;
constexpr int CALIB_ROW_HEAD = 8;      // 8-byte words of a row before q[M] and n_m[M]: J, g, h sums, n_used, n_unlabelled, n_own_absent, 2 spare

struct alignas(8) CalibRec {           // the record of include/cmps.h (cmps_bank_calibrate_rec), field for field
    double xent_start, xent_end, g_logk, resid_prior, curvature;
    long long n_used, n_unlabelled, n_own_absent;
    int passes, flags, n_unfitted, reserved;
};
static_assert(sizeof(CalibRec) == 80, "the record of cmps_bank_calibrate is 80 bytes");

struct alignas(8) CalibState {         // the head of the scratch buffer: what one update launch leaves for the next
    int done, iter, last, lo_known, hi_known, have_best, spare0, spare1;
    double lo, hi;                     // the sign bracket of g in kappa: g(lo) < 0 < g(hi) where the end is known, else the box's end
    double best_J, best_g, best_h, best_resid, xent_start;
    double spare[5];
};
static_assert(sizeof(CalibState) == 128, "the solver state is 128 bytes");
constexpr int CALIB_STEP_KAPPA = 1, CALIB_STEP_PRIOR = 2;                                      // CalibState::last
constexpr int CALIB_DO_SAVE = 1, CALIB_DO_SWEEP = 2, CALIB_DO_RESTORE = 4;                      // what thread 0 asks of the workgroup
constexpr int CALIB_CONVERGED = 1, CALIB_AT_MIN = 2, CALIB_AT_MAX = 4, CALIB_NO_DATA = 8, CALIB_MAX_ITER = 16;

__host__ __device__ inline int calib_groups(long long N) {
    const long long tiles = (N + CALIB_TILE - 1) / CALIB_TILE;
    return (int)(tiles < CALIB_MAX_G ? tiles : CALIB_MAX_G);
}
// scratch: CalibState | best theta [1 + M] | rows [G][CALIB_ROW_HEAD + 2 M], everything in 8-byte words
__host__ __device__ inline size_t calib_row_words(int M) { return (size_t)CALIB_ROW_HEAD + 2 * (size_t)M; }

// grid G
__global__ __launch_bounds__(CALIB_TILE) void k_calib_pass(const float* __restrict__ loss, int M, long long N, long long ld,
                                                           const int* __restrict__ label, const double* __restrict__ theta,
                                                           unsigned char* __restrict__ scratch, int first) {
    if (!first && reinterpret_cast<const CalibState*>(scratch)->done) return;
    __shared__ double ptile[CALIB_TILE][CALIB_TILE + 1];
    __shared__ double qacc[CLASSIFY_MAX_M];
    __shared__ unsigned long long cnt[CLASSIFY_MAX_M];
    __shared__ double red[3][CALIB_TILE];
    __shared__ long long redn[3][CALIB_TILE];
    const int tid = threadIdx.x;
    const double kappa = theta[0];
    const double* c = theta + 1;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int m = tid; m < M; m += CALIB_TILE) { qacc[m] = 0.0; cnt[m] = 0ull; }
    __syncthreads();
    double sJ = 0.0, sg = 0.0, sh = 0.0;
    long long n_used = 0, n_unl = 0, n_abs = 0;
    const long long tiles = (N + CALIB_TILE - 1) / CALIB_TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long b = tile * CALIB_TILE + tid;
        const float* col = loss + b;
        bool used = false;
        int y = -1;
        float l1 = 0.f;
        double amin = 0.0, inv_S = 0.0;
        if (b < N) {
            y = label[b];
            const bool labelled = y >= 0 && y < M;
            const float xl = labelled ? col[(long long)y * ld] : 0.f;
            if (!labelled) n_unl += 1;
            else if (!is_finite_f32(xl)) n_abs += 1;
            else {
                used = true;
                l1 = xl;                                                                      // smallest present loss (the own one is present)
#pragma unroll 8
                for (int m = 0; m < M; ++m) {
                    const float x = col[(long long)m * ld];
                    if (is_finite_f32(x) && x < l1) l1 = x;
                }
                amin = inf;
#pragma unroll 4
                for (int m = 0; m < M; ++m) {
                    const float x = col[(long long)m * ld];
                    if (is_finite_f32(x)) {
                        const double a = kappa * ((double)x - (double)l1) - c[m];
                        if (a < amin) amin = a;
                    }
                }
                double S = 0.0, S1 = 0.0, S2 = 0.0;                                           // in member order
#pragma unroll 4
                for (int m = 0; m < M; ++m) {
                    const float x = col[(long long)m * ld];
                    if (is_finite_f32(x)) {
                        const double d = (double)x - (double)l1;
                        const double e = exp(-((kappa * d - c[m]) - amin));
                        S += e;
                        S1 += e * d;
                        S2 += e * (d * d);
                    }
                }
                inv_S = 1.0 / S;
                const double dy = (double)xl - (double)l1;
                const double E = S1 * inv_S;
                sJ += ((kappa * dy - c[y]) - amin) + log(S);
                sg += dy - E;
                sh += S2 * inv_S - E * E;
                n_used += 1;
                atomicAdd(cnt + y, 1ull);
            }
        }
        for (int m0 = 0; m0 < M; m0 += CALIB_TILE) {                                          // (uniform: every thread meets the barriers)
            const int len = M - m0 < CALIB_TILE ? M - m0 : CALIB_TILE;
            for (int j = 0; j < len; ++j) {
                double p = 0.0;
                if (used) {
                    const float x = col[(long long)(m0 + j) * ld];
                    if (is_finite_f32(x)) p = exp(-((kappa * ((double)x - (double)l1) - c[m0 + j]) - amin)) * inv_S;
                }
                ptile[j][tid] = p;
            }
            __syncthreads();
            if (tid < len) {
                double s = 0.0;
#pragma unroll 8
                for (int i = 0; i < CALIB_TILE; ++i) s += ptile[tid][i];                      // in clip order
                qacc[m0 + tid] += s;                                                          // in tile order
            }
            __syncthreads();
        }
    }
    red[0][tid] = sJ, red[1][tid] = sg, red[2][tid] = sh;
    redn[0][tid] = n_used, redn[1][tid] = n_unl, redn[2][tid] = n_abs;
    __syncthreads();
    for (int w = CALIB_TILE / 2; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                red[i][tid] += red[i][tid + w];
                redn[i][tid] += redn[i][tid + w];
            }
        }
        __syncthreads();
    }
    unsigned long long* row = reinterpret_cast<unsigned long long*>(scratch + sizeof(CalibState)) + (size_t)(1 + M) +
                              (size_t)blockIdx.x * calib_row_words(M);
    if (tid < 3) {
        reinterpret_cast<double*>(row)[tid] = red[tid][0];
        reinterpret_cast<long long*>(row)[3 + tid] = redn[tid][0];
    }
    for (int m = tid; m < M; m += CALIB_TILE) {
        reinterpret_cast<double*>(row)[CALIB_ROW_HEAD + m] = qacc[m];
        row[CALIB_ROW_HEAD + M + m] = cnt[m];
    }
}

// grid 1
__global__ __launch_bounds__(CALIB_UPD_NT) void k_calib_update(double* __restrict__ theta, CalibRec* __restrict__ rec,
                                                               unsigned char* __restrict__ scratch, int M, int G, int fit, int max_iter,
                                                               double tol, double kmin, double kmax, int first) {
    CalibState* st = reinterpret_cast<CalibState*>(scratch);
    if (!first && st->done) return;
    __shared__ double s_sum[3];
    __shared__ long long s_cnt[3];
    __shared__ double s_res[CALIB_UPD_NT];
    __shared__ int s_unf[CALIB_UPD_NT];
    __shared__ int s_do;
    const int tid = threadIdx.x;
    double* best = reinterpret_cast<double*>(scratch + sizeof(CalibState));                   // [1 + M]
    const unsigned long long* rows = reinterpret_cast<const unsigned long long*>(best + 1 + M);
    const size_t W = calib_row_words(M);
    if (tid < 3) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += reinterpret_cast<const double*>(rows + (size_t)g * W)[tid];          // in row order
        s_sum[tid] = s;
    } else if (tid < 6) {
        long long s = 0;
        for (int g = 0; g < G; ++g) s += reinterpret_cast<const long long*>(rows + (size_t)g * W)[tid];
        s_cnt[tid - 3] = s;
    }
    __syncthreads();
    const long long n = s_cnt[0];
    const double inv_n = n > 0 ? 1.0 / (double)n : 0.0;
    double qv[CALIB_UPD_ROWS], nv[CALIB_UPD_ROWS];
    double res = 0.0;
    int unf = 0;
#pragma unroll
    for (int j = 0; j < CALIB_UPD_ROWS; ++j) {
        const int m = tid + j * CALIB_UPD_NT;
        qv[j] = nv[j] = 0.0;
        if (m < M) {
            double q = 0.0;
            unsigned long long k = 0ull;
            for (int g = 0; g < G; ++g) {
                const unsigned long long* row = rows + (size_t)g * W;
                q += reinterpret_cast<const double*>(row)[CALIB_ROW_HEAD + m];
                k += row[CALIB_ROW_HEAD + M + m];
            }
            qv[j] = q, nv[j] = (double)k;
            if (k == 0ull) unf += 1;
            else res = fmax(res, fabs(q - (double)k) * inv_n);
        }
    }
    s_res[tid] = res;
    s_unf[tid] = unf;
    __syncthreads();
    for (int w = CALIB_UPD_NT / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            s_res[tid] = fmax(s_res[tid], s_res[tid + w]);
            s_unf[tid] += s_unf[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool fit_t = (fit & 1) != 0, fit_p = (fit & 2) != 0;
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        int act = 0;
        double kappa = theta[0];
        const int it = first ? 0 : st->iter;
        if (first) {
            st->last = 0, st->lo_known = st->hi_known = st->have_best = 0, st->spare0 = st->spare1 = 0;
            st->lo = kmin, st->hi = kmax;
            st->best_J = st->best_g = st->best_h = st->best_resid = st->xent_start = 0.0;
        }
        const double J = s_sum[0] * inv_n, g = s_sum[1] * inv_n, h = s_sum[2] * inv_n;
        const double resid = fit_p ? s_res[0] : 0.0;
        CalibRec r{0.0, 0.0, 0.0, 0.0, 0.0, n, s_cnt[1], s_cnt[2], it + 1, 0, s_unf[0], 0};
        bool finish = false;
        if (n == 0) {
            r.flags = CALIB_NO_DATA;
            finish = true;
        } else {
            if (it == 0 && fit_t && max_iter > 0 && !(kappa >= kmin && kappa <= kmax)) {
                kappa = kappa > kmax ? kmax : kmin;                                           // a start outside the box (or a NaN) is put on it:
                theta[0] = kappa;                                                             // the fit, and xent_start, begin there
            } else {
                if (!st->have_best) st->xent_start = J;                                       // (the first theta inside the box)
                const bool is_best = !st->have_best || J < st->best_J || st->best_J != st->best_J;
                if (is_best) {
                    st->have_best = 1;
                    st->best_J = J, st->best_g = g, st->best_h = h, st->best_resid = resid;
                    best[0] = kappa;
                    act |= CALIB_DO_SAVE;
                }
                const bool out_min = fit_t && kappa == kmin && g > 0.0, out_max = fit_t && kappa == kmax && g < 0.0;
                const bool temp_ok = !fit_t || fabs(kappa * g) <= tol || out_min || out_max;
                const bool prior_ok = !fit_p || resid <= tol;
                const bool conv = temp_ok && prior_ok;
                if (conv && J <= st->xent_start) {
                    r.flags = CALIB_CONVERGED | (out_min ? CALIB_AT_MIN : 0) | (out_max ? CALIB_AT_MAX : 0);
                    r.xent_end = J, r.g_logk = kappa * g, r.resid_prior = resid, r.curvature = h;
                    finish = true;
                } else if (conv || it >= max_iter) {                                          // the best theta seen, the one with the lowest J
                    const double bk = best[0], bg = st->best_g;
                    r.flags = CALIB_MAX_ITER | (fit_t && bk == kmin && bg > 0.0 ? CALIB_AT_MIN : 0) | (fit_t && bk == kmax && bg < 0.0 ? CALIB_AT_MAX : 0);
                    r.xent_end = st->best_J, r.g_logk = bk * bg, r.resid_prior = st->best_resid, r.curvature = st->best_h;
                    if (!is_best) {
                        act |= CALIB_DO_RESTORE;
                        if (fit_t) theta[0] = bk;
                    }
                    finish = true;
                } else if (fit_t && !temp_ok && (!fit_p || prior_ok || st->last != CALIB_STEP_KAPPA)) {
                    // a Newton step on g, at most a factor 8 in kappa, kept inside the sign bracket: an end whose sign is not known is
                    // the box's and is tried itself, a known one sends the step to the middle of the bracket in log kappa
                    if (g < 0.0) { st->lo = kappa; st->lo_known = 1; } else { st->hi = kappa; st->hi_known = 1; }
                    double cand = h > 0.0 ? kappa - g / h : (g < 0.0 ? inf : -inf);
                    if (!(cand < kappa * 8.0)) cand = kappa * 8.0;
                    if (!(cand > kappa * 0.125)) cand = kappa * 0.125;
                    if (cand >= st->hi) cand = st->hi_known ? sqrt(st->lo * st->hi) : st->hi;
                    else if (cand <= st->lo) cand = st->lo_known ? sqrt(st->lo * st->hi) : st->lo;
                    theta[0] = cand;
                    st->last = CALIB_STEP_KAPPA;
                } else {                                                                      // c moves: the bracket is opened again
                    act |= CALIB_DO_SWEEP;
                    st->last = CALIB_STEP_PRIOR;
                    st->lo = kmin, st->hi = kmax, st->lo_known = st->hi_known = 0;
                }
            }
        }
        st->iter = it + 1;
        st->done = finish ? 1 : 0;
        if (finish) {
            if (n > 0) r.xent_start = st->xent_start;
            *rec = r;
        }
        s_do = act;
    }
    __syncthreads();
    const int act = s_do;
    if (act == 0) return;
#pragma unroll
    for (int j = 0; j < CALIB_UPD_ROWS; ++j) {
        const int m = tid + j * CALIB_UPD_NT;
        if (m >= M) continue;
        if (act & CALIB_DO_SAVE) best[1 + m] = theta[1 + m];
        if (nv[j] == 0.0) continue;                                                           // an unfitted member keeps its bits
        if (act & CALIB_DO_SWEEP) theta[1 + m] += qv[j] > 0.0 ? log(nv[j] / qv[j]) : 700.0;   // (q_m == 0: every own p underflowed)
        if ((act & CALIB_DO_RESTORE) && (fit & 2)) theta[1 + m] = best[1 + m];
    }
}

}  // namespace

size_t calib_scratch_bytes(int M, long long N) {
    return sizeof(CalibState) + sizeof(double) * ((size_t)(1 + M) + (size_t)calib_groups(N) * calib_row_words(M));
}

// The caller (cmps_bank_calibrate) has checked: 1 <= M <= 1024, N >= 1, ld >= N, M ld <= 2^62, fit in [0, 3], tol and the box finite and
// positive, theta, record and scratch 8-byte aligned and the scratch of calib_scratch_bytes(M, N) bytes; no pointer is null.  `first`: the
// first pair of a call, which reads nothing of what the scratch held
hipError_t launch_calib_pass(const float* loss, int M, long long N, long long ld, const int* label, const double* theta, void* scratch,
                             int first, hipStream_t s) {
    hipLaunchKernelGGL(k_calib_pass, dim3(calib_groups(N)), dim3(CALIB_TILE), 0, s, loss, M, N, ld, label, theta,
                       static_cast<unsigned char*>(scratch), first);
    return hipGetLastError();
}

hipError_t launch_calib_update(double* theta, void* record, void* scratch, int M, long long N, int fit, int max_iter, double tol,
                               double kappa_min, double kappa_max, int first, hipStream_t s) {
    hipLaunchKernelGGL(k_calib_update, dim3(1), dim3(CALIB_UPD_NT), 0, s, theta, static_cast<CalibRec*>(record),
                       static_cast<unsigned char*>(scratch), M, calib_groups(N), fit, max_iter, tol, kappa_min, kappa_max, first);
    return hipGetLastError();
}

// The caller (cmps_loss_stats) has checked: B >= 1, first_id >= 0, first_id + B representable, stats 8-byte aligned
hipError_t launch_loss_stats(const float* loss, int B, long long first_id, int reset, void* stats, hipStream_t s) {
    hipLaunchKernelGGL(k_loss_stats, dim3(1), dim3(STATS_NT), 0, s, loss, B, first_id, reset, static_cast<LossStats*>(stats));
    return hipGetLastError();
}

// The caller (cmps_bank_classify_stats) has checked: 1 <= M <= 1024, B >= 1, ld >= B, first_id >= 0, first_id + B representable, stats
// 8-byte aligned and of cmps_bank_classify_stats_bytes(M) bytes; label and best may be null
hipError_t launch_classify_stats(const float* loss, int M, int B, long long ld, const int* label, long long first_id, int reset, void* stats,
                                 int* best, hipStream_t s) {
    hipLaunchKernelGGL(k_classify_stats, dim3(1), dim3(STATS_NT), 0, s, loss, M, B, ld, label, first_id, reset,
                       static_cast<ClassifyHead*>(stats), best);
    return hipGetLastError();
}

// The caller (cmps_bank_classify_weights) has checked: 1 <= M <= 1024, B >= 1, ld >= B, ldw >= B, inv_temp finite and > 0, the two weights
// finite and >= 0, record 8-byte aligned and of 40 bytes; no pointer is null
hipError_t launch_classify_weights(const float* loss, int M, int B, long long ld, const int* label, double inv_temp, double gen_weight,
                                   double disc_weight, int reset, float* weight, long long ldw, void* record, hipStream_t s) {
    hipLaunchKernelGGL(k_classify_weights, dim3(1), dim3(STATS_NT), 0, s, loss, M, B, ld, label, inv_temp, gen_weight, disc_weight, reset,
                       weight, ldw, static_cast<ClassifyWeightsRec*>(record));
    return hipGetLastError();
}

// The caller (cmps_bank_posterior) has checked: 1 <= M <= 1024, n >= 1, steps >= 1, M n steps <= 2^31 - 1, inv_temp finite and > 0,
// log_prior and decision 8-byte aligned, and with a decision: threshold in (0, 1], first_step >= 0, first_step + steps representable;
// every pointer but nll may be null
hipError_t launch_bank_posterior(const float* nll, int M, int n, int steps, const float* total_in, const double* log_prior, double inv_temp,
                                 float* total_out, float* post, int* best, float* conf, double threshold, long long first_step, int reset,
                                 void* decision, hipStream_t s) {
    auto go = [&](auto kernel, int C) -> hipError_t {
        const size_t shm = posterior_lds_bytes(M, C);
        const hipError_t e = lds_attr(kernel, shm);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(n), dim3(POST_NT), shm, s, nll, M, n, steps, total_in, log_prior, inv_temp, total_out, post, best,
                           conf, threshold, first_step, reset, static_cast<BankDecision*>(decision));
        return hipGetLastError();
    };
    // R: the rows of a chunk a thread holds, M <= R POST_NT / C; beyond 256 members a chunk does not fit the registers (R = 0)
    if (M <= 64) return go(k_bank_posterior<64, 8>, 64);
    if (M <= 128) return go(k_bank_posterior<64, 16>, 64);
    if (M <= POSTERIOR_PREFETCH_M) return go(k_bank_posterior<64, 32>, 64);
    if (M <= POSTERIOR_WIDE_M) return go(k_bank_posterior<64, 0>, 64);
    return go(k_bank_posterior<32, 0>, 32);
}

}  // namespace cmps
