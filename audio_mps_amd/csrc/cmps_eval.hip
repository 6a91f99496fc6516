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
// k_classify_weights (cmps_bank_classify_weights), last: the same losses turned into the per-clip, per-member cotangents of a cross-entropy step.
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

}  // namespace

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

}  // namespace cmps
