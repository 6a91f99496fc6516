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

}  // namespace

// The caller (cmps_loss_stats) has checked: B >= 1, first_id >= 0, first_id + B representable, stats 8-byte aligned
hipError_t launch_loss_stats(const float* loss, int B, long long first_id, int reset, void* stats, hipStream_t s) {
    hipLaunchKernelGGL(k_loss_stats, dim3(1), dim3(STATS_NT), 0, s, loss, B, first_id, reset, static_cast<LossStats*>(stats));
    return hipGetLastError();
}

}  // namespace cmps
