// The input of a training step, produced where it is used (include/cmps.h states both contracts; tests/_data_ref.py restates them in numpy).
//
// k_batch_gather (cmps_batch_gather; the reference's audio_dataset.batch(...) -> get_next(), data.py:37-43, for a dataset that is already in
// device memory):  audio[b * T + j] = data[index[b] * clip_len + offset[b] + j].  A copy at memory bandwidth: block (x, y) handles chunk x
// (GATHER_CHUNK quads = 16 KB) of the rows y, y + gridDim.y, ...  A row is cut on its DESTINATION: `head` elements up to the first 16-byte
// boundary of the row, then whole quads, then the tail; quads leave as one 16-byte store each, head and tail element by element.  The source
// of a quad sits wherever index, offset and head put it, so in general it is only 4-byte aligned.  LOAD FORM: one 16-byte load per quad at
// 4-byte alignment (a float4 whose type says aligned(4): gfx950's global memory path takes a dwordx4 at any dword address, and the lanes of a
// wave still cover one contiguous 1 KiB) -- not four dword loads, which would issue four times the instructions for the same bytes, and not
// a staging pass through LDS, which a straight copy has no use for.  All of a thread's loads are issued before its first store.
// A row whose index or offset is out of range is written as quiet NaNs and nothing is read for it.
//
// k_batch_gather_i16 (cmps_batch_gather_i16): the same gather out of a dataset held as int16 (16-bit PCM), widened on the way:
// audio[b * T + j] = (float)data[index[b] * clip_len + offset[b] + j] * scale -- an exact conversion and one float32 multiply.  Grid, row
// guard and the destination-side cut (head, 16-byte stores, tail) are k_batch_gather's; a quad of outputs is 8 source bytes at an address
// that is only 2-byte aligned.  LOAD FORM: naturally aligned loads only.  With a = the quad's byte address and sh = a & 2 (the same for
// every quad of a row, since quads are 8 bytes apart), one 8-byte load at the dword address a - sh, and where sh = 2 one more dword behind it;
// the three dwords are then shifted right by 8 * sh bits (plain 64-bit shifts, which the compiler turns into its funnel shift).  Not a wide
// load at a 2-byte address: whether gfx950's global path takes one depends on the alignment mode the driver configured, which this library
// does not control, while a dwordx2 at a dword address is the form k_batch_gather already relies on.  Head and tail go element by element
// (2-byte loads).  READS: of a valid row only its T samples, except that where sh = 2 the first quad's load starts 2 bytes before its
// first sample and the last quad's extra dword ends 2 bytes behind its last -- the aligned dwords that hold those samples, inside the
// buffer everywhere but at its two ends.  There every dword is checked against [data, data + n_clips * clip_len): a dword that would cross
// an end of the buffer is read as its one 2-byte half that lies inside, so not a byte outside the buffer is ever touched.
//
// k_damped_sine (cmps_damped_sine_fill; the reference's synthetic batch, data.py:8-22): clip c = first_clip + b draws its Gamma(2) delay
// from ONE Philox call (counter word 3 = 1: apart from the noise's draws), hoisted out of the sample loop; a thread then evaluates quads of
// samples, grid-strided along the row, and stores a quad as 16 bytes where the row base is 16-byte aligned, element by element otherwise.
// Nothing is read from memory; no LDS, no cross-lane traffic.
#include "cmps_internal.h"
#include "cmps_philox.h"

namespace cmps {

namespace {

constexpr int DATA_NT = 256;
constexpr int GATHER_PASSES = 4;                            // quads per thread and chunk
constexpr int GATHER_CHUNK = DATA_NT * GATHER_PASSES;       // quads per chunk
constexpr int GATHER_BLOCKS = 2048;                         // about eight blocks per CU; the rest of the rows by the kernel's stride

typedef float quad_a4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at 4-byte alignment: the load form above

// grid (chunks, rows in flight); chunks = ceil((T / 4) / GATHER_CHUNK), at least 1
__global__ __launch_bounds__(DATA_NT) void k_batch_gather(const float* __restrict__ data, long long n_clips, long long clip_len,
                                                          const int* __restrict__ index, const int* __restrict__ offset, int B, int T,
                                                          float* __restrict__ audio) {
    const int tid = threadIdx.x, c = blockIdx.x;
    const bool last = c == (int)gridDim.x - 1;
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long long idx = index[b], off = offset ? (long long)offset[b] : 0ll;
        const bool ok = idx >= 0 && idx < n_clips && off >= 0 && off <= clip_len - (long long)T;
        const float* src = data + (ok ? idx * clip_len + off : 0ll);               // (dereferenced only where ok)
        float* dst = audio + (size_t)b * (size_t)T;
        const int to_boundary = (4 - (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3;
        const int head = to_boundary < T ? to_boundary : T;
        const int nq = (T - head) >> 2, tail0 = head + 4 * nq;                      // quads; the first element behind them
        if (c == 0 && tid < head) dst[tid] = ok ? src[tid] : qnan;
        if (last && tid < T - tail0) dst[tail0 + tid] = ok ? src[tail0 + tid] : qnan;
        const int q0 = c * GATHER_CHUNK + tid;
        quad_a4 v[GATHER_PASSES];
#pragma unroll
        for (int p = 0; p < GATHER_PASSES; ++p) {
            const int q = q0 + p * DATA_NT;
            v[p] = quad_a4{qnan, qnan, qnan, qnan};
            if (ok && q < nq) v[p] = *reinterpret_cast<const quad_a4*>(src + head + 4 * (long long)q);
        }
#pragma unroll
        for (int p = 0; p < GATHER_PASSES; ++p) {
            const int q = q0 + p * DATA_NT;
            if (q < nq) *reinterpret_cast<float4*>(dst + head + 4 * (long long)q) = make_float4(v[p].x, v[p].y, v[p].z, v[p].w);
        }
    }
}

typedef uint32_t pair_a4 __attribute__((ext_vector_type(2), aligned(4)));   // 8 bytes at 4-byte alignment

// The dword at the 4-byte aligned address p, read only where it lies in [lo, hi) (2-byte granules; what lies outside reads as zero)
__device__ __forceinline__ uint32_t load_dword_inside(const char* p, const char* lo, const char* hi) {
    if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
    if (p >= lo && p + 2 <= hi) v = *reinterpret_cast<const uint16_t*>(p);
    if (p + 2 >= lo && p + 4 <= hi) v |= (uint32_t)*reinterpret_cast<const uint16_t*>(p + 2) << 16;
    return v;
}

// grid as k_batch_gather
__global__ __launch_bounds__(DATA_NT) void k_batch_gather_i16(const short* __restrict__ data, long long n_clips, long long clip_len,
                                                              const int* __restrict__ index, const int* __restrict__ offset, int B, int T,
                                                              float scale, float* __restrict__ audio) {
    const int tid = threadIdx.x, c = blockIdx.x;
    const bool last = c == (int)gridDim.x - 1;
    const float qnan = __uint_as_float(0x7fc00000u);
    const char* const lo = reinterpret_cast<const char*>(data);
    const char* const hi = lo + 2 * n_clips * clip_len;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long long idx = index[b], off = offset ? (long long)offset[b] : 0ll;
        const bool ok = idx >= 0 && idx < n_clips && off >= 0 && off <= clip_len - (long long)T;
        const short* src = data + (ok ? idx * clip_len + off : 0ll);               // (dereferenced only where ok)
        float* dst = audio + (size_t)b * (size_t)T;
        const int to_boundary = (4 - (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3;
        const int head = to_boundary < T ? to_boundary : T;
        const int nq = (T - head) >> 2, tail0 = head + 4 * nq;                      // quads; the first element behind them
        if (c == 0 && tid < head) dst[tid] = ok ? (float)src[tid] * scale : qnan;
        if (last && tid < T - tail0) dst[tail0 + tid] = ok ? (float)src[tail0 + tid] * scale : qnan;
        const char* q_base = reinterpret_cast<const char*>(src + head);            // the first quad's source: 2-byte aligned
        const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(q_base) & 2);
        q_base -= sh;                                                               // ... and the dword that holds its first sample
        const int q0 = c * GATHER_CHUNK + tid;
        uint32_t w[GATHER_PASSES][3];
#pragma unroll
        for (int p = 0; p < GATHER_PASSES; ++p) {
            const int q = q0 + p * DATA_NT;
            w[p][0] = w[p][1] = w[p][2] = 0u;
            if (ok && q < nq) {
                const char* a = q_base + 8 * (long long)q;
                if (a >= lo && a + 8 <= hi) {
                    const pair_a4 v = *reinterpret_cast<const pair_a4*>(a);
                    w[p][0] = v.x; w[p][1] = v.y;
                } else {                                                            // (an end of the buffer)
                    w[p][0] = load_dword_inside(a, lo, hi);
                    w[p][1] = load_dword_inside(a + 4, lo, hi);
                }
                if (sh) w[p][2] = load_dword_inside(a + 8, lo, hi);
            }
        }
#pragma unroll
        for (int p = 0; p < GATHER_PASSES; ++p) {
            const int q = q0 + p * DATA_NT;
            if (q < nq) {
                const uint32_t x0 = (uint32_t)((((uint64_t)w[p][1] << 32) | w[p][0]) >> (8 * sh));
                const uint32_t x1 = (uint32_t)((((uint64_t)w[p][2] << 32) | w[p][1]) >> (8 * sh));
                float4 v = make_float4(qnan, qnan, qnan, qnan);
                if (ok) v = make_float4((float)(short)(x0 & 0xffffu) * scale, (float)((int)x0 >> 16) * scale,
                                        (float)(short)(x1 & 0xffffu) * scale, (float)((int)x1 >> 16) * scale);
                *reinterpret_cast<float4*>(dst + head + 4 * (long long)q) = v;
            }
        }
    }
}

// One sample of the clip, in the operation order include/cmps.h fixes (no contraction: there is no a * b + c in it, and none may be made)
__device__ __forceinline__ float damped_sine_at(int j, float delay, float dt) {
#pragma clang fp contract(off)
    const float w = (float)(2.0 * 3.14159265358979323846 * 261.6);                 // fl32(2 pi 261.6)
    const float t = ((float)j - delay) * dt;
    const float sign = t > 0.0f ? 1.0f : (t < 0.0f ? -1.0f : 0.0f);
    return ((0.5f * (sign + 1.0f)) * sinf(w * t)) * expf(-t / 0.1f);
}

// grid (blocks along a row, rows in flight); half_delay = fl32(T / 200.0), dt = fl32(delta_t)
__global__ __launch_bounds__(DATA_NT) void k_damped_sine(uint32_t key0, uint32_t key1, unsigned long long first_clip, int B, int T,
                                                         float half_delay, float dt, float* __restrict__ audio) {
    const int step = 4 * DATA_NT * (int)gridDim.x;                                  // T <= 2^24 and at most 64 blocks: no overflow
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const unsigned long long clip = first_clip + (unsigned long long)b;
        uint32_t x[4];
        philox4x32_10((uint32_t)clip, (uint32_t)(clip >> 32), 0u, 1u, key0, key1, x);
        const float u0 = (float)((x[0] >> 8) + 1u) * 0x1p-24f, u1 = (float)((x[1] >> 8) + 1u) * 0x1p-24f;
        const float delay = half_delay * (-(logf(u0) + logf(u1)));
        float* row = audio + (size_t)b * (size_t)T;
        const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
        for (int j0 = 4 * ((int)blockIdx.x * DATA_NT + (int)threadIdx.x); j0 < T; j0 += step) {
            if (aligned && j0 + 3 < T) {
                *reinterpret_cast<float4*>(row + j0) = make_float4(damped_sine_at(j0, delay, dt), damped_sine_at(j0 + 1, delay, dt),
                                                                   damped_sine_at(j0 + 2, delay, dt), damped_sine_at(j0 + 3, delay, dt));
            } else {
                for (int j = j0; j < j0 + 4 && j < T; ++j) row[j] = damped_sine_at(j, delay, dt);
            }
        }
    }
}

}  // namespace

// (chunks, rows in flight) of both gathers
static dim3 gather_grid(int B, int T) {
    const int quads = T / 4;
    const int gx = quads > GATHER_CHUNK ? (quads + GATHER_CHUNK - 1) / GATHER_CHUNK : 1;
    int gy = GATHER_BLOCKS / gx > 1 ? GATHER_BLOCKS / gx : 1;
    if (gy > B) gy = B;
    return dim3((unsigned)gx, (unsigned)gy);
}

// The caller (cmps_batch_gather) has checked: B >= 1, T >= 1, 1 <= n_clips < 2^31, clip_len >= T
hipError_t launch_batch_gather(const float* data, long long n_clips, long long clip_len, const int* index, const int* offset, int B, int T,
                               float* audio, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_gather, gather_grid(B, T), dim3(DATA_NT), 0, s, data, n_clips, clip_len, index, offset, B, T, audio);
    return hipGetLastError();
}

// The caller (cmps_batch_gather_i16) has checked the same, and scale finite and positive
hipError_t launch_batch_gather_i16(const short* data, long long n_clips, long long clip_len, const int* index, const int* offset, int B, int T,
                                   float scale, float* audio, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_gather_i16, gather_grid(B, T), dim3(DATA_NT), 0, s, data, n_clips, clip_len, index, offset, B, T, scale, audio);
    return hipGetLastError();
}

// The caller (cmps_damped_sine_fill) has checked: B >= 1, 1 <= T <= 2^24, delta_t finite and positive, first_clip + B <= 2^64 - 1
hipError_t launch_damped_sine(unsigned long long seed, unsigned long long first_clip, int B, int T, double delta_t, float* audio, hipStream_t s) {
    const int quads = (T + 3) / 4;
    int gx = (quads + DATA_NT - 1) / DATA_NT;
    if (gx > 64) gx = 64;
    const int gy = B < 65535 ? B : 65535;
    hipLaunchKernelGGL(k_damped_sine, dim3((unsigned)gx, (unsigned)gy), dim3(DATA_NT), 0, s, (uint32_t)seed, (uint32_t)(seed >> 32), first_clip, B, T,
                       (float)((double)T / 200.0), (float)delta_t, audio);
    return hipGetLastError();
}

}  // namespace cmps
