// The samplers' Gaussian noise, drawn on the device (cmps_noise_fill; the reference draws it where it samples: tf.random_normal inside
// `sample`, model.py:246 / :88, 96, 106).  The generator is counter-based, so the noise of a step is a pure function of
// (seed, path, step) -- include/cmps.h states the definition, tests/_noise_ref.py restates it in numpy:
//
//   q = s >> 2, r = s & 3;   (x0 .. x3) = Philox4x32-10(counter = (q lo, q hi, path, 0), key = (seed lo, seed hi))
//   pair j in {0, 1}:  u = ((x[2j] >> 8) + 1) 2^-24 in (0, 1],  v = (x[2j+1] >> 8) 2^-23 in [0, 2)       (both exact in float32)
//                      rad = sqrtf(-2 logf(u));  z[2j] = rad cospif(v),  z[2j+1] = rad sinpif(v);         z(seed, path, s) = z[r]
//
// k_noise_philox writes noise[b * length + j] = stddev * z(seed, first_path + b, first_step + j): one thread per quad q of one path (one
// Philox call, four normals), grid-stride over the paths.  A quad wholly inside the row whose destination is 16-byte aligned leaves as
// one 16-byte store, any other quad (the first and last of a row, a row whose base is not aligned, first_step not a multiple of 4)
// element by element.  Nothing is read from memory; no LDS, no cross-lane traffic.
#include "cmps_internal.h"
#include "cmps_philox.h"

namespace cmps {

namespace {

constexpr int NOISE_NT = 256;

// the pair (rad cospif(v), rad sinpif(v)) of two Philox words: the accurate logf / sqrtf / cospif / sinpif (near u -> 1 the result is the
// small difference a fast logarithm gets wrong); u > 0, so neither Inf nor NaN arises and |z| <= sqrt(48 ln 2)
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& z0, float& z1) {
    const float u = (float)((xa >> 8) + 1u) * 0x1p-24f;
    const float v = (float)(xb >> 8) * 0x1p-23f;
    const float rad = sqrtf(-2.0f * logf(u));
    z0 = rad * cospif(v);
    z1 = rad * sinpif(v);
}

// nq = quads a row touches, q_lo = first_step >> 2.  grid (ceil(nq / NOISE_NT), paths in flight)
__global__ __launch_bounds__(NOISE_NT) void k_noise_philox(uint32_t key0, uint32_t key1, unsigned long long first_step, unsigned long long q_lo,
                                                           long long nq, uint32_t first_path, int n, int length, float stddev,
                                                           float* __restrict__ noise) {
    const long long qi = (long long)blockIdx.x * NOISE_NT + threadIdx.x;
    if (qi >= nq) return;
    const unsigned long long q = q_lo + (unsigned long long)qi;
    const long long j0 = (long long)((q << 2) - first_step);          // the row index of the quad's first normal: -3 .. length - 1
    const bool whole = j0 >= 0 && j0 + 3 < (long long)length;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        uint32_t x[4];
        philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), first_path + (uint32_t)b, 0u, key0, key1, x);
        float z[4];
        box_muller(x[0], x[1], z[0], z[1]);
        box_muller(x[2], x[3], z[2], z[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = stddev * z[r];
        float* row = noise + (size_t)b * (size_t)length;
        if (whole && (reinterpret_cast<uintptr_t>(row + j0) & 15) == 0) {
            *reinterpret_cast<float4*>(row + j0) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long j = j0 + r;
                if (j >= 0 && j < (long long)length) row[j] = z[r];
            }
        }
    }
}

}  // namespace

// The caller (cmps_noise_fill) has checked: n >= 1, length >= 1, first_path + n <= 2^32, first_step + length <= 2^64
hipError_t launch_noise_philox(unsigned long long seed, unsigned long long first_step, unsigned first_path, int n, int length, float stddev,
                               float* noise, hipStream_t s) {
    const unsigned long long q_lo = first_step >> 2, q_hi = (first_step + (unsigned long long)(length - 1)) >> 2;
    const long long nq = (long long)(q_hi - q_lo) + 1;                  // <= length / 4 + 2
    const long long gx = (nq + NOISE_NT - 1) / NOISE_NT;
    long long gy = n < 65535 ? n : 65535;
    if (gx * gy > (1ll << 22)) gy = (1ll << 22) / gx > 1 ? (1ll << 22) / gx : 1;   // the rest of the paths by the kernel's stride
    hipLaunchKernelGGL(k_noise_philox, dim3((unsigned)gx, (unsigned)gy), dim3(NOISE_NT), 0, s, (uint32_t)seed, (uint32_t)(seed >> 32), first_step,
                       q_lo, nq, (uint32_t)first_path, n, length, stddev, noise);
    return hipGetLastError();
}

}  // namespace cmps
