// Philox4x32-10, the counter-based generator behind everything the library draws on the device: the samplers' normals (cmps_noise.hip,
// counter word 3 = 0) and the delays of the synthetic training clips (cmps_data.hip, counter word 3 = 1).  include/cmps.h states the rounds
// and three known answers; tests/_noise_ref.py restates them in numpy.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace cmps {

// Philox4x32-10 in the Random123 form: ten rounds, the key bumped before every round but the first
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t x[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t hi0 = __umulhi(M0, c0), hi1 = __umulhi(M1, c2);
#else
        const uint32_t hi0 = (uint32_t)(((uint64_t)M0 * c0) >> 32), hi1 = (uint32_t)(((uint64_t)M1 * c2) >> 32);
#endif
        const uint32_t lo0 = M0 * c0, lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

}  // namespace cmps
