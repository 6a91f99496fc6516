// What the workgroup-per-clip, correctness-first kernels share (cmps_block.hip, cmps_legacy.hip, cmps_rho.hip: the independent
// implementation the fast kernels are tested against): the prefetching two-matrix row loop, the owner-computes iteration over the
// D x D gradient elements and its slab write-out, the loss sum of the finalize kernels, the phase of one frequency.  Everything is
// __forceinline__: a kernel that calls these compiles to what it compiled to with the text written out.
#pragma once
#include "cmps_lane_util.h"

namespace cmps {

namespace {

constexpr int JLOOP_ROWS = 8;      // matrix rows fetched ahead per block

// body(j, M1[j][t], M2[j][t]) for j = 0 .. D-1 in order, the matrix elements (L2 resident: three D x D tables do not fit L1 above
// D = 32) fetched a block of JLOOP_ROWS rows ahead of their use: one L2 round trip per block instead of one per row
template <class Body>
__device__ __forceinline__ void jloop2(const float2* __restrict__ M1, const float2* __restrict__ M2, int D, int DP, int t, Body body) {
    constexpr int JB = JLOOP_ROWS;
    float2 n1[JB], n2[JB];
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
        const int j = jj < D ? jj : D - 1;
        n1[jj] = M1[j * DP + t];
        n2[jj] = M2[j * DP + t];
    }
    for (int j0 = 0; j0 < D; j0 += JB) {
        float2 c1[JB], c2[JB];
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) { c1[jj] = n1[jj]; c2[jj] = n2[jj]; }
        if (j0 + JB < D) {
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) {
                int j = j0 + JB + jj;
                j = j < D ? j : D - 1;
                n1[jj] = M1[j * DP + t];
                n2[jj] = M2[j * DP + t];
            }
        }
        if (j0 + JB <= D) {
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) body(j0 + jj, c1[jj], c2[jj]);
        } else {
#pragma unroll
            for (int jj = 0; jj < JB; ++jj)
                if (j0 + jj < D) body(j0 + jj, c1[jj], c2[jj]);
        }
    }
}

// Owner computes: thread t of NT owns the elements idx = t + m NT (m < EPT) of a D x D matrix, row-major; body(m, i, j) for every
// owned element (i, j), m being the index of its register accumulator.  NT * EPT >= D * D is the launchers' business.
template <int NT, int EPT, class Body>
__device__ __forceinline__ void for_owned(int D, Body body) {
    const int t = threadIdx.x;
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
        const int idx = t + m * NT;
        if (idx < D * D) {
            const int i = idx / D, j = idx % D;
            body(m, i, j);
        }
    }
}

// the owned elements of Rbar and Qbar into the four planes of a slab: Rbar_re | Rbar_im | Qbar_re | Qbar_im, each [DP][DP]
// (DD = DP * DP) row-major.  The caller has zeroed the planes (the padding stays zero).
template <int NT, int EPT>
__device__ __forceinline__ void store_rq_planes(float* slab, int DD, int D, int DP, const float2 (&Rb)[EPT], const float2 (&Qb)[EPT]) {
    for_owned<NT, EPT>(D, [&](int m, int i, int j) {
        const int o = i * DP + j;
        slab[o] = Rb[m].x;
        slab[DD + o] = Rb[m].y;
        slab[2 * DD + o] = Qb[m].x;
        slab[3 * DD + o] = Qb[m].y;
    });
}

// sum_b loss_b in double by lanes 0 .. 63 of one wave (threadIdx.x < 64): strided partials, then a fixed-order tree; valid in lane 0
__device__ __forceinline__ double loss_sum_wave(const float* loss, int B) {
    double ls = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) ls += (double)loss[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ls += __shfl_xor(ls, off, 64);
    return ls;
}

// exp(i fl(freq t)) as (cos, sin): the lab-frame phase of one component (model.py:305)
__device__ __forceinline__ float2 phase(float freq, float t) {
    const float th = __fmul_rn(freq, t);
    float sn, cs;
    sincosf(th, &sn, &cs);
    return make_float2(cs, sn);
}

}  // namespace

}  // namespace cmps
