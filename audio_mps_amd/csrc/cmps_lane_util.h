// Device primitives every kernel family uses: register vector types, lane exchanges (readlane, DPP, permlane swaps), the LDS progress
// counters of the two-wave hand-overs, packing / scaling of bf16 and fp16 MFMA operands, the workgroup sum.  Each is a few
// instructions, __forceinline__, and exists once: a kernel file defines only what is its own.
#pragma once
#include "cmps_internal.h"

namespace cmps {

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
// eight bf16 values, under the two element types the builtins ask for: __bf16 (v_mfma_f32_32x32x16_bf16 of the D <= 32 kernels' rank-1
// sums) and short (bit patterns: the fragments the D > 32 kernels build with integer instructions)
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ v2f mk2(float a, float b) { v2f r; r.x = a; r.y = b; return r; }
__device__ __forceinline__ v2f lo2(v4f q) { return __builtin_shufflevector(q, q, 0, 1); }
__device__ __forceinline__ v2f hi2(v4f q) { return __builtin_shufflevector(q, q, 2, 3); }

// ---- lane exchanges ----
__device__ __forceinline__ float rdlane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
// lanes l and l ^ 32: lower lanes receive x + x', upper lanes y + y' (the cross-half combine of the split layout, the sum over the two
// clips of a pair)
__device__ __forceinline__ float swap32_add(float x, float y) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// the value the lane 16 away holds (the Re <-> Im partner of the same row and clip): v_permlane16_swap of x with itself leaves
// the even rows' values in r[0] and the odd rows' values in r[1], in both rows of a pair
__device__ __forceinline__ float partner16(float x, bool odd_row) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return odd_row ? __uint_as_float(r[0]) : __uint_as_float(r[1]);
}

__device__ __forceinline__ float rsq_newton(float m) {   // 1 / sqrt(m): v_rsq_f32 + one Newton step
    const float r = __builtin_amdgcn_rsqf(m);
    return r * (1.5f - 0.5f * m * r * r);
}

// ---- progress counters in LDS (the hand-over between the waves of a clip), accessed with explicit DS instructions (a `volatile int*`
// cast would decay to a generic pointer: flat accesses plus a vmcnt(0) wait that also drains the stash stores) ----
__device__ __forceinline__ int flag_load(unsigned addr) {
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ void flag_store(unsigned addr, int v, int lane) {
    if (lane == 0) asm volatile("ds_write_b32 %0, %1" : : "v"(addr), "v"(v) : "memory");
}

// ---- MFMA operands ----
__device__ __forceinline__ unsigned pack_hi16(unsigned lo_word, unsigned hi_word) {   // (lo_word >> 16) | (hi_word & 0xFFFF0000)
    return __builtin_amdgcn_perm(hi_word, lo_word, 0x07060302u);
}
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {                  // round to nearest even, (lo, hi) packed
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ unsigned cvt_pk_f16(float lo, float hi) {                   // round to nearest even, (lo, hi) packed
    unsigned r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// exact three-way bf16 split of two floats (even element in the low half of every packed word)
__device__ __forceinline__ void split3_pk(float fe, float fo, unsigned& H, unsigned& M, unsigned& L) {
    const unsigned xe = __float_as_uint(fe), xo = __float_as_uint(fo);
    H = __builtin_amdgcn_perm(xo, xe, 0x07060302u);
    const float re = fe - __uint_as_float(xe & 0xFFFF0000u), ro = fo - __uint_as_float(xo & 0xFFFF0000u);
    const unsigned me = __float_as_uint(re), mo = __float_as_uint(ro);
    M = __builtin_amdgcn_perm(mo, me, 0x07060302u);
    const float le = re - __uint_as_float(me & 0xFFFF0000u), lo = ro - __uint_as_float(mo & 0xFFFF0000u);
    L = __builtin_amdgcn_perm(__float_as_uint(lo), __float_as_uint(le), 0x07060302u);   // <= 8 bits left: exact
}
// the largest power of two S with bound S < 2^target (bound = m 2^e, 1/2 <= m < 1); exponent clamped so that S and 1 / S are normal
__device__ __forceinline__ float pow2_below(float bound, int target) {
    const int e = (int)((__float_as_uint(bound) >> 23) & 0xFFu) - 126;
    int se = target - e;
    se = se > 60 ? 60 : se < -60 ? -60 : se;
    return __uint_as_float((unsigned)(127 + se) << 23);
}
__device__ __forceinline__ s16x8 xor_bits(s16x8 v, unsigned mask) {                   // `mask` XORed into every word of a fragment
    v4u t = __builtin_bit_cast(v4u, v);
    t = v4u{t.x ^ mask, t.y ^ mask, t.z ^ mask, t.w ^ mask};
    return __builtin_bit_cast(s16x8, t);
}

// Sum over the workgroup, result to every thread; fixed order (deterministic).  Two barriers.
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    constexpr int NW = NT / 64;
    if constexpr (NW == 1) return v;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    __syncthreads();
    return s;
}

}  // namespace

}  // namespace cmps
