// Parameter-derived tables, rebuilt once per optimiser step (everything here is batch-independent).
// Reference lines: model.py:16,266,281 (float32 time accumulation), :304-305 (phases), :308 (adjoint),
// :312 (-delta_t sigma^2 / 2), :41-42 (complex R).
#include "cmps_internal.h"

namespace cmps {

// A bank (cmps_bank_set_params_dev) builds every member's tables in one launch: member = blockIdx.y, whose workspace lies `ws` bytes
// and whose parameters `par` floats behind its predecessor's.  A plain launch has one member and both strides 0.

// t_0 = 0; t_{k+1} = fl32(t_k + dt), strictly sequential (one lane).  dtk[k] = t_k - t_{k+1} is exact.
__global__ void k_ttable(float dt, int N, float* __restrict__ ttab, float* __restrict__ dtk, size_t ws) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    ttab = bank_shift(ttab, blockIdx.y * ws); dtk = bank_shift(dtk, blockIdx.y * ws);
    float t = 0.0f;
    for (int k = 0; k <= N; ++k) {
        ttab[k] = t;
        float tn = __fadd_rn(t, dt);
        if (k < N) dtk[k] = __fsub_rn(t, tn);
        t = tn;
    }
    for (int k = N; k < N + 64; ++k) dtk[k] = 0.0f;  // padding read by the wave kernel's chunked loads
}

// Pack R, R^T, psi0, freqs into DP-strided, zero-padded tables; Q = c_half * R^dagger R (fp64 accumulate,
// rounded once).
__global__ void k_pack(int D, int DP, const float* __restrict__ R_re, const float* __restrict__ R_im,
                       const float* __restrict__ freqs, const float* __restrict__ psi0_re,
                       const float* __restrict__ psi0_im, float c_half, float2* __restrict__ R,
                       float2* __restrict__ RT, float2* __restrict__ Q, float2* __restrict__ psi0,
                       float* __restrict__ freqs_out, size_t ws, size_t par) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    {
        const size_t po = blockIdx.y * par, wo = blockIdx.y * ws;
        R_re += po; R_im += po; freqs += po; psi0_re += po; psi0_im += po;
        R = bank_shift(R, wo); RT = bank_shift(RT, wo); Q = bank_shift(Q, wo); psi0 = bank_shift(psi0, wo); freqs_out = bank_shift(freqs_out, wo);
    }
    if (idx < DP * DP) {
        const int i = idx / DP, j = idx % DP;
        float2 r = make_float2(0.f, 0.f), rt = make_float2(0.f, 0.f), q = make_float2(0.f, 0.f);
        if (i < D && j < D) {
            r = make_float2(R_re[i * D + j], R_im[i * D + j]);
            rt = make_float2(R_re[j * D + i], R_im[j * D + i]);
            double qr = 0.0, qi = 0.0;  // (R^dagger R)[i][j] = sum_k conj(R[k][i]) R[k][j]
            for (int k = 0; k < D; ++k) {
                const double ar = R_re[k * D + i], ai = -(double)R_im[k * D + i];
                const double br = R_re[k * D + j], bi = R_im[k * D + j];
                qr += ar * br - ai * bi;
                qi += ar * bi + ai * br;
            }
            q = make_float2((float)((double)c_half * qr), (float)((double)c_half * qi));
        }
        R[idx] = r;
        RT[idx] = rt;
        Q[idx] = q;
    }
    if (idx < DP) {
        const bool in = idx < D;
        psi0[idx] = in ? make_float2(psi0_re[idx], psi0_im[idx]) : make_float2(0.f, 0.f);
        freqs_out[idx] = in ? freqs[idx] : 0.f;
    }
}

// rho_k[d] = phi_k[d] * conj(phi_{k+1}[d]) with phi_k[d] = exp(i * fl32(f_d * t_k))  (model.py:305: the
// argument of the exponential is the float32 product).  The two float32 angles are subtracted exactly in
// double, the rotation is evaluated in double and rounded once to float32.
//
// Rounding rho_k to float32 leaves a phase (and modulus) error of ~3e-8 per step.  In the reference the state
// lives in the lab frame and is re-expressed with phases_k at every step, so table errors telescope; in the
// rotating frame used here they would accumulate as a random walk over the clip (~4e-6 rad after 16000 steps),
// which measurably shifts the log-likelihood (~1.5e-5 relative, the same for every clip).  So the table is
// built with error feedback at chunk granularity: the LAST entry of every 64-step chunk is replaced by
// fl32(target / actual), where actual is the exact (double) product of the float32 entries so far and target
// is exp(-i fl32(f t_{k+1})), making the accumulated rotation exact at every chunk boundary.
//
// pass 1: one thread per (chunk, d): raw entries, the exact product of the chunk's entries but the last,
//         and the target accumulated rotation at the end of the chunk.
__global__ void k_rho_raw(int D, int DP, int N, const float* __restrict__ freqs, const float* __restrict__ ttab,
                          float2* __restrict__ rho, double2* __restrict__ prod, double2* __restrict__ target, size_t ws) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    {
        const size_t wo = blockIdx.y * ws;
        freqs = bank_shift(freqs, wo); ttab = bank_shift(ttab, wo); rho = bank_shift(rho, wo); prod = bank_shift(prod, wo); target = bank_shift(target, wo);
    }
    const int NC = (N + 63) / 64;
    if (idx >= NC * DP) return;
    const int c = idx / DP, d = idx % DP;
    const int k0 = c * 64, k1 = (k0 + 64 < N ? k0 + 64 : N);     // steps [k0, k1)
    double pr = 1.0, pi = 0.0;
    const float f = d < D ? freqs[d] : 0.f;
    for (int k = k0; k < k1; ++k) {
        float2 out = make_float2(1.f, 0.f);
        if (d < D) {
            const float th0 = __fmul_rn(f, ttab[k]);
            const float th1 = __fmul_rn(f, ttab[k + 1]);
            double sn, cs;
            sincos((double)th0 - (double)th1, &sn, &cs);
            out = make_float2((float)cs, (float)sn);
        }
        rho[(size_t)k * DP + d] = out;
        if (k < k1 - 1) {
            const double nr = pr * (double)out.x - pi * (double)out.y;
            pi = pr * (double)out.y + pi * (double)out.x;
            pr = nr;
        }
    }
    if (c == NC - 1) rho[(size_t)N * DP + d] = make_float2(1.f, 0.f);   // row N: padding read by prefetches
    prod[idx] = make_double2(pr, pi);
    double sn = 0.0, cs = 1.0;
    if (d < D) sincos(-(double)__fmul_rn(f, ttab[k1]), &sn, &cs);
    target[idx] = make_double2(cs, sn);
}
// pass 2: one thread per d, sequential over chunks (a few hundred iterations of double arithmetic).
__global__ void k_rho_fix(int DP, int N, float2* __restrict__ rho, const double2* __restrict__ prod,
                          const double2* __restrict__ target, size_t ws) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    rho = bank_shift(rho, blockIdx.y * ws); prod = bank_shift(prod, blockIdx.y * ws); target = bank_shift(target, blockIdx.y * ws);
    if (d >= DP) return;
    const int NC = (N + 63) / 64;
    double ar = 1.0, ai = 0.0;   // exact accumulated rotation of the float32 table so far
    // The loop is serial (the rounding of every chunk's last entry feeds the next) and its arithmetic is short: with the next chunk's inputs
    // fetched one iteration ahead it ran at the memory latency, 250 x 0.3 us = 74 us inside every optimiser step at C3.  Four chunks'
    // inputs are now in flight ahead of the four being worked on.
    constexpr int PF = 4;
    double2 pq[PF], tq[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) {
        const int cc = j < NC ? j : NC - 1;
        pq[j] = prod[cc * DP + d]; tq[j] = target[cc * DP + d];
    }
    for (int c0 = 0; c0 < NC; c0 += PF) {
        double2 pn[PF], tn[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int cc = c0 + PF + j < NC ? c0 + PF + j : NC - 1;
            pn[j] = prod[cc * DP + d]; tn[j] = target[cc * DP + d];
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int c = c0 + j;
            if (c < NC) {
                const double2 p = pq[j], t = tq[j];
                const int klast = (c * 64 + 64 < N ? c * 64 + 64 : N) - 1;
                const double br = ar * p.x - ai * p.y, bi = ar * p.y + ai * p.x;     // before the chunk's last entry
                const double den = br * br + bi * bi;
                const double lr = (t.x * br + t.y * bi) / den, li = (t.y * br - t.x * bi) / den;   // target / actual
                const float2 last = make_float2((float)lr, (float)li);
                rho[(size_t)klast * DP + d] = last;
                ar = br * (double)last.x - bi * (double)last.y;
                ai = br * (double)last.y + bi * (double)last.x;
            }
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) { pq[j] = pn[j]; tq[j] = tn[j]; }
    }
}

// |Q|_F <= 2^-19 ?  Decided ONCE per parameter set, here; both chain kernels of the wide family (k_fwd_chain16 / k_bwd_chain16 have an
// instance for either case) read the word.  Rounds 4's kernels each recomputed the norm in their prologue and compared it with the
// threshold themselves: two separately compiled sums at a boundary can disagree, and then both instances run, or neither.
__global__ void k_qflag(int DP, const float2* __restrict__ Q, unsigned* __restrict__ flag, size_t ws) {
    Q = bank_shift(Q, blockIdx.y * ws); flag = bank_shift(flag, blockIdx.y * ws);
    __shared__ double red[4];
    double f = 0.0;
    for (int idx = threadIdx.x; idx < DP * DP; idx += 256) f += (double)Q[idx].x * Q[idx].x + (double)Q[idx].y * Q[idx].y;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) f += __shfl_xor(f, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) flag[0] = sqrt(red[0] + red[1] + red[2] + red[3]) <= 1.9073486328125e-6 ? 1u : 0u;   // 2^-19
}

hipError_t launch_prep(const Dev& P, const float* R_re, const float* R_im, const float* freqs,
                       const float* psi0_re, const float* psi0_im, float dt, bool rebuild_ttab,
                       float* ttab, float* dtk, float2* R, float2* RT, float2* Q, float2* psi0,
                       float* freqs_out, float2* rho, double2* rfix, hipStream_t s, int M, size_t par) {
    const size_t ws = P.bank_stride;
    if (rebuild_ttab) hipLaunchKernelGGL(k_ttable, dim3(1, M), dim3(64), 0, s, dt, P.N, ttab, dtk, ws);
    const int n = P.DP * P.DP;
    hipLaunchKernelGGL(k_pack, dim3((n + 255) / 256, M), dim3(256), 0, s, P.D, P.DP, R_re, R_im, freqs,
                       psi0_re, psi0_im, P.c_half, R, RT, Q, psi0, freqs_out, ws, par);
    if (P.D > 32 && P.qflag)
        hipLaunchKernelGGL(k_qflag, dim3(1, M), dim3(256), 0, s, P.DP, (const float2*)Q, const_cast<unsigned*>(P.qflag), ws);
    const int NC = (P.N + 63) / 64;
    const int m = NC * P.DP;
    double2* prod = rfix;
    double2* target = rfix + m;
    hipLaunchKernelGGL(k_rho_raw, dim3((unsigned)((m + 63) / 64), M), dim3(64), 0, s, P.D, P.DP, P.N,
                       (const float*)freqs_out, (const float*)ttab, rho, prod, target, ws);
    hipLaunchKernelGGL(k_rho_fix, dim3((unsigned)((P.DP + 63) / 64), M), dim3(64), 0, s, P.DP, P.N, rho,
                       (const double2*)prod, (const double2*)target, ws);
    return hipGetLastError();
}

}  // namespace cmps
