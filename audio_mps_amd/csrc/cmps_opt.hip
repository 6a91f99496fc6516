// Device-resident optimiser step: the chain rule from the reduced effective-parameter gradient sums back to
// the raw variables -- adjoint of model.py:36-42 (rsqrt(reg) scaling + the row-broadcast diagonal removal), :49, :221-222 --
// the regularisers of train.py:55-60, tf.train.AdamOptimizer (train.py:89; beta1 0.9, beta2 0.999, eps 1e-8 from
// logging/graph.pbtxt:32102-32192) and the next step's effective parameters (model.py:36-42, 49, 221-222), all in ONE
// workgroup on the caller's stream: a training step then has no device -> host synchronisation and no host arithmetic.
// The host implementation (audio_mps_amd/model.py::chain_rule, train.py::AdamOptimizer) stays the tested reference for it:
// the chain rule is evaluated in double like numpy's, Adam in float32 with numpy's rounding points (no contraction).
//
//   vars / adam_m / adam_v : [A | Rx D^2 | Ry D^2 | freqs D | psi_x D | psi_y D]           (2 D^2 + 3 D + 1 floats)
//   grad_sums              : what cmps_psi_loss_bwd writes (sums over clips)                 (2 D^2 + 3 D + 2 floats)
//   params_out             : [R_re D^2 | R_im D^2 | freqs D | psi0_re D | psi0_im D | A]    (input of cmps_set_params_dev)
//   losses_out             : [mean_b loss_b, total loss (with regularisers)]
//
// k_rho_apply_step is the same step for RhoCMPS (model.py:119-132 in place of :221-222; host reference RhoCMPS.chain_rule / columns):
//   vars / adam_m / adam_v : [A | Rx D^2 | Ry D^2 | freqs D | Wx rank D | Wy rank D]         (2 D^2 + D + 1 + 2 rank D floats)
//   grad_sums              : what cmps_rho_loss_bwd writes: the layout above + [phibar_re rank D | phibar_im rank D]
//   params_out             : as above, the psi_0 slot = e_0;   phi_out : [phi_re rank D | phi_im rank D] (input of cmps_rho_set_state)
// What the two kernels share (effective R, regulariser sums, column sums, c_r / c_h scaling, Adam, losses) is written once below.
#include "cmps_internal.h"

// numpy's rounding points means every product and sum rounds on its own.  hipcc contracts a * b + c into one fma by default, and HIP's
// __fmul_rn / __fadd_rn / __fsub_rn are the plain operators compiled under the header's settings, which do not stop it: Adam's m and v
// came out as v_fmac_f32 (one rounding where the host has two; hundreds of ulp of m where b1 m and (1 - b1) g cancel).  So: no
// contraction anywhere in this file, the double expressions of the chain rule included, and the float32 rounding points are spelled
// with the helpers below, whose operators are compiled under this pragma.
#pragma clang fp contract(off)

namespace cmps {

namespace {

constexpr int ONT = 1024;

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }      // (hipcc's float32 division is correctly rounded)

__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < ONT / 64; ++w) s += red[w];
    return s;
}

// effective R of model.py:36-42 from the raw variables, in the host's float32 rounding: Z = fl(c_r Rx) + i fl(c_r Ry), R[i][j] = Z[i][j] - Z[j][j]
__device__ __forceinline__ float2 eff_R(const float* Rx, const float* Ry, int D, int i, int j, float c_r, bool scaled) {
    const float zx = scaled ? mul_rn(c_r, Rx[i * D + j]) : Rx[i * D + j], zy = scaled ? mul_rn(c_r, Ry[i * D + j]) : Ry[i * D + j];
    const float dx = scaled ? mul_rn(c_r, Rx[j * D + j]) : Rx[j * D + j], dy = scaled ? mul_rn(c_r, Ry[j * D + j]) : Ry[j * D + j];
    return make_float2(sub_rn(zx, dx), sub_rn(zy, dy));
}

// float32 square root rounded to nearest, as np.sqrt returns it.  (__fsqrt_rn is HIP's native v_sqrt_f32: 1 ulp, not correctly rounded;
// the double root rounded once to float32 is -- 53 bits are more than twice 24 plus 2.)
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }

// tf.train.AdamOptimizer with numpy's float32 rounding points (audio_mps_amd/train.py::AdamOptimizer.apply_gradients)
__device__ __forceinline__ void adam(float* var, float* m, float* v, int idx, float g, float lr_t, float b1, float omb1, float b2,
                                     float omb2, float eps) {
    const float mn = add_rn(mul_rn(b1, m[idx]), mul_rn(omb1, g));
    const float vn = add_rn(mul_rn(b2, v[idx]), mul_rn(mul_rn(omb2, g), g));
    m[idx] = mn;
    v[idx] = vn;
    var[idx] = sub_rn(var[idx], div_rn(mul_rn(lr_t, mn), add_rn(sqrt_rn(vn), eps)));
}

struct OptArgs {
    int D, apply;
    double inv_batch, h_reg, r_reg;
    float c_r, c_h, lr_t, b1, omb1, b2, omb2, eps;
    int scaled_r, scaled_h, with_reg;
    int rank;                                                     // k_rho_apply_step only
};

// ---- the half k_apply_step and k_rho_apply_step share: vars = [A | Rx | Ry | freqs | ...], gs = [Rbar | fbar | 2 D | Abar | loss_sum | ...] ----

__device__ __forceinline__ int nonfinite(const float* gs, int lo, int hi) {
    int bad = 0;
    for (int idx = lo + threadIdx.x; idx < hi; idx += ONT) bad |= !isfinite(gs[idx]);
    return bad;
}

// A gradient with Inf / NaN in it next to a FINITE loss sum is the signature of an fp16-split operand that left its scaled range
// (include/cmps.h: CMPS_ERR_F16_RANGE): such a step is skipped -- variables and Adam slots stay as they are, losses[1] = NaN marks
// it -- instead of poisoning every variable.  The decision reads the all-reduced buffer, so every rank takes the same one.
__device__ __forceinline__ bool skip_step(const OptArgs& a, const float* gs, int bad, float* losses) {
    const int D = a.D, DD = D * D;
    const bool skip = __syncthreads_or(bad) != 0 && isfinite(gs[2 * DD + 3 * D + 1]);
    if (skip && threadIdx.x == 0) {
        losses[0] = (float)((double)gs[2 * DD + 3 * D + 1] * a.inv_batch);
        losses[1] = __builtin_nanf("");
    }
    return skip;
}

__device__ __forceinline__ double eff_f(const OptArgs& a, const float* fr, int d) {
    return a.scaled_h ? (double)mul_rn(a.c_h, fr[d]) : (double)fr[d];
}

// regulariser terms on the CURRENT effective parameters (train.py:55-60): sf = sum freqs^2, sr = sum |R|^2
__device__ __forceinline__ void reg_sums(const OptArgs& a, const float* Rx, const float* Ry, const float* fr, double* red, double& sf,
                                         double& sr) {
    const int D = a.D, DD = D * D, t = threadIdx.x;
    sf = 0.0, sr = 0.0;
    for (int d = t; d < D; d += ONT) {
        const double f = eff_f(a, fr, d);
        sf += f * f;
    }
    for (int idx = t; idx < DD; idx += ONT) {
        const float2 r = eff_R(Rx, Ry, D, idx / D, idx % D, a.c_r, a.scaled_r);
        sr += (double)r.x * r.x + (double)r.y * r.y;
    }
    sf = block_sum_d(sf, red);
    sr = block_sum_d(sr, red);
}

// column sums of Rbar (adjoint of the row-broadcast diagonal removal, model.py:42); visible after the next barrier
__device__ __forceinline__ void col_sums(const OptArgs& a, const float* Rx, const float* Ry, const float* gs, double* colsum) {
    const int D = a.D, DD = D * D;
    const double wr = a.with_reg ? 2.0 * a.r_reg : 0.0;
    for (int j = threadIdx.x; j < D; j += ONT) {
        double cx = 0.0, cy = 0.0;
        for (int i = 0; i < D; ++i) {
            const float2 r = eff_R(Rx, Ry, D, i, j, a.c_r, a.scaled_r);
            cx += (double)gs[i * D + j] * a.inv_batch + wr * r.x;
            cy += (double)gs[DD + i * D + j] * a.inv_batch + wr * r.y;
        }
        colsum[2 * j] = cx;
        colsum[2 * j + 1] = cy;
    }
}

__device__ __forceinline__ void write_losses(const OptArgs& a, const float* gs, double sf, double sr, float* losses) {
    if (threadIdx.x == 0) {
        const double loss = (double)gs[2 * a.D * a.D + 3 * a.D + 1] * a.inv_batch;
        losses[0] = (float)loss;
        losses[1] = (float)(a.with_reg ? loss + a.h_reg * sf + a.r_reg * sr : loss);
    }
}

#define CMPS_ADAM(idx, g) adam(vars, am, av, (idx), (g), a.lr_t, a.b1, a.omb1, a.b2, a.omb2, a.eps)

// gradient w.r.t. the raw freqs (model.py:49 with the c_h scaling, train.py:55-60), from the OLD freqs[d]
__device__ __forceinline__ float freqs_grad(const OptArgs& a, const float* gs, const float* fr, int d) {
    const double f = eff_f(a, fr, d);
    const double fb = (double)gs[2 * a.D * a.D + d] * a.inv_batch + (a.with_reg ? 2.0 * a.h_reg * f : 0.0);
    return (float)((a.scaled_h ? (double)a.c_h : 1.0) * fb);
}

// gradients w.r.t. Rx, Ry (model.py:36-42 with the c_r scaling) + Adam; the callers' loops over d (freqs and what follows them in
// the buffer) and A come behind it.  R's diagonal feeds a whole column of
// the effective R: every gradient is formed from the OLD variables (into the scratch buffer) before any variable is updated.
// Needs col_sums and a barrier before; ends without one.
__device__ __forceinline__ void step_common(const OptArgs& a, float* vars, float* am, float* av, const float* gs, const double* colsum,
                                            float* gxy) {
    const int D = a.D, DD = D * D, t = threadIdx.x;
    const float* Rx = vars + 1;
    const float* Ry = Rx + DD;
    const double wr = a.with_reg ? 2.0 * a.r_reg : 0.0;
    for (int idx = t; idx < DD; idx += ONT) {
        const int i = idx / D, j = idx % D;
        const float2 r = eff_R(Rx, Ry, D, i, j, a.c_r, a.scaled_r);
        double zx = (double)gs[idx] * a.inv_batch + wr * r.x, zy = (double)gs[DD + idx] * a.inv_batch + wr * r.y;
        if (i == j) { zx -= colsum[2 * j]; zy -= colsum[2 * j + 1]; }
        gxy[2 * idx] = (float)((a.scaled_r ? (double)a.c_r : 1.0) * zx);
        gxy[2 * idx + 1] = (float)((a.scaled_r ? (double)a.c_r : 1.0) * zy);
    }
    __syncthreads();
    for (int idx = t; idx < DD; idx += ONT) {
        CMPS_ADAM(1 + idx, gxy[2 * idx]);
        CMPS_ADAM(1 + DD + idx, gxy[2 * idx + 1]);
    }
}

__device__ __forceinline__ void adam_A(const OptArgs& a, float* vars, float* am, float* av, const float* gs) {
    if (threadIdx.x == 0) CMPS_ADAM(0, (float)((double)gs[2 * a.D * a.D + 3 * a.D] * a.inv_batch));
}

// effective R and A of the (updated) variables: model.py:36-42, 19 (freqs: eff_f32 in the callers' loops over d)
__device__ __forceinline__ void write_params_common(const OptArgs& a, const float* vars, float* params) {
    const int D = a.D, DD = D * D, t = threadIdx.x;
    const float* Rx = vars + 1;
    const float* Ry = Rx + DD;
    for (int idx = t; idx < DD; idx += ONT) {
        const float2 r = eff_R(Rx, Ry, D, idx / D, idx % D, a.c_r, a.scaled_r);
        params[idx] = r.x;
        params[DD + idx] = r.y;
    }
    if (t == 0) params[2 * DD + 3 * D] = vars[0];
}
__device__ __forceinline__ float eff_f32(const OptArgs& a, const float* fr, int d) { return a.scaled_h ? mul_rn(a.c_h, fr[d]) : fr[d]; }

// A bank (cmps_bank_apply_step): one workgroup per member, member = blockIdx.x.  Its buffers are row `member` of the callers' arrays
// (BankArgs: floats, for the scratch doubles, between two rows) and what is free per member comes from hyper[member] = (learning_rate,
// h_reg, r_reg, c_r, c_h); lr_t = (learning_rate * bias_num) / bias_den in double, the host's `lr * sqrt(1 - b2^t) / (1 - b1^t)` to
// the bit (audio_mps_amd/train.py::Trainer._apply).  The plain step is the instance BANK = false: it sees its arguments as before (the
// per-member values pass through the vector unit, which costs the bank instance two vector registers the plain one does not pay).
struct BankArgs {
    const double* hyper;          // [M][5] (the plain step: unused)
    double bias_num, bias_den;
    size_t n_vars, n_grad, n_scratch;
};

template <bool BANK>
__global__ __launch_bounds__(ONT) void k_apply_step(OptArgs a, BankArgs k, float* __restrict__ vars, float* __restrict__ am, float* __restrict__ av,
                                                    const float* __restrict__ gs, float* __restrict__ params,
                                                    float* __restrict__ losses, double* __restrict__ colsum) {
    __shared__ double red[ONT / 64];
    if constexpr (BANK) {
        const size_t m = blockIdx.x;
        const double* hy = k.hyper + 5 * m;
        // (workgroup-uniform values that the vector unit computes: back into scalar registers, where the plain step's arguments live)
        auto uni = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
        a.lr_t = uni((float)((hy[0] * k.bias_num) / k.bias_den));
        auto uni_d = [](double x) {
            return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
        };
        a.h_reg = uni_d(hy[1]); a.r_reg = uni_d(hy[2]);
        a.c_r = uni((float)hy[3]); a.c_h = uni((float)hy[4]);
        a.scaled_r = __builtin_amdgcn_readfirstlane(hy[3] != 1.0 ? 1 : 0); a.scaled_h = __builtin_amdgcn_readfirstlane(hy[4] != 1.0 ? 1 : 0);
    }
    {   // (the plain step: one workgroup, strides 0; without an update the null buffers are moved and never read)
        const size_t m = blockIdx.x;
        vars += m * k.n_vars; params += m * k.n_vars; am += m * k.n_vars; av += m * k.n_vars;
        gs += m * k.n_grad; losses += 2 * m; colsum += m * k.n_scratch;
    }
    const int D = a.D, DD = D * D, t = threadIdx.x;
    float* Rx = vars + 1;
    float* Ry = Rx + DD;
    float* fr = Ry + DD;
    float* px = fr + D;
    float* py = px + D;
    const bool skip = a.apply && skip_step(a, gs, nonfinite(gs, 0, 2 * DD + 3 * D + 1), losses);
    if (a.apply && !skip) {
        double sf, sr;
        reg_sums(a, Rx, Ry, fr, red, sf, sr);
        col_sums(a, Rx, Ry, gs, colsum);
        // ---- psi_0 adjoint (model.py:221-222): p0bar -> (psi_x, psi_y) ----
        double ss = 0.0, ib = 0.0;
        for (int d = t; d < D; d += ONT) {
            const double x = px[d], y = py[d];
            ss += x * x + y * y;
            ib += (double)gs[2 * DD + D + d] * a.inv_batch * x + (double)gs[2 * DD + 2 * D + d] * a.inv_batch * y;   // Re(conj(p0bar) p)
        }
        ss = block_sum_d(ss, red);
        ib = block_sum_d(ib, red);
        __syncthreads();                                           // colsum visible
        const double mm = ss > 1e-12 ? ss : 1e-12, inv = 1.0 / sqrt(mm);
        const double pc = ss > 1e-12 ? 2.0 * (ib * (-0.5 * inv / mm)) : 0.0;
        write_losses(a, gs, sf, sr, losses);
        step_common(a, vars, am, av, gs, colsum, reinterpret_cast<float*>(colsum + 2 * D));
        for (int d = t; d < D; d += ONT) {
            const double f = a.scaled_h ? (double)mul_rn(a.c_h, fr[d]) : (double)fr[d];
            const double fb = (double)gs[2 * DD + d] * a.inv_batch + (a.with_reg ? 2.0 * a.h_reg * f : 0.0);
            const float gf = (float)((a.scaled_h ? (double)a.c_h : 1.0) * fb);
            const double bx = (double)gs[2 * DD + D + d] * a.inv_batch, by = (double)gs[2 * DD + 2 * D + d] * a.inv_batch;
            const float gpx = (float)(bx * inv + pc * (double)px[d]), gpy = (float)(by * inv + pc * (double)py[d]);
            CMPS_ADAM(1 + 2 * DD + d, gf);
            CMPS_ADAM(1 + 2 * DD + D + d, gpx);
            CMPS_ADAM(1 + 2 * DD + 2 * D + d, gpy);
        }
        adam_A(a, vars, am, av, gs);
        __syncthreads();
    }
    // ---- effective parameters of the (updated) variables: model.py:36-42, 49, 221-222 ----
    write_params_common(a, vars, params);
    float ssf = 0.f;
    for (int d = t; d < D; d += ONT) {
        params[2 * DD + d] = eff_f32(a, fr, d);
        const float ab = hypotf(px[d], py[d]);                    // tf.abs of a complex64, then tf.square (model.py:331)
        ssf += ab * ab;
    }
    const float ss32 = (float)block_sum_d((double)ssf, red);
    const float invn = div_rn(1.0f, sqrt_rn(fmaxf(ss32, 1e-12f)));
    for (int d = t; d < D; d += ONT) {
        params[2 * DD + D + d] = mul_rn(px[d], invn);
        params[2 * DD + 2 * D + d] = mul_rn(py[d], invn);
    }
}

// RhoCMPS (audio_mps_amd/model.py::RhoCMPS.chain_rule, ::columns): the variables end in Wx, Wy [rank, D], the gradient sums in the
// column cotangents phibar_re, phibar_im [rank, D] (cmps_rho_loss_bwd); phi_out = the columns of the (updated) W.
// A bank (cmps_rho_bank_apply_step): one workgroup per member, as k_apply_step<BANK> -- the per-member values from hyper[member], the
// buffers row `member` of the callers' arrays (RhoBankArgs: floats, for the scratch doubles, between two rows).
struct RhoBankArgs {
    const double* hyper;          // [M][5] (the plain step: unused)
    double bias_num, bias_den;
    size_t n_vars, n_params, n_phi, n_grad, n_scratch;
};

template <bool BANK>
__global__ __launch_bounds__(ONT) void k_rho_apply_step(OptArgs a, RhoBankArgs k, float* __restrict__ vars, float* __restrict__ am,
                                                        float* __restrict__ av, const float* __restrict__ gs,
                                                        float* __restrict__ params, float* __restrict__ phi_out,
                                                        float* __restrict__ losses, double* __restrict__ colsum) {
    __shared__ double red[ONT / 64];
    if constexpr (BANK) {
        const size_t m = blockIdx.x;
        const double* hy = k.hyper + 5 * m;
        // (workgroup-uniform values that the vector unit computes: back into scalar registers, where the plain step's arguments live)
        auto uni = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
        a.lr_t = uni((float)((hy[0] * k.bias_num) / k.bias_den));
        auto uni_d = [](double x) {
            return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
        };
        a.h_reg = uni_d(hy[1]); a.r_reg = uni_d(hy[2]);
        a.c_r = uni((float)hy[3]); a.c_h = uni((float)hy[4]);
        a.scaled_r = __builtin_amdgcn_readfirstlane(hy[3] != 1.0 ? 1 : 0); a.scaled_h = __builtin_amdgcn_readfirstlane(hy[4] != 1.0 ? 1 : 0);
        // (without an update the null buffers are moved and never read)
        vars += m * k.n_vars; am += m * k.n_vars; av += m * k.n_vars; params += m * k.n_params; phi_out += m * k.n_phi;
        gs += m * k.n_grad; losses += 2 * m; colsum += m * k.n_scratch;
    }
    const int D = a.D, DD = D * D, RD = a.rank * D, t = threadIdx.x;
    float* Rx = vars + 1;
    float* Ry = Rx + DD;
    float* fr = Ry + DD;
    float* Wx = fr + D;
    float* Wy = Wx + RD;
    const int tail = 2 * DD + 3 * D + 2;                          // phibar_re [RD] | phibar_im [RD]
    // (the two psi_0 blocks of the pure-state layout are unused on this path and not read)
    const bool skip = a.apply && skip_step(a, gs, nonfinite(gs, 0, 2 * DD + D) | nonfinite(gs, 2 * DD + 3 * D, 2 * DD + 3 * D + 1) |
                                                  nonfinite(gs, tail, tail + 2 * RD), losses);
    if (a.apply && !skip) {
        double sf, sr;
        reg_sums(a, Rx, Ry, fr, red, sf, sr);
        col_sums(a, Rx, Ry, gs, colsum);
        // ---- column adjoint (model.py:128-130): phi = conj(W) / |W| over all rank * D entries as one vector, no floor on |W| ----
        double ss = 0.0;
        for (int idx = t; idx < RD; idx += ONT) {
            const double x = Wx[idx], y = Wy[idx];
            ss += x * x + y * y;
        }
        const double nrm = sqrt(block_sum_d(ss, red));
        double c = 0.0;
        for (int idx = t; idx < RD; idx += ONT)                   // Re(conj(phi) phibar), phi = (Wx - i Wy) / nrm
            c += (double)Wx[idx] / nrm * ((double)gs[tail + idx] * a.inv_batch) + -(double)Wy[idx] / nrm * ((double)gs[tail + RD + idx] * a.inv_batch);
        c = block_sum_d(c, red);
        __syncthreads();                                           // colsum visible
        write_losses(a, gs, sf, sr, losses);
        step_common(a, vars, am, av, gs, colsum, reinterpret_cast<float*>(colsum + 2 * D));
        for (int d = t; d < D; d += ONT) CMPS_ADAM(1 + 2 * DD + d, freqs_grad(a, gs, fr, d));
        adam_A(a, vars, am, av, gs);
        // every W gradient needs only its own entry and the two sums above (taken from the OLD W): updated in place
        for (int idx = t; idx < RD; idx += ONT) {
            const double pr = (double)Wx[idx] / nrm, pi = -(double)Wy[idx] / nrm;
            const double br = (double)gs[tail + idx] * a.inv_batch, bi = (double)gs[tail + RD + idx] * a.inv_batch;
            const float gwx = (float)((br - c * pr) / nrm), gwy = (float)(-((bi - c * pi) / nrm));
            CMPS_ADAM(1 + 2 * DD + D + idx, gwx);
            CMPS_ADAM(1 + 2 * DD + D + RD + idx, gwy);
        }
        __syncthreads();
    }
    // ---- effective parameters and columns of the (updated) variables: model.py:36-42, 49, 128-130; the psi_0 slot is e_0 ----
    write_params_common(a, vars, params);
    for (int d = t; d < D; d += ONT) {
        params[2 * DD + d] = eff_f32(a, fr, d);
        params[2 * DD + D + d] = d == 0 ? 1.f : 0.f;
        params[2 * DD + 2 * D + d] = 0.f;
    }
    double ss = 0.0;
    for (int idx = t; idx < RD; idx += ONT) {
        const double x = Wx[idx], y = Wy[idx];
        ss += x * x + y * y;
    }
    const double nrm = sqrt(block_sum_d(ss, red));
    for (int idx = t; idx < RD; idx += ONT) {
        phi_out[idx] = (float)((double)Wx[idx] / nrm);
        phi_out[RD + idx] = (float)(-(double)Wy[idx] / nrm);
    }
}

#undef CMPS_ADAM

}  // namespace

size_t apply_step_scratch_bytes(int D) { return (size_t)2 * D * sizeof(double) + (size_t)2 * D * D * sizeof(float); }

size_t rho_apply_step_scratch_bytes(int D, int rank) { (void)rank; return apply_step_scratch_bytes(D); }   // W is updated in place

static OptArgs opt_args(int D, int rank, bool apply, double inv_batch, double lr_t, double beta1, double beta2, double eps, double h_reg,
                        double r_reg, double c_r, double c_h, bool with_reg) {
    OptArgs a{};
    a.D = D; a.rank = rank; a.apply = apply ? 1 : 0;
    a.inv_batch = inv_batch; a.h_reg = h_reg; a.r_reg = r_reg;
    a.c_r = (float)c_r; a.c_h = (float)c_h;
    a.scaled_r = c_r != 1.0; a.scaled_h = c_h != 1.0; a.with_reg = with_reg ? 1 : 0;
    a.lr_t = (float)lr_t;
    a.b1 = (float)beta1; a.omb1 = (float)(1.0 - beta1);           // numpy: a python float times a float32 array rounds the scalar to float32
    a.b2 = (float)beta2; a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    return a;
}

hipError_t launch_apply_step(int D, bool apply, double inv_batch, double lr_t, double beta1, double beta2, double eps, double h_reg,
                             double r_reg, double c_r, double c_h, bool with_reg, float* vars, float* am, float* av,
                             const float* grad_sums, float* params_out, float* losses_out, double* scratch, hipStream_t s) {
    const OptArgs a = opt_args(D, 0, apply, inv_batch, lr_t, beta1, beta2, eps, h_reg, r_reg, c_r, c_h, with_reg);
    hipLaunchKernelGGL(k_apply_step<false>, dim3(1), dim3(ONT), 0, s, a, BankArgs{}, vars, am, av, grad_sums, params_out, losses_out, scratch);
    return hipGetLastError();
}

hipError_t launch_bank_apply_step(int D, int M, bool apply, double inv_batch, double bias_num, double bias_den, double beta1, double beta2,
                                  double eps, const double* hyper, bool with_reg, float* vars, float* am, float* av, const float* grad_sums,
                                  float* params_out, float* losses_out, double* scratch, hipStream_t s) {
    const OptArgs a = opt_args(D, 0, apply, inv_batch, 0.0, beta1, beta2, eps, 0.0, 0.0, 1.0, 1.0, with_reg);     // (k_apply_step fills the per-member ones)
    const size_t DD = (size_t)D * D;
    const BankArgs k{hyper, bias_num, bias_den, 2 * DD + 3 * D + 1, 2 * DD + 3 * D + 2, apply_step_scratch_bytes(D) / sizeof(double)};
    hipLaunchKernelGGL(k_apply_step<true>, dim3(M), dim3(ONT), 0, s, a, k, vars, am, av, grad_sums, params_out, losses_out, scratch);
    return hipGetLastError();
}

hipError_t launch_rho_apply_step(int D, int rank, bool apply, double inv_batch, double lr_t, double beta1, double beta2, double eps,
                                 double h_reg, double r_reg, double c_r, double c_h, bool with_reg, float* vars, float* am, float* av,
                                 const float* grad_sums, float* params_out, float* phi_out, float* losses_out, double* scratch,
                                 hipStream_t s) {
    const OptArgs a = opt_args(D, rank, apply, inv_batch, lr_t, beta1, beta2, eps, h_reg, r_reg, c_r, c_h, with_reg);
    hipLaunchKernelGGL(k_rho_apply_step<false>, dim3(1), dim3(ONT), 0, s, a, RhoBankArgs{}, vars, am, av, grad_sums, params_out, phi_out, losses_out,
                       scratch);
    return hipGetLastError();
}

hipError_t launch_rho_bank_apply_step(int D, int rank, int M, bool apply, double inv_batch, double bias_num, double bias_den, double beta1,
                                      double beta2, double eps, const double* hyper, bool with_reg, float* vars, float* am, float* av,
                                      const float* grad_sums, float* params_out, float* phi_out, float* losses_out, double* scratch,
                                      hipStream_t s) {
    const OptArgs a = opt_args(D, rank, apply, inv_batch, 0.0, beta1, beta2, eps, 0.0, 0.0, 1.0, 1.0, with_reg);  // (the kernel fills the per-member ones)
    const size_t DD = (size_t)D * D, RD = (size_t)rank * D;
    const RhoBankArgs k{hyper, bias_num, bias_den, 1 + 2 * DD + D + 2 * RD, 2 * DD + 3 * D + 1, 2 * RD, 2 * DD + 3 * D + 2 + 2 * RD,
                        rho_apply_step_scratch_bytes(D, rank) / sizeof(double)};
    hipLaunchKernelGGL(k_rho_apply_step<true>, dim3(M), dim3(ONT), 0, s, a, k, vars, am, av, grad_sums, params_out, phi_out, losses_out, scratch);
    return hipGetLastError();
}

}  // namespace cmps
