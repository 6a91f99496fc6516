// RhoCMPS, the density-matrix scan (model.py:55-203), general D, correctness-first.
//
// The reference carries rho [B, D, D] and applies  rho' = U rho U^dagger,  U = 1 - (dt sigma^2/2) Rt^dagger Rt + s Rt
// (model.py:172-187), loss += -log(1 + Re tr((Rt + Rt^dagger) rho') x / A) (:166, 189-196), rho = rho' / max(tr rho', eps)
// (:198-203).  rho_0 = W^dagger W / tr (:127-132) has rank r = initial_rank (default D), and U rho U^dagger keeps the rank,
// so this file never forms the D x D matrix in the scan: it carries the r columns phi_a of rho = sum_a phi_a phi_a^dagger
// (phi_a(0) = conj(W[a, :]) / sqrt(tr W^dagger W)) through the SAME rotating-frame step as the pure-state kernels,
//
//     y_a = u_a + Q u_a + s R u_a,     e = sum_a y_a^dagger (R + R^dagger) y_a,     n = sum_a |y_a|^2  (= tr rho'),
//     u_a <- rho_k * y_a / sqrt(max(n, 1e-12)),
//
// coupled only through the two scalars e and n: 3 r D^2 complex MACs per step instead of the 4 D^3 of the matrix form.
// One workgroup owns one clip; thread t owns component t of every column; the columns live in LDS.
// Reverse sweep (cotangents g_a of u_a, convention zbar = dL/dRe z + i dL/dIm z), cf. cmps_block.hip:
//     yhb_a = conj(rho_k) g_a;  dot = sum_a Re(yhat_a^dagger yhb_a);  ybar_a = (yhb_a - yhat_a dot)/sqrt(n) + 2 ebar H y_a
//     Rbar += 2 ebar sum_a y_a y_a^dagger + s sum_a ybar_a u_a^dagger;   Qbar += sum_a ybar_a u_a^dagger
//     g_a  = ybar_a + Q ybar_a + s R^dagger ybar_a;   fbar += dt_k sum_a Im(g_a conj(u_a(k+1)))
#include "cmps_block_util.h"

namespace cmps {

// ------------------------------------------------------------------------------------------------
// forward: RhoCMPS._build_loss_rho (model.py:133-144)
// ------------------------------------------------------------------------------------------------
template <int NT, int CW>
__global__ __launch_bounds__(NT) void k_fwd_rho(Dev P, RhoDev W, const float* __restrict__ audio,
                                                float* __restrict__ loss_out, int save, float2* gcols) {
    extern __shared__ float2 sh[];
    const int D = P.D, DP = P.DP, N = P.N, r = W.rank, rD = r * D;
    // the column arrays live in LDS when they fit and in the workspace (RhoDev::cols, L1 / L2 resident) when they do not
    // (rank * D above ~10000 here: the reference's default rank = D at D > 100, model.py:62-65)
    float2* base = gcols ? gcols + (size_t)blockIdx.x * 4 * rD : sh;
    float2* cur = base;
    float2* nxt = base + rD;
    float* red = reinterpret_cast<float*>(gcols ? sh : sh + 2 * rD);
    const int b = blockIdx.x, t = threadIdx.x;
    const bool act = t < D;
    // the mat-vecs: thread (tt, grp) owns component tt of the columns a0 .. a0 + CW - 1, a0 = CW (grp + NG i) -- one matrix element is
    // loaded once per chunk of CW columns (round 4; before: once per column, with only D of the NT threads at work)
    const int DPT = (NT == 64 || D <= 64) ? 64 : 128, tt = t & (DPT - 1), grp = t / DPT, NG = NT / DPT;
    const bool mact = tt < D;
    const float* xrow = audio + (size_t)b * P.T;
    float2* st = save ? W.stash + block_row_pair(b, N, 0, DP, r) : nullptr;
    if (act)
        for (int a = 0; a < r; ++a) cur[a * D + t] = W.phi0[a * DP + t];
    float loss = 0.f;
    for (int k = 0; k < N; ++k) {
        const float x = xrow[k + 1] - xrow[k];     // model.py:138
        const float s = x / dev_A(P);                   // :175
        __syncthreads();
        if (mact) {
            for (int a0 = grp * CW; a0 < r; a0 += NG * CW) {
                const int na = (r - a0) < CW ? (r - a0) : CW;
                int co[CW];                              // a ragged last chunk repeats its last column: no branch inside the j loop
#pragma unroll
                for (int c = 0; c < CW; ++c) co[c] = (a0 + (c < na ? c : na - 1)) * D;
                float2 v[CW], q[CW];
#pragma unroll
                for (int c = 0; c < CW; ++c) v[c] = q[c] = make_float2(0.f, 0.f);
                jloop2(P.RT, P.Q, D, DP, tt, [&](int j, float2 m1, float2 m2) {
#pragma unroll
                    for (int c = 0; c < CW; ++c) {
                        const float2 uj = cur[co[c] + j];
                        v[c] = cfma(m1, uj, v[c]);                // (R u_a)_t
                        q[c] = cfma_conj_a(m2, uj, q[c]);         // (Q u_a)_t, Q Hermitian
                    }
                });
#pragma unroll
                for (int c = 0; c < CW; ++c)
                    if (c < na) {
                        const int a = a0 + c;
                        const float2 u = cur[a * D + tt];
                        const float2 y = make_float2(u.x + q[c].x + s * v[c].x, u.y + q[c].y + s * v[c].y);   // column of U rho U^dagger, :186
                        nxt[a * D + tt] = y;
                        if (save) st[block_row_pair(0, N, k, DP, r, a) + tt] = y;
                    }
            }
        }
        __syncthreads();
        float pe = 0.f, pn = 0.f;
        if (mact) {
            for (int a0 = grp * CW; a0 < r; a0 += NG * CW) {
                const int na = (r - a0) < CW ? (r - a0) : CW;
                int co[CW];                              // a ragged last chunk repeats its last column: no branch inside the j loop
#pragma unroll
                for (int c = 0; c < CW; ++c) co[c] = (a0 + (c < na ? c : na - 1)) * D;
                float2 hy[CW];
#pragma unroll
                for (int c = 0; c < CW; ++c) hy[c] = make_float2(0.f, 0.f);
                jloop2(P.RT, P.R, D, DP, tt, [&](int j, float2 m1, float2 m2) {
#pragma unroll
                    for (int c = 0; c < CW; ++c) {
                        const float2 yj = nxt[co[c] + j];
                        hy[c] = cfma(m1, yj, hy[c]);
                        hy[c] = cfma_conj_a(m2, yj, hy[c]);       // ((R + R^dagger) y_a)_t, :193-194
                    }
                });
#pragma unroll
                for (int c = 0; c < CW; ++c)
                    if (c < na) {
                        const float2 y = nxt[(a0 + c) * D + tt];
                        pe += y.x * hy[c].x + y.y * hy[c].y;
                        pn += y.x * y.x + y.y * y.y;
                    }
            }
        }
        const float e = block_sum<NT>(pe, red);                  // Re tr(x rho'), :195-196
        const float n = block_sum<NT>(pn, red);                  // tr rho', :200
        loss += -logf(1.0f + (e * x) / dev_A(P));                      // :166, 155
        const float sc = sqrtf(1.0f / fmaxf(n, 1e-12f));          // :201 (columns scale with the square root)
        if (act) {
            const float2 rho = P.rho[(size_t)k * DP + t];
            for (int a = 0; a < r; ++a) nxt[a * D + t] = cmul(rho, cscale(sc, nxt[a * D + t]));
        }
        float2* tmp = cur; cur = nxt; nxt = tmp;
    }
    if (t == 0) loss_out[b] = loss;
}

// ------------------------------------------------------------------------------------------------
// reverse sweep
// ------------------------------------------------------------------------------------------------
template <int NT, int EPT, int CW>
__global__ __launch_bounds__(NT) void k_bwd_rho(Dev P, RhoDev W, const float* __restrict__ audio, float2* gcols) {
    extern __shared__ float2 sh[];
    const int D = P.D, DP = P.DP, N = P.N, r = W.rank, rD = r * D;
    float2* base = gcols ? gcols + (size_t)blockIdx.x * 4 * rD : sh;   // LDS, or the workspace when 4 r D complex numbers do not fit
    float2* Y = base;             // y_a of step k
    float2* YB = base + rD;       // yhb_a, then ybar_a
    float2* U = base + 2 * rD;    // H y_a, then u_a(k)
    float2* G = base + 3 * rD;    // cotangent of u_a(k+1)
    float* red = reinterpret_cast<float*>(gcols ? sh : sh + 4 * rD);
    const int b = blockIdx.x, t = threadIdx.x;
    const bool act = t < D;
    const int DPT = (NT == 64 || D <= 64) ? 64 : 128, tt = t & (DPT - 1), grp = t / DPT, NG = NT / DPT;   // the mat-vecs: as in k_fwd_rho
    const bool mact = tt < D;
    const float* xrow = audio + (size_t)b * P.T;
    const float2* st = W.stash + (size_t)b * N * r * DP;   // block_row_pair(b, N, 0, DP, r): a call moves this kernel's instructions
    const float2 zero = make_float2(0.f, 0.f);
    float2 Rb[EPT], Qb[EPT];
#pragma unroll
    for (int m = 0; m < EPT; ++m) Rb[m] = Qb[m] = zero;
    float facc = 0.f, Abar = 0.f;
    if (act)
        for (int a = 0; a < r; ++a) G[a * D + t] = zero;

    for (int k = N - 1; k >= 0; --k) {
        const float x = xrow[k + 1] - xrow[k];
        const float s = x / dev_A(P);
        const float2 rho = act ? P.rho[(size_t)k * DP + t] : make_float2(1.f, 0.f);
        float pn = 0.f;
        if (act) {
            for (int a = 0; a < r; ++a) {
                const float2 y = st[((size_t)k * r + a) * DP + t];
                Y[a * D + t] = y;
                pn += y.x * y.x + y.y * y.y;
            }
        }
        const float nraw = block_sum<NT>(pn, red);
        const float inv = sqrtf(1.0f / fmaxf(nraw, 1e-12f));
        float pd = 0.f;
        if (act) {
            const float dk = P.dtk[k];
            for (int a = 0; a < r; ++a) {
                const float2 yh = cscale(inv, Y[a * D + t]);
                const float2 un = cmul(rho, yh);
                const float2 g = G[a * D + t];
                facc += dk * (g.y * un.x - g.x * un.y);
                const float2 yhb = cmul_conj_a(rho, g);
                pd += yh.x * yhb.x + yh.y * yhb.y;
                YB[a * D + t] = yhb;
            }
        }
        const float dot = block_sum<NT>(pd, red);
        __syncthreads();
        float pe = 0.f;
        if (mact) {
            for (int a0 = grp * CW; a0 < r; a0 += NG * CW) {
                const int na = (r - a0) < CW ? (r - a0) : CW;
                int co[CW];                              // a ragged last chunk repeats its last column: no branch inside the j loop
#pragma unroll
                for (int c = 0; c < CW; ++c) co[c] = (a0 + (c < na ? c : na - 1)) * D;
                float2 hy[CW];
#pragma unroll
                for (int c = 0; c < CW; ++c) hy[c] = zero;
                jloop2(P.RT, P.R, D, DP, tt, [&](int j, float2 m1, float2 m2) {
#pragma unroll
                    for (int c = 0; c < CW; ++c) {
                        const float2 yj = Y[co[c] + j];
                        hy[c] = cfma(m1, yj, hy[c]);
                        hy[c] = cfma_conj_a(m2, yj, hy[c]);
                    }
                });
#pragma unroll
                for (int c = 0; c < CW; ++c)
                    if (c < na) {
                        const float2 y = Y[(a0 + c) * D + tt];
                        pe += y.x * hy[c].x + y.y * hy[c].y;
                        U[(a0 + c) * D + tt] = hy[c];
                    }
            }
        }
        const float e = block_sum<NT>(pe, red);
        const float ex = e * x;
        const float z = ex / dev_A(P);
        const float zbar = -1.0f / (1.0f + z);
        const float ebar = zbar * x / dev_A(P);
        Abar += zbar * (-ex / (dev_A(P) * dev_A(P)));
        const float te = 2.0f * ebar;
        float pnp = 0.f;
        if (act) {
            for (int a = 0; a < r; ++a) {
                const float2 yhb = YB[a * D + t], hy = U[a * D + t];
                const float2 yh = cscale(inv, Y[a * D + t]);
                float2 yb;
                if (nraw > 1e-12f)
                    yb = make_float2((yhb.x - yh.x * dot) * inv, (yhb.y - yh.y * dot) * inv);
                else
                    yb = cscale(inv, yhb);
                yb.x += te * hy.x;
                yb.y += te * hy.y;
                YB[a * D + t] = yb;
                float2 up;
                if (k > 0) {
                    up = st[((size_t)(k - 1) * r + a) * DP + t];
                    pnp += up.x * up.x + up.y * up.y;
                } else {
                    up = W.phi0[a * DP + t];
                }
                U[a * D + t] = up;
            }
        }
        if (k > 0) {
            const float nprev = block_sum<NT>(pnp, red);
            const float invp = sqrtf(1.0f / fmaxf(nprev, 1e-12f));
            if (act) {
                const float2 rhop = P.rho[(size_t)(k - 1) * DP + t];
                for (int a = 0; a < r; ++a) U[a * D + t] = cmul(rhop, cscale(invp, U[a * D + t]));
            }
        }
        __syncthreads();
        float ps = 0.f;
        if (mact) {
            for (int a0 = grp * CW; a0 < r; a0 += NG * CW) {
                const int na = (r - a0) < CW ? (r - a0) : CW;
                int co[CW];                              // a ragged last chunk repeats its last column: no branch inside the j loop
#pragma unroll
                for (int c = 0; c < CW; ++c) co[c] = (a0 + (c < na ? c : na - 1)) * D;
                float2 bq[CW], d[CW];
#pragma unroll
                for (int c = 0; c < CW; ++c) bq[c] = d[c] = zero;
                jloop2(P.Q, P.R, D, DP, tt, [&](int j, float2 m1, float2 m2) {
#pragma unroll
                    for (int c = 0; c < CW; ++c) {
                        const float2 yj = YB[co[c] + j];
                        bq[c] = cfma_conj_a(m1, yj, bq[c]);      // (Q ybar_a)_t
                        d[c] = cfma_conj_a(m2, yj, d[c]);        // (R^dagger ybar_a)_t
                    }
                });
#pragma unroll
                for (int c = 0; c < CW; ++c)
                    if (c < na) {
                        const int a = a0 + c;
                        const float2 uk = U[a * D + tt], ybt = YB[a * D + tt];
                        ps += d[c].x * uk.x + d[c].y * uk.y;
                        G[a * D + tt] = make_float2(ybt.x + bq[c].x + s * d[c].x, ybt.y + bq[c].y + s * d[c].y);
                    }
            }
        }
        const float sbar = block_sum<NT>(ps, red);
        Abar += sbar * (-x / (dev_A(P) * dev_A(P)));
        for_owned<NT, EPT>(D, [&](int m, int i, int j) {
            float2 o1 = zero, o2 = zero;
            for (int a = 0; a < r; ++a) {
                const float2 yi = Y[a * D + i], yj = Y[a * D + j], ybi = YB[a * D + i], uj = U[a * D + j];
                o1.x += yi.x * yj.x + yi.y * yj.y;
                o1.y += yi.y * yj.x - yi.x * yj.y;
                o2.x += ybi.x * uj.x + ybi.y * uj.y;
                o2.y += ybi.y * uj.x - ybi.x * uj.y;
            }
            Rb[m].x += te * o1.x + s * o2.x;
            Rb[m].y += te * o1.y + s * o2.y;
            Qb[m].x += o2.x;
            Qb[m].y += o2.y;
        });
        __syncthreads();
    }
    // slab: the pure-state layout (psi_0 slots zero) followed by the cotangents of the r initial columns
    float* slab = W.slabs + (size_t)b * W.slab_floats;
    const int DD = DP * DP;
    for (int idx = t; idx < (int)W.slab_floats; idx += NT) slab[idx] = 0.f;
    __syncthreads();
    store_rq_planes<NT, EPT>(slab, DD, D, DP, Rb, Qb);
    if (act) {
        slab[4 * DD + t] = facc;
        float* tail = slab + 4 * DD + 3 * DP + 2;
        for (int a = 0; a < r; ++a) {
            const float2 g = G[a * D + t];
            tail[a * DP + t] = g.x;
            tail[(r + a) * DP + t] = g.y;
        }
    }
    if (t == 0) slab[4 * DD + 3 * DP] = Abar;
}

// tail of the gradient buffer: d phi_re [r][D] | d phi_im [r][D]
__global__ void k_finalize_rho(Dev P, RhoDev W, float* __restrict__ grad_out) {
    const int D = P.D, DP = P.DP, r = W.rank;
    const float* tail = W.sums + 4 * DP * DP + 3 * DP + 2;
    float* out = grad_out + 2 * D * D + 3 * D + 2;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (int idx = tid; idx < 2 * r * D; idx += nth) {
        const int a = idx / D, d = idx % D;      // a in [0, 2r): re rows then im rows
        out[idx] = tail[a * DP + d];
    }
}

// ------------------------------------------------------------------------------------------------
// rho_evolve_with_data / rho_evolve_with_sampling / purity (model.py:76-107): lab-frame rho after every
// step from the stashed columns,  rho_k = phases_k (sum_a y_a y_a^dagger) phases_k^dagger / max(n, eps)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_states_rho(Dev P, RhoDev W, int steps, float* __restrict__ rho_out,
                                                    float* __restrict__ purity_out, int direct) {
    extern __shared__ float2 sh[];
    const int D = P.D, DP = P.DP, r = W.rank;
    // direct != 0: the r columns do not fit in LDS and are read from the stash (L1 / L2) every time they are needed
    float2* Y = sh;                                         // [r][D] (direct == 0)
    float2* ph = direct ? sh : sh + r * D;                  // [D]
    float* red = reinterpret_cast<float*>(ph + D);
    const size_t row = blockIdx.x;                          // b * steps + k
    const int k = (int)(row % steps), t = threadIdx.x;
    const int b = (int)(row / steps);
    const float2* st = W.stash + block_row_pair(b, steps, k, DP, r);
    const float* stw = reinterpret_cast<const float*>(W.stash) + wave_row(b, steps, k, r);   // wave and MFMA layouts: one wave row per column
    auto ldY = [&](int a, int d) {                          // every layout's positions: cmps_stash_layout.h
        if (W.stash_layout == RHO_STASH_WIDE) {             // the wide kernels' rows: one vector per pair of columns
            const float* v = W.vstash + wide_stash_vec(DP, rho_wide_pair(b, W.vrank, a), steps, k, 0);
            return make_float2(v[wide_pos(d, 0, rho_wide_clip(a))], v[wide_pos(d, 1, rho_wide_clip(a))]);
        }
        const float* w = stw + a * WAVE_ROW;
        return W.stash_layout == RHO_STASH_WAVE ? make_float2(w[wave16_pos(d, 0, 0)], w[wave16_pos(d, 1, 0)])
             : W.stash_layout == RHO_STASH_MFMA ? make_float2(w[wave32_pos(d, 0, 0)], w[wave32_pos(d, 1, 0)]) : st[a * DP + d];
    };
    float pn = 0.f;
    for (int idx = t; idx < r * D; idx += 256) {
        const int a = idx / D, d = idx % D;
        const float2 y = ldY(a, d);
        if (!direct) Y[idx] = y;
        pn += y.x * y.x + y.y * y.y;
    }
    if (t < D) ph[t] = phase(P.freqs[t], P.ttab[k]);
    const float n = block_sum<256>(pn, red);
    const float inv = 1.0f / fmaxf(n, 1e-12f);
    __syncthreads();
    float pp = 0.f;
    for (int idx = t; idx < D * D; idx += 256) {
        const int i = idx / D, j = idx % D;
        float2 o = make_float2(0.f, 0.f);
        for (int a = 0; a < r; ++a) {
            const float2 yi = direct ? ldY(a, i) : Y[a * D + i], yj = direct ? ldY(a, j) : Y[a * D + j];
            o.x += yi.x * yj.x + yi.y * yj.y;
            o.y += yi.y * yj.x - yi.x * yj.y;
        }
        o = cscale(inv, o);
        pp += o.x * o.x + o.y * o.y;                        // tr rho^2 = sum |rho_ij|^2 (Hermitian), model.py:96
        if (rho_out) {
            const float2 w = cmul(cmul(ph[i], o), make_float2(ph[j].x, -ph[j].y));
            rho_out[(row * D * D + idx) * 2] = w.x;
            rho_out[(row * D * D + idx) * 2 + 1] = w.y;
        }
    }
    const float pur = block_sum<256>(pp, red);
    if (purity_out && t == 0) purity_out[row] = pur;
}

// ------------------------------------------------------------------------------------------------
// RhoCMPS._update_ancilla_rho (model.py:172-187) for a general rho [B][D][D]: one workgroup per (clip, row i)
//   U[i][j] = delta_ij + phases_i (Q[i][j] + s R[i][j]) conj(phases_j);   out = (U rho) U^dagger
// ------------------------------------------------------------------------------------------------
__global__ void k_update_ancilla_rho(Dev P, const float* __restrict__ rho_in, const float* __restrict__ signal,
                                     float tt, float* __restrict__ rho_out) {
    extern __shared__ float2 sh[];
    const int D = P.D, DP = P.DP;
    float2* ph = sh;            // [D]
    float2* Ui = sh + D;        // row i of U
    float2* Ti = sh + 2 * D;    // row i of U rho
    const int b = blockIdx.x / D, i = blockIdx.x % D, t = threadIdx.x;
    const bool act = t < D;
    const float s = signal[b] / dev_A(P);
    if (act) ph[t] = phase(P.freqs[t], tt);
    __syncthreads();
    auto Uel = [&](int a, int c) {
        const float2 q = P.Q[c * DP + a];           // Q[a][c] = conj(Q[c][a])
        const float2 rr = P.RT[c * DP + a];         // R[a][c]
        const float2 m = make_float2(q.x + s * rr.x, -q.y + s * rr.y);
        float2 u = cmul(cmul(ph[a], m), make_float2(ph[c].x, -ph[c].y));
        if (a == c) u.x += 1.0f;
        return u;
    };
    if (act) Ui[t] = Uel(i, t);
    __syncthreads();
    const float* rin = rho_in + (size_t)b * D * D * 2;
    if (act) {
        float2 acc = make_float2(0.f, 0.f);
        for (int j = 0; j < D; ++j)
            acc = cfma(Ui[j], make_float2(rin[(j * D + t) * 2], rin[(j * D + t) * 2 + 1]), acc);
        Ti[t] = acc;
    }
    __syncthreads();
    if (act) {
        float2 acc = make_float2(0.f, 0.f);        // out[i][l=t] = sum_k T[i][k] conj(U[l][k])
        for (int k = 0; k < D; ++k) {
            const float2 u = Uel(t, k);
            acc = cfma(Ti[k], make_float2(u.x, -u.y), acc);
        }
        float* o = rho_out + ((size_t)b * D * D + (size_t)i * D + t) * 2;
        o[0] = acc.x;
        o[1] = acc.y;
    }
}

// ------------------------------------------------------------------------------------------------
// RhoCMPS.sample / rho_evolve_with_sampling / purity (model.py:86-116, 160-167)
// PRIMED (cmps_rho_sample_primed): PF = prime_T - 1 teacher-forced steps (increment prime[k + 1] - prime[k], model.py:138; running sum 0;
// e dt, taken before the update, to pred[b][k] when asked) in front of the `length` sampled ones, which read noise[b][k - PF] and write
// out[b][k - PF]; table row and stash row k throughout.  The unprimed instance (cmps_rho_sample) ignores its last argument and is the
// kernel as it was (profiles/rho_primed_isa_identity.log).
// STREAM (cmps_rho_stream): the primed scan as one segment of a longer one -- PF or length may be 0, step k of the launch runs on table
// row ST.k0 + k (noise, out, pred and the stash rows keep the segment's own k), and the columns S (in whichever home they have) and the
// running sum come from the path's record when ST.in is set and go to it behind the last step when ST.out is.  Thread t moves the
// components t of all columns, the ones it alone writes in a step.  The other instances ignore ST and are the kernels they were
// (profiles/rho_stream_isa_identity.log).
// SCORE (cmps_rho_stream_score): a stream segment of forced steps that also gives every step's loss increment (model.py:152-158, 169-170).
// Behind the barrier that follows the update, when Wb holds all of y_a = u_a + Q u_a + s R u_a (un-normalised, frame of t_k), one more pass:
// thread t forms (R y_a)[t] from RT for every column (four at a time) and sums Re(conj(y_a[t]) (R y_a)[t]); e' = 2 x the block's sum = Re tr((Rt +
// Rt^dagger) rho'), z = (e' x) / A, lv = -log(1 + z) as in k_fwd_rho above.  The pass reads Wb across threads: nothing writes Wb between
// that barrier and the one at the top of the next step (the rotation reads a thread's own components and writes S).  lv is added to the
// running loss (SC.loss[b]: read on a resumed scan, written behind the last step) and stored to SC.nll[b][k] when set.  The columns, the
// running sum, pred and the stash are untouched.  The other instances ignore SC and are the kernels they were
// (profiles/rho_stream_score_isa_identity.log).
// ------------------------------------------------------------------------------------------------
template <int NT, bool PRIMED, bool STREAM = false, bool SCORE = false>
__global__ __launch_bounds__(NT) void k_sample_rho(Dev P, RhoDev W, const float* __restrict__ noise, int length,
                                                   float* __restrict__ out, int save, float2* gcols, PrimeDev PR, StreamDev ST, ScoreDev SC) {
    static_assert(PRIMED || !STREAM, "a stream segment is a primed scan");
    static_assert(STREAM || !SCORE, "a scored segment is a stream segment");
    extern __shared__ float2 sh[];
    const int D = P.D, DP = P.DP, r = W.rank, rD = r * D;
    float2* base = gcols ? gcols + (size_t)blockIdx.x * 4 * rD : sh;
    float2* S = base;             // u_a
    float2* Vb = base + rD;       // R u_a
    float2* Wb = base + 2 * rD;   // u_a + Q u_a
    float* red = reinterpret_cast<float*>(gcols ? sh : sh + 3 * rD);
    const int b = blockIdx.x, t = threadIdx.x;
    const bool act = t < D;
    const int PF = PRIMED ? PR.PF : 0, nsteps = PF + length;        // (unprimed: nsteps = length)
    const float* prow = PRIMED ? PR.prime + (size_t)b * PR.stride : nullptr;      // (stride 0: one clip shared by all paths)
    float2* st = save ? W.stash + block_row_pair(b, nsteps, 0, DP, r) : nullptr;
    float samp = 0.f;
    const float2* rin = nullptr;                                    // (STREAM) this path's record to carry on from
    if constexpr (STREAM) rin = ST.in ? reinterpret_cast<const float2*>(ST.in + (size_t)b * ST.rec) : nullptr;
    if (STREAM && rin) {
        if (act)
            for (int a = 0; a < r; ++a) S[a * D + t] = rin[a * D + t];
        samp = ST.in[(size_t)b * ST.rec + 2 * rD];
    } else {
        if (act)
            for (int a = 0; a < r; ++a) S[a * D + t] = W.phi0[a * DP + t];
    }
    [[maybe_unused]] float loss = 0.f;                              // SCORE: the path's running loss (model.py:155)
    if constexpr (SCORE) {
        if (rin) loss = SC.loss[b];
    }
    for (int k = 0; k < nsteps; ++k) {
        __syncthreads();
        float pe = 0.f;
        if (act) {
            for (int a = 0; a < r; ++a) {
                const float2* ua = S + a * D;
                float2 v = make_float2(0.f, 0.f), q = make_float2(0.f, 0.f);
                for (int j = 0; j < D; ++j) {
                    const float2 uj = ua[j];
                    v = cfma(P.RT[j * DP + t], uj, v);
                    q = cfma_conj_a(P.Q[j * DP + t], uj, q);
                }
                const float2 u = ua[t];
                pe += u.x * v.x + u.y * v.y;
                Vb[a * D + t] = v;
                Wb[a * D + t] = cadd(u, q);
            }
        }
        const float e = 2.0f * block_sum<NT>(pe, red);                            // Re tr((Rt + Rt^dagger) rho), :189-196
        float inc;
        const bool forced = PRIMED && k < PF;
        if constexpr (PRIMED) {
            inc = forced ? prow[k + 1] - prow[k] : e * P.dt + noise[(size_t)b * length + (k - PF)];
            samp = forced ? 0.f : samp + inc;
        } else {
            inc = e * P.dt + noise[(size_t)b * length + k];                        // :162
            samp += inc;                                                           // :163
        }
        const float s = inc / dev_A(P);                                                 // :164, 175
        float pn = 0.f;
        if (act) {
            for (int a = 0; a < r; ++a) {
                const float2 w = Wb[a * D + t], v = Vb[a * D + t];
                const float2 y = make_float2(w.x + s * v.x, w.y + s * v.y);
                Wb[a * D + t] = y;
                pn += y.x * y.x + y.y * y.y;
                if (save) st[block_row_pair(0, nsteps, k, DP, r, a) + t] = y;
            }
        }
        const float n = block_sum<NT>(pn, red);
        const float sc = sqrtf(1.0f / fmaxf(n, 1e-12f));                           // :165
        __syncthreads();
        if constexpr (SCORE) {                                      // (every step of a scored segment is forced: inc is the clip's increment)
            float ph = 0.f;
            if (act) {
                constexpr int CW = 4;                               // columns per chunk: one matrix element is loaded once for CW of them
                for (int a0 = 0; a0 < r; a0 += CW) {
                    const int na = (r - a0) < CW ? (r - a0) : CW;
                    const float2* ya[CW];                           // a ragged last chunk repeats its last column: no branch inside the j loop
#pragma unroll
                    for (int c = 0; c < CW; ++c) ya[c] = Wb + (a0 + (c < na ? c : na - 1)) * D;
                    float2 h[CW];
#pragma unroll
                    for (int c = 0; c < CW; ++c) h[c] = make_float2(0.f, 0.f);
                    for (int j = 0; j < D; ++j) {
                        const float2 m = P.RT[j * DP + t];
#pragma unroll
                        for (int c = 0; c < CW; ++c) h[c] = cfma(m, ya[c][j], h[c]);      // (R y_a)_t
                    }
#pragma unroll
                    for (int c = 0; c < CW; ++c)
                        if (c < na) {
                            const float2 y = ya[c][t];
                            ph += y.x * h[c].x + y.y * h[c].y;
                        }
                }
            }
            const float e2 = 2.0f * block_sum<NT>(ph, red);          // Re tr((Rt + Rt^dagger) rho'), :189-196 on the columns of :186
            const float z = (e2 * inc) / dev_A(P);                   // :166
            const float lv = -logf(1.0f + z);
            loss += lv;                                              // :155
            if (t == 0 && SC.nll) SC.nll[(size_t)b * PF + k] = lv;
        }
        if (act) {
            const float2 rho = P.rho[(size_t)(STREAM ? ST.k0 + k : k) * DP + t];
            for (int a = 0; a < r; ++a) S[a * D + t] = cmul(rho, cscale(sc, Wb[a * D + t]));
        }
        if constexpr (PRIMED) {
            if (t == 0) {
                if (!forced) out[(size_t)b * length + (k - PF)] = dev_A(P) * samp;
                else if (PR.pred) PR.pred[(size_t)b * PF + k] = e * P.dt;
            }
        } else {
            if (t == 0) out[(size_t)b * length + k] = dev_A(P) * samp;                  // :116
        }
    }
    if constexpr (SCORE) {
        if (t == 0) SC.loss[b] = loss;
    }
    if constexpr (STREAM) {
        if (ST.out) {                                               // (in == out: thread t read these components before the first step)
            float* rec = ST.out + (size_t)b * ST.rec;
            if (act)
                for (int a = 0; a < r; ++a) reinterpret_cast<float2*>(rec)[a * D + t] = S[a * D + t];
            if (t == 0) rec[2 * rD] = samp;
        }
    }
}

// pack the r initial columns into the DP-strided table (a bank: member = blockIdx.y, whose columns lie 2 r D floats and whose table
// `ws` bytes behind its predecessor's; a plain launch has one member)
__global__ void k_pack_phi(int D, int DP, int r, const float* __restrict__ re, const float* __restrict__ im,
                           float2* __restrict__ phi0, size_t ws) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    re += (size_t)blockIdx.y * 2 * r * D; im += (size_t)blockIdx.y * 2 * r * D;
    phi0 = bank_shift(phi0, blockIdx.y * ws);
    if (idx >= r * DP) return;
    const int a = idx / DP, d = idx % DP;
    phi0[idx] = d < D ? make_float2(re[a * D + d], im[a * D + d]) : make_float2(0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
hipError_t launch_pack_phi(const Dev& P, const RhoDev& W, const float* re, const float* im, hipStream_t s, int M) {
    const int n = W.rank * P.DP;
    hipLaunchKernelGGL(k_pack_phi, dim3((n + 255) / 256, M), dim3(256), 0, s, P.D, P.DP, W.rank, re, im,
                       const_cast<float2*>(W.phi0), P.bank_stride);
    return hipGetLastError();
}

// beyond RHO_LDS_MAX (cmps_internal.h: rho_cols_spill) the column arrays go to RhoDev::cols (the workspace)
static float2* cols_if_needed(const RhoDev& W, size_t lds_bytes, size_t& shm, int blocks) {
    if (lds_bytes <= RHO_LDS_MAX) { shm = lds_bytes; return nullptr; }
    shm = 1024;                                   // reduction scratch (and the phases of k_states_rho) only
    return (W.cols && blocks <= W.cols_blocks) ? W.cols : reinterpret_cast<float2*>(1);   // 1: "needed but not provided"
}

// columns per mat-vec chunk (accumulators in registers): 8 when every column group has at least 8 columns, else 4
template <int NT, int CW>
static hipError_t run_fwd_rho(const Dev& P, const RhoDev& W, const float* audio, float* loss, bool save, float2* g, size_t shm, hipStream_t s) {
    hipError_t e = lds_attr(k_fwd_rho<NT, CW>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_fwd_rho<NT, CW>), dim3(P.B), dim3(NT), shm, s, P, W, audio, loss, save ? 1 : 0, g);
    return hipGetLastError();
}
template <int NT, int EPT, int CW>
static hipError_t run_bwd_rho(const Dev& P, const RhoDev& W, const float* audio, float2* g, size_t shm, hipStream_t s) {
    hipError_t e = lds_attr(k_bwd_rho<NT, EPT, CW>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_bwd_rho<NT, EPT, CW>), dim3(P.B), dim3(NT), shm, s, P, W, audio, g);
    return hipGetLastError();
}

hipError_t launch_fwd_rho(const Dev& P, const RhoDev& W, const float* audio, float* loss, bool save, hipStream_t s) {
    size_t shm;
    float2* g = cols_if_needed(W, (size_t)2 * W.rank * P.D * sizeof(float2) + 128, shm, P.B);
    if (g == reinterpret_cast<float2*>(1)) return hipErrorInvalidValue;
    if (P.D <= 32) return W.rank >= 8 ? run_fwd_rho<64, 8>(P, W, audio, loss, save, g, shm, s) : run_fwd_rho<64, 4>(P, W, audio, loss, save, g, shm, s);
    const bool wide = W.rank >= 32;               // four column groups (of 64 threads up to D = 64, of 128 above)
    if (P.D <= 64) return wide ? run_fwd_rho<256, 8>(P, W, audio, loss, save, g, shm, s) : run_fwd_rho<256, 4>(P, W, audio, loss, save, g, shm, s);
    return wide ? run_fwd_rho<512, 8>(P, W, audio, loss, save, g, shm, s) : run_fwd_rho<512, 4>(P, W, audio, loss, save, g, shm, s);
}

hipError_t launch_bwd_rho(const Dev& P, const RhoDev& W, const float* audio, hipStream_t s) {
    size_t shm;
    float2* g = cols_if_needed(W, (size_t)4 * W.rank * P.D * sizeof(float2) + 128, shm, P.B);
    if (g == reinterpret_cast<float2*>(1)) return hipErrorInvalidValue;
    return dispatch_block_bwd(P.D, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, GROUPS = NT == 64 ? 1 : NT == 256 ? 4 : 8;   // column groups: NT / 64 up to D = 64, NT / 128 above
        return dispatch_bool(W.rank >= 8 * GROUPS, [&](auto cw8) {
            return run_bwd_rho<NT, BLOCK_EPT, decltype(cw8)::value ? 8 : 4>(P, W, audio, g, shm, s);
        });
    });
}

hipError_t launch_finalize_rho(const Dev& P, const RhoDev& W, float* grad_out, hipStream_t s) {
    hipLaunchKernelGGL(k_finalize_rho, dim3(8), dim3(256), 0, s, P, W, grad_out);
    return hipGetLastError();
}

hipError_t launch_states_rho(const Dev& P, const RhoDev& W, int B, int steps, float* rho_out, float* purity_out,
                             hipStream_t s) {
    size_t shm = ((size_t)W.rank * P.D + P.D) * sizeof(float2) + 128;
    const int direct = shm > RHO_LDS_MAX ? 1 : 0;
    if (direct) shm = (size_t)P.D * sizeof(float2) + 128;
    hipError_t e = lds_attr(k_states_rho, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_states_rho, dim3((unsigned)((size_t)B * steps)), dim3(256), shm, s, P, W, steps, rho_out, purity_out, direct);
    return hipGetLastError();
}

hipError_t launch_update_ancilla_rho(const Dev& P, const float* rho_in, const float* signal, float t, int B,
                                     float* rho_out, hipStream_t s) {
    const size_t shm = (size_t)3 * P.D * sizeof(float2);
    hipLaunchKernelGGL(k_update_ancilla_rho, dim3((unsigned)(B * P.D)), dim3(round_up64(P.D)), shm, s, P, rho_in, signal, t, rho_out);
    return hipGetLastError();
}

hipError_t launch_sample_rho(const Dev& P, const RhoDev& W, const SampleDev& S, bool save, hipStream_t s) {
    size_t shm;
    float2* g = cols_if_needed(W, (size_t)3 * W.rank * P.D * sizeof(float2) + 128, shm, S.n);
    if (g == reinterpret_cast<float2*>(1)) return hipErrorInvalidValue;
    return dispatch_block_nt(P.D, [&](auto nt) {
        return dispatch_sample_mode(sample_mode(S), [&](auto mode) {
            constexpr int NT = decltype(nt)::value, M = decltype(mode)::value;
            const hipError_t e = lds_attr(k_sample_rho<NT, M >= SAMPLE_PRIMED, M >= SAMPLE_STREAM, M == SAMPLE_SCORE>, shm);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((k_sample_rho<NT, M >= SAMPLE_PRIMED, M >= SAMPLE_STREAM, M == SAMPLE_SCORE>), dim3(S.n), dim3(NT), shm, s, P, W, S.noise,
                               S.length, S.out, save ? 1 : 0, g, S.PR, stream_of(S), score_of(S));
            return hipGetLastError();
        });
    });
}

}  // namespace cmps
