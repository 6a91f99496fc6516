// Two wavefronts per clip (D <= 32): the forward scan split into a CHAIN wave and a LOSS wave.
//
// Why: a lone wave issues one VALU instruction per ~5.4 cycles, two waves on one SIMD issue one per ~4.1 cycles
// combined (profiles/r1_ubench_two_waves.log), and at B = 1024 clips there is exactly one clip per SIMD.  The forward
// step has a serial part (u -> y = u + Q u + s R u -> |y|^2 -> u') and a part nothing waits for (H y, e = y^dagger H y,
// the stash row, the loss).  k_fwd_wave runs the second one step late inside the same wave; here it runs in a second
// wave that shares the SIMDs with the chain waves and fills their idle issue slots:
//
//   chain wave (waves 0-3 of the workgroup, raised priority): per step one mat-vec chain and the rotation of the
//     UN-normalised state z_k; writes z_k (256 B, split layout) into a ring in LDS; per 32-step chunk one power-of-two
//     rescale and publishes `prod` = chunks written.  The loss wave turns the rows into y_k = c_k z_k.
//   loss wave (waves 4-7): nothing waits for it, so it works a whole 32-step chunk at a time ON THE MATRIX CORES: the 32 rows
//     y_k of the chunk form Y [32 steps x 64 reals], and H Y^T is one real GEMM Y W (W = the 64 x 64 real form of
//     H = R + R^dagger) = 2 tiles x 4 k-steps of v_mfma_f32_32x32x16_bf16.  Both operands are split EXACTLY into three bf16
//     pieces (8 + 8 + 8 significand bits, by truncation) and six products per pair are accumulated in fp32
//     (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid: 24 operand bits, what is dropped is <= 2^-23 |a||b|), so H y_k is
//     fp32-faithful; 48 MFMAs per chunk replace 32 x 32 packed FMAs plus 9 LDS reads per step.  Then e_k = y_k . (H y_k)
//     (products transposed through LDS, column sums), the stash rows (y_k, H y_k), log(1 + e x / A) in the reference's
//     operation order and the sequential float32 loss accumulation (model.py:279, 294); publishes `cons`.
//
// One mat-vec on the chain, not two: y = ut + Q ut + s_k R ut = ut + M_k ut with M_k = Q + s_k R.  Forming M_k costs one
// packed FMA per complex entry (16 per lane) against the two a second mat-vec costs, and it does not depend on the state:
// M_{k+1} is formed in the shadow of step k's LDS broadcast, where the in-order wave would otherwise wait.
//
// Synchronisation is two LDS counters per clip and NO barrier: the ring holds two chunks; the loss wave starts chunk
// c when prod >= c + 1, the chain wave starts chunk c (c >= 2) when cons >= c - 1.  LDS operations of one wave
// complete in order, so a counter write issued after the chunk's data is visible after it.
// Same arithmetic as k_fwd_wave (cmps_wave.hip) up to rounding, same stash layouts (plus the normalised rows of the NORM instance, below:
// what the two-wave reverse scan reads by default).  Since round 6 the chain
// carries the UN-normalised state z_k and the loss wave normalises the rows it reads.
#include "cmps_wave_util.h"

namespace cmps {

namespace {

constexpr int CH2 = 32;          // steps per chunk (ring half, rho staging, per-chunk scalar math)
constexpr int RING = 2 * CH2;    // ring slots
constexpr int RLD = 68;          // floats per ring row: 64 (y_k as n = 2 i + {re, im}) + 4 of padding, so that the 32 rows the
                                 // loss wave reads at one column offset (ds_read_b128, 16-lane groups) fall into distinct banks
constexpr int PE2_LD = 36;       // row stride (floats) of the loss wave's product buffer [step][column]: 16-B aligned rows, the
                                 // 32 rows read at one offset fall into distinct banks

// this half's 16 entries of a ring row and the lane's own value
__device__ __forceinline__ void rows_own_issue(unsigned rd, unsigned own, v4f (&o)[8], float& mine) {
    asm volatile("ds_read_b128 %0, %9\n\tds_read_b128 %1, %9 offset:16\n\t"
                 "ds_read_b128 %2, %9 offset:32\n\tds_read_b128 %3, %9 offset:48\n\t"
                 "ds_read_b128 %4, %9 offset:64\n\tds_read_b128 %5, %9 offset:80\n\t"
                 "ds_read_b128 %6, %9 offset:96\n\tds_read_b128 %7, %9 offset:112\n\t"
                 "ds_read_b32 %8, %10"
                 : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]),
                   "=&v"(mine)
                 : "v"(rd), "v"(own) : "memory");
}
template <int N>
__device__ __forceinline__ void lds_wait_own9(v4f (&o)[8], float& mine) {
    asm volatile("s_waitcnt lgkmcnt(%9)"
                 : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]), "+v"(o[6]), "+v"(o[7]), "+v"(mine)
                 : "n"(N) : "memory");
}

// One mat-vec chain (this half's 16 columns of M u) with the wave reduction of `x` threaded through it: a lone in-order
// wave pays ~20 cycles per dependent DPP step, but nothing when four independent packed FMAs sit between two steps.
// After mv1r_hi, `tot` (SGPR) holds the sum of x over the 64 lanes.
#define DPPADD(ctrl) "v_add_f32_dpp %1, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void mv1r_lo(const v2f (&M)[16], const v4f (&q)[8], v2f& acc, float& x) {
    asm(CM_FIRST(0, 2, 10) CM(0, 3, 11) DPPADD("quad_perm:[1,0,3,2]")
        CM(0, 4, 12) CM(0, 5, 13) DPPADD("quad_perm:[2,3,0,1]")
        CM(0, 6, 14) CM(0, 7, 15) DPPADD("row_half_mirror")
        CM(0, 8, 16) CM(0, 9, 17) DPPADD("row_mirror")
        : "=&v"(acc), "+v"(x)
        : "v"(M[0]), "v"(M[1]), "v"(M[2]), "v"(M[3]), "v"(M[4]), "v"(M[5]), "v"(M[6]), "v"(M[7]),
          "v"(lo2(q[0])), "v"(hi2(q[0])), "v"(lo2(q[1])), "v"(hi2(q[1])), "v"(lo2(q[2])), "v"(hi2(q[2])),
          "v"(lo2(q[3])), "v"(hi2(q[3])));
}
__device__ __forceinline__ void mv1r_hi(const v2f (&M)[16], const v4f (&q)[8], v2f& acc, float& x, float& tot) {
    asm(CM(0, 3, 11) CM(0, 4, 12) CM(0, 5, 13)
        "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        CM(0, 6, 14) CM(0, 7, 15)
        "v_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        CM(0, 8, 16) CM(0, 9, 17)
        "v_readlane_b32 %2, %1, 63\n\t"
        CM(0, 10, 18)
        : "+v"(acc), "+v"(x), "=s"(tot)
        : "v"(M[8]), "v"(M[9]), "v"(M[10]), "v"(M[11]), "v"(M[12]), "v"(M[13]), "v"(M[14]), "v"(M[15]),
          "v"(lo2(q[4])), "v"(hi2(q[4])), "v"(lo2(q[5])), "v"(hi2(q[5])), "v"(lo2(q[6])), "v"(hi2(q[6])),
          "v"(lo2(q[7])), "v"(hi2(q[7])));
}
#undef DPPADD
// The serial tail of a chain step on ROTATED PARTIALS.  The mat-vec leaves in lane (i, h) the plain complex partial sum
// am = (M u)_i over K-half h.  The identity term joins it in the lane's own slot, G = am + mask u (mask = (1, 0) in half 0, (0, 1) in
// half 1: one packed FMA, behind the chain so that the 32 small products are not accumulated onto an O(1) seed); then
//     z_i     = G(half 0) + G(half 1)              -> split layout by ONE exchange + add   (the ring row)
//     rho z_i = G rho (half 0) + G rho (half 1)    -> split layout by ONE exchange + add   (the next broadcast)
// because the rotation is linear: it is applied to the partial pair of each lane, an ordinary complex product, BEFORE the halves are
// combined.  The two exchanges are independent of each other, and the state's path holds one of them where it held two (combine, then
// the partner component for the rotation), no select and no copies.
// v_permlane32_swap_b32 needs two wait states behind the VALU writes of its operands; each exchange's are the other path's work:
//     1 G  = v_pk_fma      2 Gr = v_pk_mul      3 Gr = v_pk_fma      4 swap G (written by 1: 2, 3 between)      5 z = v_add
//     6 swap Gr (written by 3: 4, 5 between)      7 ring write of z      8 u = v_add      9.. the broadcast of u
// ONE statement, the ring write and the broadcast (bcast_issue_tab_off, cmps_wave_util.h) included: hipcc pads a statement whose operands
// the statement before wrote with an s_nop, and it cannot see the distances above.  The exchange names the HALVES of the pairs G and Gr,
// which an operand cannot, so the two pairs are the fixed registers v[250:253], declared clobbered (the chain wave has them to spare).
// Outputs as bcast_issue_tab_off's, valid only after a matching lds_wait*; ROFF / TOFF: compile-time offsets on the ring / table address.
template <int ROFF, int TOFF>
__device__ __forceinline__ void rot_tail_bcast(v2f am, float u, v2f mask, unsigned ring, unsigned wr, unsigned rd, unsigned tab,
                                               float& z, float& un, v4f (&o)[8], v2f& rho) {
    const v2f u2 = __builtin_shufflevector(mk2(u, 0.f), mk2(u, 0.f), 0, -1);   // only the low half is read: the high half is left undefined
    // (rho: this step's entry in, the next step's out, in place: a second variable would be copied into the first at a loop's back-edge,
    // in front of the counted wait -- see bcast_issue_tab_sync, cmps_wave_util.h)
    asm volatile("v_pk_fma_f32 v[250:251], %12, %13, %11 op_sel_hi:[1,0,1]\n\t"
                 "v_pk_mul_f32 v[252:253], v[250:251], %8 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
                 "v_pk_fma_f32 v[252:253], v[250:251], %8, v[252:253] op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]\n\t"
                 "v_permlane32_swap_b32 v250, v251\n\t"
                 "v_add_f32 %9, v250, v251\n\t"
                 "v_permlane32_swap_b32 v252, v253\n\t"
                 "ds_write_b32 %14, %9 offset:%18\n\t"
                 "v_add_f32 %10, v252, v253\n\t"
                 "ds_write_b32 %15, %10\n\t"
                 "ds_read_b128 %0, %16\n\tds_read_b128 %1, %16 offset:16\n\t"
                 "ds_read_b128 %2, %16 offset:32\n\tds_read_b128 %3, %16 offset:48\n\t"
                 "ds_read_b128 %4, %16 offset:64\n\tds_read_b128 %5, %16 offset:80\n\t"
                 "ds_read_b128 %6, %16 offset:96\n\tds_read_b128 %7, %16 offset:112\n\t"
                 "ds_read_b64 %8, %17 offset:%19"
                 : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]),
                   "+v"(rho), "=&v"(z), "=&v"(un)
                 : "v"(am), "v"(mask), "v"(u2), "v"(ring), "v"(wr), "v"(rd), "v"(tab), "n"(ROFF), "n"(TOFF)
                 : "memory", "v250", "v251", "v252", "v253");
}
// wait for the second half of a broadcast; `dep` ties the wait behind the first FMA block (a plain asm statement the
// scheduler would otherwise be free to sink below this volatile one)
template <int N>
__device__ __forceinline__ void lds_wait_hi_t_after(v4f (&o)[8], v2f& t, v2f& dep) {
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(o[4]), "+v"(o[5]), "+v"(o[6]), "+v"(o[7]), "+v"(t), "+v"(dep) : "n"(N) : "memory");
}
}  // namespace

// Diagnostic builds only (scripts/ablate.py passes -DCMPS_DIAG -DCMPS_DIAG_NO_LOSS / -DCMPS_DIAG_NO_CHAIN; results are wrong,
// the timing tells what each wave costs alone).  tests/test_capi_load.py compiles both so that they cannot rot.
#if defined(CMPS_DIAG) && defined(CMPS_DIAG_NO_LOSS)
#define DIAG_NO_LOSS 1
#else
#define DIAG_NO_LOSS 0
#endif
#if defined(CMPS_DIAG) && defined(CMPS_DIAG_NO_CHAIN)
#define DIAG_NO_CHAIN 1
#else
#define DIAG_NO_CHAIN 0
#endif

// LEGACY: the arithmetic of the previous-generation AudioMPS (cmps_legacy.hip: the recurrence and its graph.pbtxt lines) on the same
// machinery.  With rho = 1 and psi_0 = e_0 in the tables (cmps_legacy_set_params) the chain is the same linear step,
// y_k = inv_{k-1} (y_{k-1} + M_k y_{k-1}), M_k = Q + dt x_k R; what differs is the loss wave: e_k = psi_k^dagger H psi_k is taken on the
// normalised state BEFORE the update, i.e. e_k = (y_{k-1}^dagger H y_{k-1}) / max(|y_{k-1}|^2, 1e-12) (e_0 = H_00), and
// loss += (x_k - e_k)^2 / 2.  The stash rows (y_k, H y_k) and the |y_k|^2 rows are the same; the e rows hold the legacy e_k.
// HF16 (round 5; what CMPS_RANK1_F16X2 / DEFAULT select for the PsiCMPS arithmetic): the loss wave's GEMM with two power-of-two scaled fp16
// pieces per operand and three products (hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16) instead of three bf16 pieces and six: the
// arithmetic of the wide family's k_hy_wide<f16x2>.  Scales: W from its largest entry (below 2^15), the chunk's y rows from
// the guaranteed bound |y_k|_2 <= 1 + |Q|_F + max_chunk |s_k| |R|_F (below 2^14); one exact multiply takes them out of the accumulators.
// NORM (with SAVE, PsiCMPS arithmetic): the stash rows are written NORMALISED for the two-wave reverse scan (STASH_WAVE32N,
// cmps_wave_bwd2.hip): (yhat_k[n], p_k[n]) with yhat_k = y_k inv_k, inv_k = rsq_newton(max(n_k, 1e-12)), p_k = 2 ebar_k (H y_k),
// ebar_k = -(x_k / A) / (1 + z_k) -- three multiplies per component and step that the reverse CHAIN wave would otherwise issue, done here
// where the most issue slots are free.  The rows are stored behind the e_k column sums and the per-chunk scalar stage (2 ebar_k needs e_k).
template <bool SAVE, bool LEGACY = false, bool HF16 = false, bool NORM = false>
__global__ __launch_bounds__(128 * WAVES, 1) void k_fwd_wave2(Dev Pk, const float* __restrict__ audio,
                                                              float* __restrict__ loss_out) {
    const Dev P = bank_view(Pk, blockIdx.y);                               // the member's workspace (a plain launch: Pk itself)
    audio += blockIdx.y * P.bank_audio;
    loss_out += blockIdx.y * P.bank_loss;
    // rho rows of the chain wave's chunk, two buffers (round 5): the next chunk's rows are fetched in two halves of 16 rows and committed
    // into the OTHER buffer while the current one is being read, so only 16 registers ride through the chunk instead of 32 -- with 32
    // hipcc spilled four of them to scratch memory and reloaded them behind an s_waitcnt vmcnt(0) at every chunk end (ISA of round 4)
    __shared__ __attribute__((aligned(16))) float4 stR[WAVES][2][CH2 * 16];
    __shared__ __attribute__((aligned(16))) float2 bcU[WAVES][DPW];
    __shared__ __attribute__((aligned(16))) float ring[WAVES][RING][RLD];   // y_k, n = 2 i + {re, im}, rows padded (RLD)
    __shared__ __attribute__((aligned(16))) float pe[WAVES][CH2 * PE2_LD]; // y_k[n] (H y_k)[n], [step][column]
    __shared__ int flags[WAVES][2];                                         // [clip][0: prod, 1: cons]
    __shared__ float esc[WAVES][4];                                         // 4^-e of the rescale entering chunk c, slot c & 3
    __shared__ __attribute__((aligned(16))) float cst[WAVES][CH2];          // loss wave: c_k of the chunk's rows (C/D layout reads)
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int w = wv & (WAVES - 1), role = wv / WAVES;
    const int i = lane & 31, h = lane >> 5;
    const bool hb = h != 0;
    if (threadIdx.x < 2 * WAVES) (&flags[0][0])[threadIdx.x] = 0;
    __syncthreads();
    const int b = blockIdx.x * WAVES + w;
    if (b >= P.B) return;      // both waves of the clip leave together
    const int N = P.N, T = P.T, NC2 = (N + CH2 - 1) / CH2, NC = (N + CH - 1) / CH;
    const float* xrow = audio + (size_t)b * T;
    const float A = dev_A(P);
    float* sc = SAVE ? P.scal + scal_off(b, NC, 0) : nullptr;
    const unsigned aRing = lds_addr(&ring[w][0][0]);
    constexpr int RROWB = RLD * 4;                                          // bytes per ring row
    const unsigned aProd = lds_addr(&flags[w][0]), aCons = lds_addr(&flags[w][1]);

    if (role == 0) {
        // ------------------------------------------------------------------ chain wave
        if (DIAG_NO_CHAIN) return;
        __builtin_amdgcn_s_setprio(3);
        stagger(w);
        v2f MR[16], MQ[16], MM[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            MR[m] = ld2(&P.R[i * DPW + 16 * h + m]);
            MQ[m] = ld2(&P.Q[i * DPW + 16 * h + m]);
        }
        const unsigned aUw = lds_addr(&bcU[w][0]) + i * 8 + h * 4, aUr = lds_addr(&bcU[w][0]) + h * 128;
        const unsigned aYw = aRing + i * 8 + h * 4;
        unsigned aRho = lds_addr(&stR[w][0][0]) + i * 8;
        const float4* rho4 = reinterpret_cast<const float4*>(P.rho);
        v4f sr[4];
        {
            v4f s8[8];
            stage_load<8>(rho4, 0, N, lane, s8);
            stage_commit<8>(stR[w][0], lane, s8);
        }
        float xa0 = lane < T ? xrow[lane] : 0.f;
        float xa1 = lane + 1 < T ? xrow[lane + 1] : 0.f;
        const float2 p0 = P.psi0[i];
        float u = hb ? p0.y : p0.x;
        const v2f hmask = hb ? mk2(0.f, 1.f) : mk2(1.f, 0.f);          // the lane's own slot of a complex partial (rot_tail)
        v4f qu[8];
        v2f rho;
        // The normalisation is linear, so the chain does not apply it at all: it carries the un-normalised product
        // z_k = zt_k + M_k zt_k, zt_k = rho_{k-1} z_{k-1} (zt_0 = psi_0), and the loss wave turns the rows back into
        // y_k = c_k z_k (c_k from |z_{k-1}|^2, see there).  What keeps z in fp32 range is one exact power-of-two rescale
        // 2^-e per chunk, entering the next chunk: e from |z|^2 of step CH2 - 3, whose wave reduction rides inside the FMA
        // blocks of step CH2 - 2 (the only step with one); 4^-e goes to the loss wave through esc[].
        float xsq = 0.f, mlate = 1.f;
        float sv = LEGACY ? P.dt * (xa1 - xa0) : (xa1 - xa0) / A;   // model.py:263, 303: s_k = x_k / A, one step per lane (legacy: dt x_k)
        // M_k = Q + s_k R (model.py:308-313 with the two products merged): one packed FMA per complex entry
#define FORM_M(S_)                                                                                            \
        {                                                                                                     \
            const float s_ = (S_);                                                                            \
            const v2f s2_ = mk2(s_, s_);                                                                      \
            _Pragma("unroll") for (int m = 0; m < 16; ++m) MM[m] = __builtin_elementwise_fma(MR[m], s2_, MQ[m]); \
        }
        FORM_M(rdlane(sv, 0))
        bcast_issue_tab_sync(aUw, aUr, u, aRho, qu, rho);
        for (int c = 0; c < NC2; ++c) {
            const int kbeg = c * CH2;
            const int cnt = (N - kbeg) < CH2 ? (N - kbeg) : CH2;
            const int cn = c + 1 < NC2 ? c + 1 : NC2 - 1;
            float4* nxt = stR[w][(c + 1) & 1];                         // the buffer the next chunk will read
            {
                stage_load<4>(rho4, cn * CH2, N, lane, sr);            // rows 0 .. 15 of the next chunk
                const int idx = cn * CH2 + lane;
                xa0 = idx < T ? xrow[idx] : 0.f;
                xa1 = idx + 1 < T ? xrow[idx + 1] : 0.f;
            }
            if (!DIAG_NO_LOSS && c >= 2)                              // the ring half about to be overwritten
                while (flag_load(aCons) < c - 1) __builtin_amdgcn_s_sleep(1);
            unsigned ay = aYw + (c & 1) * (CH2 * RROWB);
#define CHAIN_STEP(KK)                                                                                        \
            {                                                                                                 \
                const int kk_ = (KK);                                                                         \
                lds_wait_lo<5>(qu);                                                                           \
                v2f am;                                                                                       \
                mv1_lo(MM, qu, am);                                                                           \
                lds_wait_hi_t_after<0>(qu, rho, am);                                                          \
                mv1_hi(MM, qu, am);                                                                           \
                const int kn = kk_ + 1 < CH2 ? kk_ + 1 : 0;               /* chunk end: a dummy, retired below */ \
                float y, un;                                              /* z_k -> ring row; rho_k z_k -> broadcast */ \
                rot_tail_bcast<0, 0>(am, u, hmask, ay, aUw, aUr, aRho + kn * 256, y, un, qu, rho);            \
                ay += RROWB;                                                                                  \
                u = un;                                                                                       \
                FORM_M(rdlane(sv, kn))                                    /* in the shadow of the broadcast */ \
            }
            // a full chunk runs unrolled with compile-time step numbers: every LDS offset is an immediate, the lane selects of
            // v_readlane / v_writelane are constants (no M0 save / restore), no loop bookkeeping on the serial chain
#define CHAIN_STEPC(KK)                                                                                       \
            {                                                                                                 \
                lds_wait_lo<5>(qu);                                                                           \
                v2f am;                                                                                       \
                if constexpr ((KK) == CH2 - 2) {                          /* mlate = |z_{CH2-3}|^2 */         \
                    mv1r_lo(MM, qu, am, xsq);                                                                 \
                    lds_wait_hi_t_after<0>(qu, rho, am);                                                      \
                    mv1r_hi(MM, qu, am, xsq, mlate);                                                          \
                } else {                                                                                      \
                    mv1_lo(MM, qu, am);                                                                       \
                    lds_wait_hi_t_after<0>(qu, rho, am);                                                      \
                    mv1_hi(MM, qu, am);                                                                       \
                }                                                                                             \
                float y, un;                                                                                  \
                if constexpr ((KK) == CH2 - 1) {                          /* chunk end: the table read is a dummy, retired below. */ \
                    v2f rend = rho;                                       /* Into a register of its own: written into rho it would be */ \
                    rot_tail_bcast<(KK) * RROWB, 0>(am, u, hmask, ay, aUw, aUr, aRho, y, un, qu, rend);   /* copied where the two chunk */ \
                } else {                                                  /* paths join, in front of the wait */ \
                    rot_tail_bcast<(KK) * RROWB, ((KK) + 1) * 256>(am, u, hmask, ay, aUw, aUr, aRho, y, un, qu, rho); \
                }                                                                                             \
                u = un;                                                                                       \
                FORM_M(rdlane(sv, ((KK) + 1) & (CH2 - 1)))                                                    \
                if constexpr ((KK) == CH2 - 3) xsq = y * y;                                                   \
            }
            if (cnt == CH2) {
                CHAIN_STEPC(0) CHAIN_STEPC(1) CHAIN_STEPC(2) CHAIN_STEPC(3) CHAIN_STEPC(4) CHAIN_STEPC(5) CHAIN_STEPC(6) CHAIN_STEPC(7)
                stage_commit<4>(nxt, lane, sr);                        // (requested eight steps ago)
                stage_load<4>(rho4, cn * CH2 + 16, N, lane, sr);       // rows 16 .. 31
                CHAIN_STEPC(8) CHAIN_STEPC(9) CHAIN_STEPC(10) CHAIN_STEPC(11) CHAIN_STEPC(12) CHAIN_STEPC(13) CHAIN_STEPC(14)
                CHAIN_STEPC(15) CHAIN_STEPC(16) CHAIN_STEPC(17) CHAIN_STEPC(18) CHAIN_STEPC(19) CHAIN_STEPC(20) CHAIN_STEPC(21)
                CHAIN_STEPC(22) CHAIN_STEPC(23)
                stage_commit<4>(nxt + 4 * 64, lane, sr);
                CHAIN_STEPC(24) CHAIN_STEPC(25) CHAIN_STEPC(26) CHAIN_STEPC(27) CHAIN_STEPC(28)
                CHAIN_STEPC(29) CHAIN_STEPC(30) CHAIN_STEPC(31)
            } else {                                                   // the clip's last, partial chunk (nothing follows it)
                for (int kk = 0; kk < cnt; ++kk) CHAIN_STEP(kk)
            }
#undef CHAIN_STEPC
#undef CHAIN_STEP
            lds_wait_hi_t<0>(qu, rho);                                 // everything of this chunk has landed
            flag_store(aProd, c + 1, lane);                            // publish (ordered behind the chunk's y rows)
            if (c + 1 < NC2) {                                         // (chunk c was full: mlate is this chunk's)
                // rescale: |z|^2 -> [1, 4) near the chunk end.  e in [-60, 60] keeps 4^-e a normal float (m = 0, inf, NaN: clamped)
                int e = ((int)((__float_as_uint(mlate) >> 23) & 0xFFu) - 127) >> 1;
                e = e > 60 ? 60 : e < -60 ? -60 : e;
                u *= __uint_as_float((unsigned)(127 - e) << 23);
                if (lane == 0) esc[w][(c + 1) & 3] = __uint_as_float((unsigned)(127 - 2 * e) << 23);   // the loss wave is at chunk >= c - 1
                aRho = lds_addr(&stR[w][(c + 1) & 1][0]) + i * 8;     // both halves of the next chunk are in place
                sv = LEGACY ? P.dt * (xa1 - xa0) : (xa1 - xa0) / A;    // the next chunk's s_k
                FORM_M(rdlane(sv, 0))                                  // the last in-loop FORM_M used the stale lane 0
                bcast_issue_tab_sync(aUw, aUr, u, aRho, qu, rho);      // (its registers cross the back-edge: the wait sits inside)
            }
        }
#undef FORM_M
        return;
    }

    // ---------------------------------------------------------------------- loss wave
    if (DIAG_NO_LOSS) return;
    __builtin_amdgcn_s_setprio(0);
    auto frag = [](const unsigned (&f)[4]) { return __builtin_bit_cast(bf16x8, v4u{f[0], f[1], f[2], f[3]}); };
    // B operand: W[m][n], the real 64 x 64 form of H = R + R^dagger acting on (re, im)-interleaved vectors,
    //   (H y)[n = 2 i + c] = sum_m y[m = 2 j + c'] W[m][n]:  W = Hr_ij for c' = c,  -Hi_ij for (c', c) = (1, 0),  +Hi_ij for (0, 1).
    // Lane (col = lane & 31, hk = lane >> 5) holds W[16 s + 8 hk + e][32 t + col], e = 0..7, for tile t and k-step s.
    auto split2h = [](float fe, float fo, unsigned& H, unsigned& L) {           // two fp16 pieces, round to nearest (11 + 1 + 11 + 1 bits)
        const h2 hh = {(_Float16)fe, (_Float16)fo};                            // plain casts: hipcc must see who produces an MFMA operand
        const h2 ll = {(_Float16)(fe - (float)hh.x), (_Float16)(fo - (float)hh.y)};
        H = __builtin_bit_cast(unsigned, hh);
        L = __builtin_bit_cast(unsigned, ll);
    };
    // the same for the pair p * sc (sc a power of two): ONE packed multiply, and each residual as ONE v_fma_mix_f32 (p sc - hi, the fp16
    // half read in place); hipcc makes a v_cvt_f32_f16 + v_fma_f32 of the C form.  The asm results feed compiler-visible conversions, never
    // an MFMA directly, so the hazard of DESIGN 4.3e cannot arise.
    auto split2h_scaled = [](v2f p, float sc, unsigned& H, unsigned& L) {
        const v2f t = p * mk2(sc, sc);
        const h2 hh = {(_Float16)t.x, (_Float16)t.y};
        H = __builtin_bit_cast(unsigned, hh);
        float re, ro;
        asm("v_fma_mix_f32 %0, %2, %4, -%5 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mix_f32 %1, %3, %4, -%5 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "=&v"(re), "=&v"(ro) : "v"(p.x), "v"(p.y), "v"(sc), "v"(H));
        const h2 ll = {(_Float16)re, (_Float16)ro};
        L = __builtin_bit_cast(unsigned, ll);
    };
    auto fragh = [](const unsigned (&f)[4]) { return __builtin_bit_cast(h8, v4u{f[0], f[1], f[2], f[3]}); };
    unsigned WH[2][4][4], WM[HF16 ? 1 : 2][HF16 ? 1 : 4][4], WL[2][4][4];
    float sW = 1.f, Qn = 0.f, Rn = 0.f;              // HF16: scale of W; Frobenius norms of Q and R (the bound of |y_k|)
    {
        const int col = lane & 31, hk = lane >> 5;
        if constexpr (HF16) {
            float mw = 0.f, q2 = 0.f, r2 = 0.f;
            for (int idx = lane; idx < DPW * DPW; idx += 64) {
                const float2 r = P.R[idx], rt = P.RT[idx], q = P.Q[idx];
                mw = fmaxf(mw, fmaxf(fabsf(r.x + rt.x), fabsf(r.y - rt.y)));
                q2 += q.x * q.x + q.y * q.y;
                r2 += r.x * r.x + r.y * r.y;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mw = fmaxf(mw, __shfl_xor(mw, off, 64));
            Qn = 1.001f * sqrtf(sum64(q2));
            Rn = 1.001f * sqrtf(sum64(r2));
            // the largest power of two with max |W| sW < 2^15 (W = 0: any scale)
            int se = 15 - ((int)((__float_as_uint(fmaxf(mw, 1e-30f)) >> 23) & 0xFFu) - 126);
            se = se > 60 ? 60 : se < -60 ? -60 : se;
            sW = __uint_as_float((unsigned)(127 + se) << 23);
            sW = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sW)));
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = 32 * t + col, ii = n >> 1, cc = n & 1;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                float wv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int m = 16 * ks + 8 * hk + e, jj = m >> 1, cp = m & 1;
                    const float2 r = P.R[ii * DPW + jj], rt = P.RT[ii * DPW + jj];      // R[ii][jj], R[jj][ii]
                    const float hr = r.x + rt.x, hi = r.y - rt.y;                         // (R + R^dagger)[ii][jj]
                    wv[e] = cp == cc ? hr : (cc ? hi : -hi);
                }
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    if constexpr (HF16) split2h(wv[2 * e2] * sW, wv[2 * e2 + 1] * sW, WH[t][ks][e2], WL[t][ks][e2]);
                    else split3_pk(wv[2 * e2], wv[2 * e2 + 1], WH[t][ks][e2], WM[t][ks][e2], WL[t][ks][e2]);
                }
            }
        }
    }
    // A operand: lane (row = lane & 31 = step of the chunk, hk) reads y_k[16 s + 8 hk + e] from the ring;
    // C/D layout of a tile: column n = 32 t + (lane & 31), rows (steps) (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 0..15
    const int crow = lane & 31, chk = lane >> 5;
    const float* ringw = &ring[w][0][0];
    float* pew = &pe[w][0];
    float2* st = SAVE ? reinterpret_cast<float2*>(P.hst + (size_t)b * N * WAVE_ROW) : nullptr;   // rows of 64 (y[n], (H y)[n]) pairs
    float loss = 0.f;
    float f_below = 2.0f * P.R[0].x, n_below = 1.f;                    // LEGACY: y^dagger H y and |y|^2 of the step below the chunk (psi_0 = e_0)
    float m_below = 1.f, g_carry = 1.f;                                // |z|^2 of the step below the chunk (|psi_0|^2 = 1), g of the chunk's first step
    for (int c = 0; c < NC2; ++c) {
        const int kbeg = c * CH2;
        const int cnt = (N - kbeg) < CH2 ? (N - kbeg) : CH2;
        const int idx = kbeg + lane;
        const float x0 = idx < T ? xrow[idx] : 0.f;
        const float x1 = idx + 1 < T ? xrow[idx + 1] : 0.f;
        if (!DIAG_NO_CHAIN)
            while (flag_load(aProd) < c + 1) __builtin_amdgcn_s_sleep(8);     // a chunk takes ~20000 cycles: poll rarely
        const float* rh = ringw + (c & 1) * (CH2 * RLD);               // this chunk's 32 rows (rows >= cnt: stale, ignored below)
        // The rows are the chain's z_k; today's y_k = c_k z_k.  With m_k = |z_k|^2 and mt_k = |zt_k|^2 = m_{k-1} (times the chunk's 4^-e
        // on its first row; |rho| = 1 enters neither: model.py takes the norm before the rotation), the reference's
        // u_k = rho y_{k-1} / sqrt(max(n_{k-1}, 1e-12)) has |u_k|^2 = g_k = n_{k-1} / max(n_{k-1}, 1e-12) (1 but after a clip), so
        // c_k = sqrt(g_k / mt_k) and n_k = |y_k|^2 = c_k^2 m_k.  Lane (crow, chk) holds half of row crow in the A-operand layout below.
        float4 F[4][2];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            F[ks][0] = *reinterpret_cast<const float4*>(rh + crow * RLD + 16 * ks + 8 * chk);
            F[ks][1] = *reinterpret_cast<const float4*>(rh + crow * RLD + 16 * ks + 8 * chk + 4);
        }
        float ck, nk;
        {
            v2f s2 = mk2(0.f, 0.f);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const v2f a = mk2(F[ks][hf].x, F[ks][hf].y), b2 = mk2(F[ks][hf].z, F[ks][hf].w);
                    s2 = __builtin_elementwise_fma(a, a, s2);
                    s2 = __builtin_elementwise_fma(b2, b2, s2);
                }
            const float mk = swap32_add(s2.x + s2.y, s2.x + s2.y);            // m_k of row crow (both halves)
            float mt = __shfl_up(mk, 1, 64);
            if (crow == 0) mt = c ? m_below * esc[w][c & 3] : m_below;
            m_below = rdlane(mk, CH2 - 1);                                  // (a partial chunk is the clip's last)
            ck = __builtin_amdgcn_rsqf(mt);                                 // g_k = 1
            nk = ck * ck * mk;
            if (g_carry != 1.f || __ballot(crow < cnt && !(nk >= 1e-12f))) {
                // the 1e-12 floor clipped (model.py:331-334), or a zero state: g_k step by step (rare; uniform branch)
                float g = g_carry;
                for (int j = 0; j < cnt; ++j) {
                    const float mtj = rdlane(mt, j), mj = rdlane(mk, j);
                    const float cj = mtj > 0.f ? sqrtf(g) * __builtin_amdgcn_rsqf(mtj) : 0.f;
                    const float nj = cj * cj * mj;
                    if (crow == j) { ck = cj; nk = nj; }
                    g = nj >= 1e-12f ? 1.f : nj / 1e-12f;
                }
                g_carry = g;
            }
        }
        if (lane < CH2) cst[w][lane] = ck;
        v16f acc0 = {}, acc1 = {};
        float sY = 1.f, unsc = 1.f;
        if constexpr (HF16) {
            // the chunk's rows: |y_k|_inf <= |y_k|_2 <= 1 + |Q|_F + |s_k| |R|_F (inv_{k-1} |ut| <= 1); s_k of this chunk sits one step per lane
            float smax = fabsf((x1 - x0) / A);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) smax = fmaxf(smax, __shfl_xor(smax, off, 64));
            const float bnd = 1.001f * (1.0f + Qn + smax * Rn);
            int se = 14 - ((int)((__float_as_uint(bnd) >> 23) & 0xFFu) - 126);
            se = se > 60 ? 60 : se < -60 ? -60 : se;
            sY = __uint_as_float(__builtin_amdgcn_readfirstlane((unsigned)(127 + se) << 23));
            unsc = __uint_as_float(0x7F000000u - __float_as_uint(sY)) * __uint_as_float(0x7F000000u - __float_as_uint(sW));   // exact 1 / (sY sW)
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            float4 f0 = F[ks][0], f1 = F[ks][1];
            if constexpr (HF16) {
                // the operand is y_k sY = z_k (c_k sY): c_k enters the split's one multiply (the bound above is one of |y_k|)
                const float scA = ck * sY;
                unsigned AH[4], AL[4];
                split2h_scaled(mk2(f0.x, f0.y), scA, AH[0], AL[0]);
                split2h_scaled(mk2(f0.z, f0.w), scA, AH[1], AL[1]);
                split2h_scaled(mk2(f1.x, f1.y), scA, AH[2], AL[2]);
                split2h_scaled(mk2(f1.z, f1.w), scA, AH[3], AL[3]);
#define MF3(ACC, T_)                                                                                           \
                ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(fragh(AH), fragh(WH[T_][ks]), ACC, 0, 0, 0);      \
                ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(fragh(AH), fragh(WL[T_][ks]), ACC, 0, 0, 0);      \
                ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(fragh(AL), fragh(WH[T_][ks]), ACC, 0, 0, 0);
                MF3(acc0, 0)
                MF3(acc1, 1)
#undef MF3
            } else {
            f0.x *= ck; f0.y *= ck; f0.z *= ck; f0.w *= ck; f1.x *= ck; f1.y *= ck; f1.z *= ck; f1.w *= ck;   // y_k
            unsigned AH[4], AM[4], AL[4];
            split3_pk(f0.x, f0.y, AH[0], AM[0], AL[0]);
            split3_pk(f0.z, f0.w, AH[1], AM[1], AL[1]);
            split3_pk(f1.x, f1.y, AH[2], AM[2], AL[2]);
            split3_pk(f1.z, f1.w, AH[3], AM[3], AL[3]);
#define MF6(ACC, T_)                                                                                           \
            ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(AH), frag(WH[T_][ks]), ACC, 0, 0, 0);           \
            ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(AH), frag(WM[HF16 ? 0 : T_][HF16 ? 0 : ks]), ACC, 0, 0, 0);           \
            ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(AM), frag(WH[T_][ks]), ACC, 0, 0, 0);           \
            ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(AH), frag(WL[T_][ks]), ACC, 0, 0, 0);           \
            ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(AL), frag(WH[T_][ks]), ACC, 0, 0, 0);           \
            ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(AM), frag(WM[HF16 ? 0 : T_][HF16 ? 0 : ks]), ACC, 0, 0, 0);
            MF6(acc0, 0)
            MF6(acc1, 1)
#undef MF6
            }
        }
        if constexpr (HF16) {                                          // packed: one v_pk_mul_f32 per two accumulator registers
            const v2f u2 = mk2(unsc, unsc);
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const v2f a = mk2(acc0[r], acc0[r + 1]) * u2, b2 = mk2(acc1[r], acc1[r + 1]) * u2;
                acc0[r] = a.x; acc0[r + 1] = a.y; acc1[r] = b2.x; acc1[r + 1] = b2.y;
            }
        }
        // y_k[n] in the C/D layout (c_k of the register's step from cst: steps 8 G + 4 chk + 0..3 in one read), products y (H y), stash rows
        float yc0[16], yc1[16], pr[16];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float4 cg = *reinterpret_cast<const float4*>(&cst[w][8 * g4 + 4 * chk]);
            const float cr[4] = {cg.x, cg.y, cg.z, cg.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * g4 + q, stp = q + 8 * g4 + 4 * chk;
                yc0[r] = cr[q] * rh[stp * RLD + crow];
                yc1[r] = cr[q] * rh[stp * RLD + 32 + crow];
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) pr[r] = yc0[r] * acc0[r] + yc1[r] * acc1[r];
        float pn[LEGACY ? 16 : 1];
        if constexpr (LEGACY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) pn[r] = yc0[r] * yc0[r] + yc1[r] * yc1[r];
        }
        // (a macro, not a lambda: the (y, H y) instances keep the instruction stream they had)
        // Stash row (kbeg + step) = 64 pairs (y[n], (H y)[n]) = 512 contiguous bytes.  Register r holds step s0 = (r & 3) +
        // 8 (r >> 2) in lanes 0-31 and step s0 + 4 in lanes 32-63, for n = 0..31 (tile 0) and n = 32..63 (tile 1): one
        // v_permlane32_swap between the two tiles puts ALL of row s0 into one register and all of row s0 + 4 into the
        // other, so every store instruction writes one whole row (lane = n).
        // A full chunk (all but a clip's last): address = uniform base (SGPR pair, one per eight rows: the immediate reaches 4095) + this
        // lane's 8 bytes (one VGPR for the whole kernel) + the row's immediate -- no 64-bit VALU address arithmetic and no per-row test.
        // (Stores by asm: dwordx2 data has no write-after-store hazard; nothing in this kernel reads the rows back.)
#define FWD2_STORE_ROWS                                                                                                                             \
            char* cbase = reinterpret_cast<char*>(st + (size_t)kbeg * WAVE_ROW_PAIRS);                                                              \
            const unsigned loff = (unsigned)lane * 8u;                                                                                              \
            if (cnt == CH2) {                                                                                                                       \
                _Pragma("unroll")                                                                                                                   \
                for (int r = 0; r < 16; ++r) {                                                                                                      \
                    const int s0 = (r & 3) + 8 * (r >> 2);                                                                                          \
                    const auto ys = __builtin_amdgcn_permlane32_swap(__float_as_uint(yc0[r]), __float_as_uint(yc1[r]), false, false);               \
                    const auto hs = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc0[r]), __float_as_uint(acc1[r]), false, false);             \
                    const v2f lo = mk2(__uint_as_float(ys[0]), __uint_as_float(hs[0])), hi = mk2(__uint_as_float(ys[1]), __uint_as_float(hs[1]));   \
                    const char* q0 = cbase + (s0 >> 3) * 4096;                                                                                      \
                    asm volatile("global_store_dwordx2 %0, %1, %2 offset:%3" :: "v"(loff), "v"(lo), "s"(q0), "n"((s0 & 7) * 512) : "memory");       \
                    asm volatile("global_store_dwordx2 %0, %1, %2 offset:%3" :: "v"(loff), "v"(hi), "s"(q0), "n"(((s0 + 4) & 7) * 512) : "memory"); \
                }                                                                                                                                   \
            } else {                                                                                                                                \
                _Pragma("unroll")                                                                                                                   \
                for (int r = 0; r < 16; ++r) {                                                                                                      \
                    const int s0 = (r & 3) + 8 * (r >> 2);                                                                                          \
                    const auto ys = __builtin_amdgcn_permlane32_swap(__float_as_uint(yc0[r]), __float_as_uint(yc1[r]), false, false);               \
                    const auto hs = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc0[r]), __float_as_uint(acc1[r]), false, false);             \
                    if (s0 < cnt)                                                                                                                   \
                        *reinterpret_cast<float2*>(cbase + s0 * 512 + loff) = make_float2(__uint_as_float(ys[0]), __uint_as_float(hs[0]));          \
                    if (s0 + 4 < cnt)                                                                                                               \
                        *reinterpret_cast<float2*>(cbase + (s0 + 4) * 512 + loff) = make_float2(__uint_as_float(ys[1]), __uint_as_float(hs[1]));    \
                }                                                                                                                                   \
            }
        if (SAVE && !NORM) { FWD2_STORE_ROWS }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        flag_store(aCons, c + 1, lane);                                // every ring read has landed: the half is free
        // e_k = sum_n y_k[n] (H y_k)[n]: transpose the per-column products through LDS, then lane (k, hh) sums columns
        // 16 hh .. 16 hh + 15 of row k and the two halves are added
#pragma unroll
        for (int r = 0; r < 16; ++r) pew[((r & 3) + 8 * (r >> 2) + 4 * chk) * PE2_LD + crow] = pr[r];
        __builtin_amdgcn_wave_barrier();
        float evec;
        {
            const float4* rowp = reinterpret_cast<const float4*>(pew + crow * PE2_LD + 16 * chk);
            const float4 q0 = rowp[0], q1 = rowp[1], q2 = rowp[2], q3 = rowp[3];
            const float part = ((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w)) +
                               (((q2.x + q2.y) + (q2.z + q2.w)) + ((q3.x + q3.y) + (q3.z + q3.w)));
            evec = swap32_add(part, part);
        }
        __builtin_amdgcn_wave_barrier();
        const float incv = x1 - x0;
        float lv;
        if constexpr (LEGACY) {
            // |y_k|^2 the same way, then the expectation on the normalised state of the step below
            float nvec2;
#pragma unroll
            for (int r = 0; r < 16; ++r) pew[((r & 3) + 8 * (r >> 2) + 4 * chk) * PE2_LD + crow] = pn[r];
            __builtin_amdgcn_wave_barrier();
            {
                const float4* rowp = reinterpret_cast<const float4*>(pew + crow * PE2_LD + 16 * chk);
                const float4 q0 = rowp[0], q1 = rowp[1], q2 = rowp[2], q3 = rowp[3];
                const float part = ((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w)) +
                                   (((q2.x + q2.y) + (q2.z + q2.w)) + ((q3.x + q3.y) + (q3.z + q3.w)));
                nvec2 = swap32_add(part, part);
            }
            __builtin_amdgcn_wave_barrier();
            float fb = __shfl_up(evec, 1, 64), nb = __shfl_up(nvec2, 1, 64);       // lanes k and k + 32 both hold step k
            if (crow == 0) { fb = f_below; nb = n_below; }
            f_below = rdlane(evec, CH2 - 1);
            n_below = rdlane(nvec2, CH2 - 1);
            const float invb = 1.0f / sqrtf(fmaxf(nb, 1e-12f));       // graph.pbtxt:14350-14594
            evec = (fb * invb) * invb;                                 // e_k = psi_k^dagger (R + R^T) psi_k  (:11857-12661)
            const float d = incv - evec;
            lv = d * d / 2.0f;                                         // :12685-12819
        } else {
            const float z = (evec * incv) / A;                         // model.py:294 operation order
            lv = -logf(1.0f + z);
            if constexpr (SAVE && NORM) {
                // the per-row factors in the reverse scan's own operations (cmps_wave_bwd2.hip::scal_commit), so that yhat and p are
                // bit for bit what its pre stage formed from (y, H y) rows; to the C/D-layout registers the way c_k went: an LDS row each
                // (cst is free since the y rows were formed, pe since the column sums were read) and one 16-byte read per four steps
                const float invk = rsq_newton(fmaxf(nk, 1e-12f));
                const float zbar = -1.0f / (1.0f + z);
                const float tev = 2.0f * (zbar * incv / A);
                __builtin_amdgcn_wave_barrier();
                if (lane < CH2) { cst[w][lane] = invk; pew[lane] = tev; }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 ig = *reinterpret_cast<const float4*>(&cst[w][8 * g4 + 4 * chk]);
                    const float4 tg = *reinterpret_cast<const float4*>(&pew[8 * g4 + 4 * chk]);
                    const v2f i01 = mk2(ig.x, ig.y), i23 = mk2(ig.z, ig.w), t01 = mk2(tg.x, tg.y), t23 = mk2(tg.z, tg.w);
#pragma unroll
                    for (int q = 0; q < 4; q += 2) {
                        const int r = 4 * g4 + q;
                        const v2f iv = q ? i23 : i01, tv = q ? t23 : t01;
                        const v2f a = mk2(yc0[r], yc0[r + 1]) * iv, b2 = mk2(yc1[r], yc1[r + 1]) * iv;
                        const v2f p0 = mk2(acc0[r], acc0[r + 1]) * tv, p1 = mk2(acc1[r], acc1[r + 1]) * tv;
                        yc0[r] = a.x; yc0[r + 1] = a.y; yc1[r] = b2.x; yc1[r + 1] = b2.y;
                        acc0[r] = p0.x; acc0[r + 1] = p0.y; acc1[r] = p1.x; acc1[r + 1] = p1.y;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                FWD2_STORE_ROWS
            }
        }
        if (cnt == CH2) {                                              // model.py:279: sequential in time.  A full chunk unrolled: the lane
#pragma unroll                                                         // selects are immediates (v_readlane + v_add per step; the counted loop
            for (int j = 0; j < CH2; ++j) loss += rdlane(lv, j);       // below costs eight instructions per step)
        } else {
            for (int j = 0; j < cnt; ++j) loss += rdlane(lv, j);
        }
        if (SAVE && lane < CH2) {
            sc[(size_t)(c >> 1) * SCAL_ROW + (c & 1) * CH2 + lane] = nk;                // n_k = |y_k|^2
            sc[(size_t)(c >> 1) * SCAL_ROW + SCAL_E + (c & 1) * CH2 + lane] = evec;
        }
    }
#undef FWD2_STORE_ROWS
    if (lane == 0) loss_out[b] = loss;
}

// norm_rows: write STASH_WAVE32N rows (the caller asks for them only with save and hf16: the two-wave reverse scan's settings)
hipError_t launch_fwd_wave2(const Dev& P, const float* audio, float* loss, bool save, bool hf16, bool norm_rows, hipStream_t s, int M) {
    const unsigned nb = (unsigned)((P.B + WAVES - 1) / WAVES);
    if (norm_rows) {
        if (!save || !hf16) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_fwd_wave2<true, false, true, true>), dim3(nb, M), dim3(128 * WAVES), 0, s, P, audio, loss);
        return hipGetLastError();
    }
    return dispatch_bool(save, [&](auto sv) {
        return dispatch_bool(hf16, [&](auto hf) {
            hipLaunchKernelGGL((k_fwd_wave2<decltype(sv)::value, false, decltype(hf)::value>), dim3(nb, M), dim3(128 * WAVES), 0, s, P, audio, loss);
            return hipGetLastError();
        });
    });
}

hipError_t launch_fwd_legacy_wave(const Dev& P, const float* audio, float* loss, bool save, hipStream_t s) {
    const unsigned nb = (unsigned)((P.B + WAVES - 1) / WAVES);
    if (save)
        hipLaunchKernelGGL((k_fwd_wave2<true, true>), dim3(nb), dim3(128 * WAVES), 0, s, P, audio, loss);
    else
        hipLaunchKernelGGL((k_fwd_wave2<false, true>), dim3(nb), dim3(128 * WAVES), 0, s, P, audio, loss);
    return hipGetLastError();
}

}  // namespace cmps
