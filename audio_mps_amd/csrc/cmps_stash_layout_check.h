// Compile-time checks of cmps_stash_layout.h and of the section sizes make_layout / make_rho_layout take from it: no run-time code.
// Included by cmps_capi.hip alone and evaluated in its host pass, so the checks cost one host compile and no device pass.
#pragma once
#include "cmps_internal.h"

#ifndef __HIP_DEVICE_COMPILE__
namespace cmps {
namespace layout_check {

// f maps 0 .. n - 1 one to one into 0 .. SIZE - 1
template <int SIZE, typename F>
constexpr bool injective(int n, F f) {
    bool seen[SIZE] = {};
    for (int j = 0; j < n; ++j) {
        const int p = f(j);
        if (p < 0 || p >= SIZE || seen[p]) return false;
        seen[p] = true;
    }
    return true;
}

// ---- scalar rows: n and e of the 64 steps of a chunk fill the row, chunks and clips follow one another ----
static_assert(injective<SCAL_ROW>(2 * SCAL_STEPS, [](int j) { return (int)(j < SCAL_STEPS ? scal_n(0, j) : scal_e(0, j - SCAL_STEPS)); }), "scalar row");
static_assert(scal_n(1, 0) == SCAL_ROW && scal_off(0, 7, 1) == SCAL_ROW && scal_off(1, 7, 0) == 7 * SCAL_ROW, "scalar row strides");
static_assert(scal_chunks(64) == 1 && scal_chunks(65) == 2, "scalar chunks");

// ---- wave rows: (component, re | im, y | H y) fills the 128 floats in either order: y and H y do not overlap ----
static_assert(injective<WAVE_ROW>(WAVE_ROW, [](int j) { return wave16_pos(j & 31, (j >> 5) & 1, j >> 6); }), "wave16 row");
static_assert(injective<WAVE_ROW>(WAVE_ROW, [](int j) { return wave32_pos(j & 31, (j >> 5) & 1, j >> 6); }), "wave32 row");
static_assert(WAVE_ROW == 2 * WAVE_ROW_PAIRS && WAVE_ROW == 4 * WAVE_ROW_QUADS, "wave row units");
static_assert(wave_row(0, 9, 1) == WAVE_ROW && wave_row(1, 9, 0) == 9 * WAVE_ROW && wave_row(1, 9, 2, 5, 3) == ((9 + 2) * 5 + 3) * WAVE_ROW, "wave row strides");
static_assert(2 * wave_clip_pair(3, 9, 5) == wave_row(3, 9, 0, 5), "wave row bases");
// the float2 a lane of the wave kernels owns: lane = i + 32 im (WAVE16, RHO_STASH_WAVE), 2 i + im (WAVE32, WAVE32N, RHO_STASH_MFMA)
constexpr bool wave_lanes() {
    for (int i = 0; i < 32; ++i)
        for (int im = 0; im < 2; ++im)
            if (wave16_pos(i, im, 0) != 2 * (i + 32 * im) || wave32_pos(i, im, 0) != 2 * (2 * i + im) || wave16_pos(i, im, 1) != wave16_pos(i, im, 0) + 1 ||
                wave32_pos(i, im, 1) != wave32_pos(i, im, 0) + 1)
                return false;
    return true;
}
static_assert(wave_lanes(), "wave row lanes");

// ---- wide and pair vectors ----
template <int PD>
constexpr bool vectors() {
    constexpr int VF = vec_floats(PD), N = 3;
    if (!injective<VF>(VF, [](int j) { return wide_pos(j % PD, (j / PD) & 1, j / (2 * PD)); })) return false;
    if (!injective<VF>(VF, [](int j) { return pair_pos(PD, j % PD, (j / PD) & 1, j / (2 * PD)); })) return false;
    // y | H y of a step, the steps of a pair and the pairs follow one another without overlap
    if (wide_stash_vec(PD, 0, N, 0, 1) != (size_t)VF || wide_stash_vec(PD, 0, N, 1, 0) != (size_t)stash_step_floats(PD) ||
        wide_stash_vec(PD, 1, N, 0, 0) != (size_t)N * stash_step_floats(PD))
        return false;
    if (wide_ybar_vec(PD, 0, N, 1) != (size_t)ybar_step_floats(PD) || wide_ybar_vec(PD, 1, N, 0) != (size_t)N * ybar_step_floats(PD)) return false;
    if (stash_step_bytes(PD) != stash_step_floats(PD) * (int)sizeof(float) || ybar_step_bytes(PD) != ybar_step_floats(PD) * (int)sizeof(float)) return false;
    // the pair family's indices are the vector plus the position inside it
    for (size_t pair = 0; pair < 2; ++pair)
        for (int step = 0; step < N; ++step)
            for (int clip = 0; clip < 2; ++clip)
                for (int comp = 0; comp < 2; ++comp)
                    for (int row = 0; row < PD; ++row) {
                        for (int yh = 0; yh < 2; ++yh)
                            if (pair_stash_index<PD>(pair, N, step, yh, clip, comp, row) != wide_stash_vec(PD, pair, N, step, yh) + pair_pos(PD, row, comp, clip))
                                return false;
                        if (pair_ybar_index<PD>(pair, N, step, clip, comp, row) != wide_ybar_vec(PD, pair, N, step) + pair_pos(PD, row, comp, clip)) return false;
                    }
    // k_grad_gemm's build threads: thread tid holds (row, clip) = (8 (tid / 16) + tid % 8, (tid / 8) % 2)
    for (int tid = 0; tid < 2 * PD; ++tid)
        for (int c = 0; c < 2; ++c) {
            const int row = 8 * (tid >> 4) + (tid & 7), clip = (tid >> 3) & 1;
            if (wide_pos_thread(tid, c) != wide_pos(row, c, clip) || pair_pos_thread(PD, tid, c) != pair_pos(PD, row, c, clip)) return false;
        }
    // the wide kernels' own lane: thread 64 w + lane holds position 64 w + lane, row 16 w + (lane & 7) + 8 (lane >> 5), component (lane >> 4) & 1,
    // clip (lane >> 3) & 1
    for (int t = 0; t < VF; ++t) {
        const int w = t >> 6, lane = t & 63;
        if (wide_pos(16 * w + (lane & 7) + 8 * (lane >> 5), (lane >> 4) & 1, (lane >> 3) & 1) != t) return false;
    }
    return true;
}
static_assert(vectors<64>() && vectors<96>() && vectors<128>(), "wide and pair vectors");

// RhoCMPS on the wide kernels: (clip, column) -> (virtual pair, clip bit) is one to one for an even vrank
constexpr bool rho_wide_map(int B, int vrank) {
    for (int b = 0; b < B; ++b)
        for (int a = 0; a < vrank; ++a)
            if (2 * rho_wide_pair(b, vrank, a) + rho_wide_clip(a) != (size_t)b * vrank + a) return false;
    return true;
}
static_assert(rho_wide_map(3, 4) && rho_wide_map(5, 6), "virtual pairs");

// ---- section sizes: the last row of the last (clip, step) ends inside the section make_layout / make_rho_layout provide ----
constexpr bool fits(size_t floats_end, size_t elem, size_t from, size_t to) { return floats_end * elem <= to - from; }

constexpr bool psi_sections(int D, int B, int T) {
    const Layout L = make_layout(D, B, T, WS_TRAIN);
    const int DP = L.DP, N = L.N, NC = (int)scal_chunks(N);
    const size_t pairs = pairs_of(B), F = sizeof(float);
    if (!fits(scal_off(B - 1, NC, NC - 1) + SCAL_ROW, F, L.off_scal, L.off_slabs)) return false;
    if (!fits(block_row_pair(B - 1, N, N - 1, DP) + DP, sizeof(float2), L.off_stash, L.off_scal)) return false;
    if (D <= 32) return fits(wave_row(B - 1, N, N - 1) + WAVE_ROW, F, L.off_hst, L.off_scal);
    return fits(wide_stash_vec(DP, pairs - 1, N, N - 1, 1) + vec_floats(DP), F, L.off_stash, L.off_scal) &&
           fits(wide_ybar_vec(DP, pairs - 1, N, N - 1) + vec_floats(DP), F, L.off_gops, L.off_opmax);
}
constexpr bool rho_sections(int D, int rank, int B, int T) {
    const RhoLayout L = make_rho_layout(D, rank, B, T, WS_TRAIN);
    const int DP = padded_D(D), N = T - 1, NC = (int)scal_chunks(N), r = rank, vr = L.vrank;
    const size_t F = sizeof(float);
    if (!fits(scal_off(B - 1, NC, NC - 1) + SCAL_ROW, F, L.off_scal, L.off_slabs)) return false;
    if (!fits(2 * block_row_pair(B - 1, N, N - 1, DP, r, r - 1) + rho_row_floats(RHO_STASH_BLOCK, DP), F, L.off_stash, L.off_scal)) return false;
    if (D <= 32) return fits(wave_row(B - 1, N, N - 1, r, r - 1) + rho_row_floats(RHO_STASH_WAVE, DP), F, L.off_stash, L.off_scal) && rho_row_floats(RHO_STASH_MFMA, DP) == WAVE_ROW;
    if (vr == 0) return false;                                      // the wide path exists for every shape checked here
    return fits(wide_stash_vec(DP, rho_wide_pair(B - 1, vr, vr - 1), N, N - 1, 1) + rho_row_floats(RHO_STASH_WIDE, DP), F, L.off_vstash, L.off_vgops) &&
           fits(wide_ybar_vec(DP, rho_wide_pair(B - 1, vr, vr - 1), N, N - 1) + vec_floats(DP), F, L.off_vgops, L.off_vopmax) &&
           fits(scal_off(B * vr - 1, NC, NC - 1) + SCAL_ROW, F, L.off_vscal, L.off_rscal) &&
           fits(scal_off(B - 1, NC, NC - 1) + SCAL_ROW, F, L.off_rscal, L.off_vslabs);
}
// odd batches, D = 33, 72, 128 (and the wave kernels' 8, 32), an odd rank, step counts on both sides of a chunk boundary
constexpr bool sections() {
    for (int B : {1, 3, 5})
        for (int T : {2, 65, 66, 130})
            for (int D : {8, 32, 33, 72, 128}) {
                if (!psi_sections(D, B, T)) return false;
                for (int rank : {1, 3, 5})
                    if (!rho_sections(D, rank, B, T)) return false;
            }
    return true;
}
static_assert(sections(), "stash, ybar and scalar sections");

}  // namespace layout_check
}  // namespace cmps
#endif
