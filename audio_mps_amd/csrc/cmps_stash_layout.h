// The rows a forward scan leaves in the workspace for the kernels that follow it -- the stash (y_k and H y_k of every step), the ybar rows
// of the gradient GEMM and the scalar rows (n_k, e_k) -- stated once: geometry constants, address functions and section sizes.  The
// writers, the reverse scans, k_grad_gemm and the read-out kernels take their addresses from here; make_layout / make_rho_layout
// (cmps_internal.h) take the section bytes.  cmps_stash_layout_check.h holds the compile-time checks (one host compile, cmps_capi.hip).
//
// The functions are plain integer arithmetic in the algebraic shape of the hot kernels' expressions: a function called with step 0,
// yh 0 or column 0 folds to the base of that clip, pair or row.  Offsets are in floats unless a name says pairs (float2) or bytes.
// The scan kernels and the gradient GEMM must keep their instructions, and in some of them a call moves instructions even where it
// inlines to the very expression it replaces (k_fwd_wave16, k_fwd_wave2, k_fwd_rho_mfma, k_bwd_rho_wave, k_bwd_rho, k_loss_wide and the
// pair kernels: scripts/isa_identity.py).  There the kernel keeps its expression and writes it with the constants below, so a changed
// row size still reaches it; a changed position formula has to be carried to those sites by hand.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace cmps {

#define CMPS_LAYOUT_FN __host__ __device__ __forceinline__ constexpr

// Which family's forward wrote the stash (Dev::stash_layout): plain ints, so that the field and the kernels' comparisons stay what they were
enum StashLayout : int {
    STASH_BLOCK = 0,     // stash [B][N][DP] float2 (cmps_block.hip)
    STASH_WAVE16 = 1,    // hst rows in lane order (cmps_wave16.hip)
    STASH_PAIR = 2,      // pair rows (cmps_pair.hip)
    STASH_WAVE32 = 3,    // hst rows of (y[n], (H y)[n]) pairs, n = 2 i + {re, im} (cmps_wave2.hip)
    STASH_WIDE = 4,      // wide rows (cmps_wide.hip): [pair][step][y | H y][wave][lane] float
    STASH_WAVE32N = 5,   // hst rows of (yhat[n], p[n]) pairs in STASH_WAVE32's positions: yhat_k = y_k / sqrt(max(n_k, 1e-12)), p_k = 2 ebar_k (H y_k)
                         // (cmps_wave2.hip, for k_bwd_wave2w alone; n_k in the scalar rows turns yhat back into y, H y is not recoverable)
};
// Which forward (or sampler) wrote the rho stash (RhoDev::stash_layout)
enum RhoStashLayout : int {
    RHO_STASH_BLOCK = 0,   // [B][N][rank][DP] float2 (cmps_rho.hip)
    RHO_STASH_WAVE = 1,    // [B][N][rank][64] (y own, H y own) (cmps_rho_wave.hip)
    RHO_STASH_MFMA = 2,    // [B][N][rank][64] pairs (y[n], (H y)[n]), n = 2 i + {re, im} (cmps_rho_mfma.hip)
    RHO_STASH_WIDE = 3,    // the wide kernels' rows, one vector per PAIR of columns: vstash [(b vrank + a) / 2][N][y | H y][4 DP] (cmps_wide.hip)
};

// ---- scalar rows: [B][NC][2][64] float, per clip and 64-step chunk n_k in floats 0..63 and e_k in 64..127, one step per lane ----
constexpr int SCAL_STEPS = 64;    // steps per chunk
constexpr int SCAL_ROW = 128;     // floats per (clip, chunk)
constexpr int SCAL_E = 64;        // first float of e
CMPS_LAYOUT_FN size_t scal_chunks(size_t N) { return (N + SCAL_STEPS - 1) / SCAL_STEPS; }
CMPS_LAYOUT_FN size_t scal_off(int b, int NC, int c) { return ((size_t)b * NC + c) * SCAL_ROW; }            // the row of (clip, chunk)
CMPS_LAYOUT_FN size_t scal_n(int c, int j) { return (size_t)c * SCAL_ROW + j; }                         // from a clip's chunk 0: n of step 64 c + j
CMPS_LAYOUT_FN size_t scal_e(int c, int j) { return (size_t)c * SCAL_ROW + SCAL_E + j; }                // ... and e
CMPS_LAYOUT_FN size_t scal_bytes(size_t B, size_t N) { return B * scal_chunks(N) * SCAL_ROW * sizeof(float); }

// ---- wave rows (hst; D <= 32): [B][N][64] pairs (y, H y), 512 B per step.  RhoCMPS on virtual clips and the RhoCMPS wave / MFMA kernels
// keep [B][N][vr][64]: column av of clip b, vr columns per step ----
constexpr int WAVE_ROW = 128;         // floats per row
constexpr int WAVE_ROW_PAIRS = 64;    // float2 per row
constexpr int WAVE_ROW_QUADS = 32;    // float4 per row
CMPS_LAYOUT_FN size_t wave_row_index(size_t b, int N, int k, int vr = 1, int av = 0) { return (b * N + k) * vr + av; }
CMPS_LAYOUT_FN size_t wave_row(size_t b, int N, int k, int vr = 1, int av = 0) { return wave_row_index(b, N, k, vr, av) * WAVE_ROW; }
// the first row of a clip with vr columns per step, in float2
CMPS_LAYOUT_FN size_t wave_clip_pair(int b, int N, int vr) { return (size_t)b * N * vr * WAVE_ROW_PAIRS; }
// position of (component i < 32, re | im, y | H y) in a row: STASH_WAVE16 and RHO_STASH_WAVE keep lane order (re on lane i, im on lane
// i + 32), STASH_WAVE32 / WAVE32N and RHO_STASH_MFMA the pairs of the real components n = 2 i + {re, im}
CMPS_LAYOUT_FN int wave16_pos(int i, int im, int hy) { return 2 * (i + 32 * im) + hy; }
CMPS_LAYOUT_FN int wave32_pos(int i, int im, int hy) { return 4 * i + 2 * im + hy; }

// ---- wide and pair vectors (32 < D <= 128): 4 PD floats, one per (row < PD, component re | im, clip of the pair) ----
constexpr int STASH_VECS = 2;     // vectors per pair and step in the stash: y | H y
constexpr int YBAR_VECS = 1;      // ... and in the ybar rows
CMPS_LAYOUT_FN int vec_floats(int PD) { return 4 * PD; }
CMPS_LAYOUT_FN int stash_step_floats(int PD) { return STASH_VECS * vec_floats(PD); }
CMPS_LAYOUT_FN int ybar_step_floats(int PD) { return YBAR_VECS * vec_floats(PD); }
CMPS_LAYOUT_FN int stash_step_bytes(int PD) { return stash_step_floats(PD) * 4; }
CMPS_LAYOUT_FN int ybar_step_bytes(int PD) { return ybar_step_floats(PD) * 4; }
// the vector (pair, step, y / H y) in the stash, and (pair, step) in the ybar rows: both families
CMPS_LAYOUT_FN size_t wide_stash_vec(int PD, size_t pair, int N, int step, int yh) { return ((pair * N + step) * STASH_VECS + yh) * (size_t)vec_floats(PD); }
CMPS_LAYOUT_FN size_t wide_ybar_vec(int PD, size_t pair, int N, int step) { return (pair * N + step) * (size_t)vec_floats(PD); }
// wide family: (row, component, clip) inside a vector -- [wave][lane], wave = row / 16, lane = 8 q + row % 8, q = (row half, component, clip)
CMPS_LAYOUT_FN int wide_pos(int row, int comp, int clip) { return 64 * (row >> 4) + 8 * (4 * ((row >> 3) & 1) + 2 * comp + clip) + (row & 7); }
// the same position for thread tid of k_grad_gemm's build role, whose (row, clip) = (8 (tid / 16) + tid % 8, (tid / 8) % 2): component c
CMPS_LAYOUT_FN int wide_pos_thread(int tid, int c) { return (((tid >> 4) << 5) | (tid & 15)) + 16 * c; }
// pair family: [clip][re | im][PD] inside a vector; (pair, step, y / H y, clip, component, row) in the stash and (pair, step, ...) in the ybar
// rows are the vector plus pair_pos, in the shape of the pair kernels (PD a template argument: as a run-time one it moves their instructions)
CMPS_LAYOUT_FN int pair_pos(int PD, int row, int comp, int clip) { return (clip * 2 + comp) * PD + row; }
// ... and of thread tid of k_grad_gemm's build role (see wide_pos_thread)
CMPS_LAYOUT_FN int pair_pos_thread(int PD, int tid, int c) { return ((((tid >> 3) & 1) * 2 + c) * PD) + 8 * (tid >> 4) + (tid & 7); }
template <int PD>
CMPS_LAYOUT_FN size_t pair_stash_index(size_t pair, int N, int step, int yh, int clip, int comp, int row) {
    return (((((pair * N + step) * 2 + yh) * 2 + clip) * 2 + comp) * PD) + row;
}
template <int PD>
CMPS_LAYOUT_FN size_t pair_ybar_index(size_t pair, int N, int step, int clip, int comp, int row) {
    return ((pair * N + step) * 4 + (clip * 2 + comp)) * PD + row;
}
// RhoCMPS on the wide kernels: column a of clip b is clip (a & 1) of virtual pair (b vrank + a) / 2
CMPS_LAYOUT_FN size_t rho_wide_pair(size_t b, int vrank, int a) { return (b * vrank + a) >> 1; }
CMPS_LAYOUT_FN int rho_wide_clip(int a) { return a & 1; }

// ---- block rows: [B][N][DP] float2 (STASH_BLOCK), with the columns [B][N][rank][DP] float2 (RHO_STASH_BLOCK).  RHO_STASH_WAVE and
// RHO_STASH_MFMA are wave rows, one per column, in wave16_pos and wave32_pos order ----
CMPS_LAYOUT_FN size_t block_row_pair(size_t b, int N, int k, int DP, int r = 1, int a = 0) { return wave_row_index(b, N, k, r, a) * DP; }
// floats of a RhoCMPS row: per column (BLOCK, WAVE, MFMA) or per pair of columns (WIDE)
CMPS_LAYOUT_FN int rho_row_floats(int layout, int DP) { return layout == RHO_STASH_BLOCK ? 2 * DP : layout == RHO_STASH_WIDE ? vec_floats(DP) : WAVE_ROW; }

// ---- section bytes (make_layout, make_rho_layout) ----
CMPS_LAYOUT_FN size_t pairs_of(size_t B) { return (B + 1) / 2; }
CMPS_LAYOUT_FN size_t wide_stash_bytes(size_t pairs, size_t N, size_t DP) { return pairs * N * STASH_VECS * vec_floats((int)DP) * sizeof(float); }
CMPS_LAYOUT_FN size_t wide_ybar_bytes(size_t pairs, size_t N, size_t DP) { return pairs * N * YBAR_VECS * vec_floats((int)DP) * sizeof(float); }
CMPS_LAYOUT_FN size_t wave_stash_bytes(size_t B, size_t N, size_t r = 1) { return B * N * r * WAVE_ROW * sizeof(float); }
CMPS_LAYOUT_FN size_t block_stash_bytes(size_t B, size_t N, size_t DP, size_t r = 1) { return B * N * r * DP * sizeof(float2); }
// pure states: D > 32 whole pairs of wide / pair vectors (the block kernels use half of it); D <= 32 the wave rows (the block rows fit inside)
CMPS_LAYOUT_FN size_t psi_stash_bytes(int D, size_t DP, size_t B, size_t N) {
    if (D > 32) return wide_stash_bytes(pairs_of(B), N, DP);
    return block_stash_bytes(B, N, DP) < wave_stash_bytes(B, N) ? wave_stash_bytes(B, N) : block_stash_bytes(B, N, DP);
}
// RhoCMPS: D <= 32 one wave row per column and step, else the block rows
CMPS_LAYOUT_FN size_t rho_stash_bytes(int D, size_t DP, size_t B, size_t N, size_t r) {
    return D <= 32 ? wave_stash_bytes(B, N, r) : block_stash_bytes(B, N, DP, r);
}

}  // namespace cmps
