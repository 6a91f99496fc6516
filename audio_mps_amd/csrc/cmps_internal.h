// Internal declarations shared by the HIP translation units of libcmps.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "cmps_stash_layout.h"

namespace cmps {

// ---------------------------------------------------------------------------------------------
// Per-kernel durations (cmps_set_option(CMPS_OPT_KERNEL_EVENTS, 1); cmps_kernel_times): while the option is on, every kernel the
// scan entry points launch is bracketed by two HIP events on the caller's stream.  Off (the default) nothing is recorded and a
// KScope is two pointer tests.  The C ABI functions set the thread-local pointer for the duration of a call.
// ---------------------------------------------------------------------------------------------
struct KTimer {
    struct Rec { const char* name; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
extern thread_local KTimer* g_ktimer;
struct KScope {
    KTimer* t; hipStream_t s; const char* name; hipEvent_t a;
    KScope(const char* name_, hipStream_t s_) : t(g_ktimer), s(s_), name(name_), a(nullptr) {
        if (t) { a = t->get(); (void)hipEventRecord(a, s); }
    }
    ~KScope() {
        if (t) { hipEvent_t b = t->get(); (void)hipEventRecord(b, s); t->recs.push_back({name, a, b}); }
    }
};


// ---------------------------------------------------------------------------------------------
// Workspace layout (all offsets in bytes from the workspace base, every section 256-B aligned).  The positions inside the stash, the
// scalar rows and the ybar rows, and the bytes of those sections, are stated in cmps_stash_layout.h.
//
//   mats     : R [D][D] float2 | RT [D][D] float2 (RT[j][i] = R[i][j]) | Q [D][D] float2
//              (Q = -(dt sigma^2 / 2) R^dagger R, Hermitian) | psi0 [D] float2 | freqs [D] float | qflag (|Q|_F <= 2^-19)
//   ttab     : t_k, k = 0..N          float32, sequential sum (model.py:16,266,281)
//   dtk      : t_k - t_{k+1}          float32 (exact), k = 0..N-1
//   rho      : [N+1][DP] float2       rho_k[d] = exp(i (fl(f_d t_k) - fl(f_d t_{k+1}))), drift-corrected (cmps_prep.hip)
//   rfix     : [2][NC][DP] double2    scratch of the drift correction
//   stash    : [B][N][DP] float2      un-normalised rotating-frame state y_k (TRAIN only; block variant)
//   hst      : [B][N][64][2] float    wave variants' stash (same region as `stash`), 512 B per step: pairs (y_k, (R + R^dagger) y_k)
//                                     per real component n = 2 i + {re, im} (32-row layout) or per lane (16-row layout)
//   scal     : [B][NC][2][64] float   per 64-step chunk: |y_k|^2 and e_k, one step per lane (wave variant)
//   gops     : [pairs][N][4 DP] float   D > 32, TRAIN: ybar_k of the reverse scan for the gradient GEMM, which builds its
//                                     operands (te y | s ybar | ybar | y | u) itself: pair kernels [clip][re | im][DP], wide kernels
//                                     [wave][lane] (round 2 kept the five operands here in bf16, 2.5 x the bytes)
//   slabs    : [B][slab] float        per-clip gradient partials (TRAIN only)
//   sums     : [slab] float           reduced partials, followed by [32][slab] double first-pass partial sums
//   status   : [2] unsigned           flag words of the last cmps_psi_loss_bwd and their OR since the last cmps_psi_grad_status
//                                     (bit 0: a gradient sum is Inf / NaN, bit 1: the loss sum is) -- written by k_reduce_slabs / k_finalize
// DP = D rounded up to a multiple of 32 (components >= D are zero padding and stay exactly zero).
// ---------------------------------------------------------------------------------------------
struct Layout {
    int D, DP, B, T, N, flags;
    size_t off_R, off_RT, off_Q, off_QT, off_psi0, off_freqs, off_qflag, off_ttab, off_dtk, off_rho, off_rfix,
        off_stash, off_hst, off_scal, off_slabs, off_sums, off_gops, off_opmax, off_status, total;
    size_t slab_floats;  // psi_slab_floats(DP)
};

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

constexpr int padded_D(int D) { return (D + 31) / 32 * 32; }   // zero padding to the next multiple of 32 (32, 64, 96, 128)

constexpr int WS_TRAIN = 1;   // CMPS_WS_TRAIN (include/cmps.h): the workspace has the stash, the slabs and the reduction buffers
// floats of a pure-state gradient slab: Rbar and Qbar as re | im planes [DP][DP], then f | psi0bar_re | psi0bar_im [DP] each, A, one spare
constexpr size_t psi_slab_floats(size_t DP) { return 4 * DP * DP + 3 * DP + 2; }
// bytes of a `sums` section for slabs of `slab` floats: the reduced slab (padded to the next 64 floats) + [32][slab] double first-pass partials
constexpr size_t sums_bytes(size_t slab) { return (slab + 64) * sizeof(float) + 32 * slab * sizeof(double); }

constexpr Layout make_layout(int D, int B, int T, int flags) {
    Layout L{};
    L.D = D; L.B = B; L.T = T; L.N = T - 1; L.flags = flags;
    // one layout serves both variants: tables are sized for the larger stride
    L.DP = padded_D(D);
    const size_t DP = (size_t)L.DP, N = (size_t)L.N;
    size_t o = 0;
    L.off_R = o;     o = align256(o + DP * DP * sizeof(float2));
    L.off_RT = o;    o = align256(o + DP * DP * sizeof(float2));
    L.off_Q = o;     o = align256(o + DP * DP * sizeof(float2));
    L.off_QT = o;    o = align256(o + DP * DP * sizeof(float2));
    L.off_psi0 = o;  o = align256(o + DP * sizeof(float2));
    L.off_freqs = o; o = align256(o + DP * sizeof(float));
    L.off_qflag = o; o = align256(o + sizeof(unsigned));
    L.off_ttab = o;  o = align256(o + (N + 1) * sizeof(float));
    L.off_dtk = o;   o = align256(o + (N + 64) * sizeof(float));
    L.off_rho = o;   o = align256(o + (N + 1) * DP * sizeof(float2));
    L.off_rfix = o;  o = align256(o + ((N + 63) / 64) * DP * 2 * sizeof(double2));
    L.slab_floats = psi_slab_floats(DP);
    L.off_stash = o;
    L.off_hst = o;
    L.off_scal = o;
    L.off_slabs = o;
    L.off_sums = o;
    L.off_gops = o;
    L.off_opmax = o;
    L.off_status = o;
    if (flags & WS_TRAIN) {
        // the two variants never run on the same stash: their layouts share one region
        L.off_hst = L.off_stash;
        o = align256(o + psi_stash_bytes(D, DP, B, N));
        L.off_scal = o;  o = align256(o + scal_bytes(B, N));
        L.off_slabs = o; o = align256(o + (size_t)B * L.slab_floats * sizeof(float));
        L.off_sums = o;  o = align256(o + sums_bytes(L.slab_floats));
        L.off_gops = o;
        // ybar rows: exactly [pairs][N][4 DP] floats (k_grad_gemm clamps every row it requests to the pair's range and its buffer
        // descriptors end at the last row; round 3's 32 rows of slack behind the section had no reader left -- ADVICE r3)
        if (D > 32) o = align256(o + wide_ybar_bytes(pairs_of(B), N, DP));
        // max |ybar| per pair (wide reverse scan -> the gradient GEMM's fp16 operand scale, CMPS_RANK1_F16X2)
        L.off_opmax = o;
        if (D > 32) o = align256(o + pairs_of(B) * sizeof(float));
        L.off_status = o; o = align256(o + 2 * sizeof(unsigned));
    }
    L.total = o;
    return L;
}

// Device-side view handed to the kernels by value.
struct Dev {
    int D, DP, B, T, N;
    const float2* R;     // [DP][DP] row-major
    const float2* RT;    // [DP][DP], RT[j][i] = R[i][j]
    const float2* Q;     // [DP][DP] row-major, Hermitian (legacy mode: general complex)
    const float2* QT;    // [DP][DP] transpose of Q (legacy mode only)
    const float2* psi0;  // [DP]
    const float* freqs;  // [DP]
    const unsigned* qflag;  // [1]: 1 when |Q|_F <= 2^-19 (k_qflag, once per cmps_set_params): which instance of the chain16 kernels runs
    const float* ttab;   // [N+1]
    const float* dtk;    // [N]
    const float2* rho;   // [N][DP]
    float2* stash;       // [B][N][DP]
    float* hst;          // [B][N][64][2] (wave variant)
    int stash_layout;    // a StashLayout: STASH_BLOCK reads `stash`, the STASH_WAVE* layouts `hst`, STASH_PAIR / STASH_WIDE their rows in `stash`
    float* scal;         // [B][NC][2][64]
    void* gops;          // ybar rows for the gradient GEMM (see the layout comment), D > 32 only
    float* opmax;        // [pairs] max |ybar| over the pair's steps and rows (written by k_bwd_wide), D > 32 only
    float* slabs;        // [B][slab]
    float* sums;         // [slab]
    size_t slab_floats;
    float A;
    const float* Adev;   // non-null: A lives in device memory (cmps_set_params_dev: device-resident optimiser step) and `A` is unset
    float dt;            // (float)delta_t (model.py:16; also the python-float factor of model.py:286)
    float c_half;        // (float)(-delta_t * sigma^2) / 2   (model.py:312)
    // RhoCMPS on the wide kernels (32 < D <= 128; cmps_wide.hip, round 5): the columns of every clip's rho are handed to the pure-state
    // kernels as VIRTUAL clips (virtual clip v = clip * phi_rank + column); then the initial vector of virtual clip v is phi0[v % phi_rank]
    // instead of psi0, dA's per-clip sum is taken once per real clip, and the reverse scan leaves every column's cotangent in gphi
    const float2* phi0;  // [phi_rank][DP] (zero rows pad an odd rank), or null: the pure-state model
    int phi_rank;        // columns per clip, even
    float* gphi;         // [virtual clips][re | im][DP]
    unsigned* status;    // [2]: flag word of the last reverse pass | OR since the last cmps_psi_grad_status (TRAIN workspaces; else null)
    int f16_shift;       // CMPS_OPT_F16_SCALE_SHIFT (diagnostic, 0): added to the exponent of the wave reverse scan's data-dependent fp16 scales
    int abar_fix;        // 1: the slabs' Abar holds -(sum_k Re(u^dagger (Q + s R^dagger) ybar)) / A (k_bwd_wave's merged mat-vec);
                         //    k_finalize adds Re sum_ij Q_ij Qbar_ji / A from the reduced Qbar
    // A bank of M same-shape models in one launch (cmps_bank_*): member m's workspace is the plain layout `bank_stride` bytes behind
    // member m - 1's, and the caller's buffers are rows of one array per member.  A plain launch has every stride 0 and one member.
    size_t bank_stride;  // bytes between two members' workspaces (M > 1: make_layout(...).total)
    size_t bank_audio;   // floats between two members' audio (B T; 0: one batch shared by every member)
    size_t bank_loss;    // floats between two members' per-clip losses (B)
    size_t bank_grad;    // floats between two members' gradient sums (2 D^2 + 3 D + 2)
    size_t bank_adev;    // floats between two members' effective parameters (2 D^2 + 3 D + 1): what Adev moves by
};

// p moved forward by `bytes` (a member's section of a bank's workspace)
template <typename T>
__host__ __device__ __forceinline__ T* bank_shift(T* p, size_t bytes) {
    using C = std::conditional_t<std::is_const<T>::value, const char, char>;
    return reinterpret_cast<T*>(reinterpret_cast<C*>(p) + bytes);
}
// The Dev of member `member` of a bank: every workspace pointer moved by member * bank_stride, Adev by member * bank_adev floats.  The
// kernels take it once at entry with member = blockIdx.y (wave-uniform: scalar arithmetic in front of the role split); nothing behind
// the entry knows about banks.  Stride 0 / member 0 (every plain launch) is the Dev as it was handed in.  Sections a workspace does
// not have (null: FWD_ONLY workspaces) and an unset Adev stay null.
__host__ __device__ __forceinline__ Dev bank_view(Dev P, unsigned member) {
    const size_t o = (size_t)member * P.bank_stride;
    P.R = bank_shift(P.R, o); P.RT = bank_shift(P.RT, o); P.Q = bank_shift(P.Q, o); P.QT = bank_shift(P.QT, o);
    P.psi0 = bank_shift(P.psi0, o); P.freqs = bank_shift(P.freqs, o); P.qflag = bank_shift(P.qflag, o);
    P.ttab = bank_shift(P.ttab, o); P.dtk = bank_shift(P.dtk, o); P.rho = bank_shift(P.rho, o);
    P.stash = bank_shift(P.stash, o); P.hst = bank_shift(P.hst, o); P.scal = bank_shift(P.scal, o);
    P.slabs = bank_shift(P.slabs, o); P.sums = bank_shift(P.sums, o);
    if (P.status) P.status = bank_shift(P.status, o);
    if (P.Adev) P.Adev += (size_t)member * P.bank_adev;
    return P;
}

// ---------------------------------------------------------------------------------------------
// RhoCMPS (cmps_rho.hip): its own caller-provided workspace next to the main one.
//   phi0  : [rank][DP] float2         columns of rho_0 = sum_a phi_a phi_a^dagger (trace 1)
//   stash : [B][N][rank][DP] float2   un-normalised rotating-frame columns y_a of every step (TRAIN / sampling states)
//   slabs : [B][slab] float           pure-state slab followed by the 2 rank DP cotangents of the initial columns
//   sums  : [slab] float + [32][slab] double first-pass partials
// ---------------------------------------------------------------------------------------------
struct RhoLayout {
    int rank;
    size_t off_phi0, off_stash, off_scal, off_slabs, off_sums, off_p1, off_cols, total, slab_floats;
    // the wide (virtual-clip) path of 32 < D <= 128, TRAIN workspaces: vrank = rank rounded up to even (0: not available)
    size_t off_wslabs, off_wsums;       // D <= 32, TRAIN: one pure-state slab per (clip, column) for the wave reverse scan on virtual clips
    int vrank;
    size_t off_vphi, off_vstash, off_vgops, off_vopmax, off_vscal, off_rscal, off_vslabs, off_vsums, off_vaudio, off_gphi, vslab_floats;
};

// RhoCMPS on the wide kernels: every pair of columns of a clip is one broadcast vector in LDS, two buffers (cmps_wide.hip::k_fwd_wide_rho)
constexpr size_t rho_wide_lds(int D, int rank) {
    const size_t PD = (size_t)padded_D(D), vr = (size_t)((rank + 1) / 2 * 2);
    return 2 * (vr / 2) * (8 * (PD / 8 + 1)) * 16 + 2 * (PD / 16) * sizeof(float) + 64;
}
constexpr bool rho_wide_ok(int D, int rank, int flags) { return D > 32 && D <= 128 && (flags & WS_TRAIN) && rho_wide_lds(D, rank) <= 120 * 1024; }

// rank * D above which the block kernels' column arrays (4 rank D complex numbers in the reverse scan) no longer fit into 160 KB of
// LDS and live in the workspace instead (RhoDev::cols): the reference's default rank = D (model.py:62-65) from D = 72 upwards
constexpr size_t RHO_LDS_COLS_MAX = 5000;
// LDS a workgroup of the block rho kernels may use for its column arrays, and the ONE predicate both the launchers (cmps_rho.hip:
// cols_if_needed) and the argument checks (cmps_capi.hip) use for "this kernel's `arrays` column arrays go to the workspace"
// (forward 2, reverse scan 4, sampler 3 arrays of rank * D complex numbers): the workspace section is provided from
// RHO_LDS_COLS_MAX upwards (sized for the reverse scan), but a kernel spills only when ITS request exceeds the LDS
constexpr size_t RHO_LDS_MAX = 160 * 1024;
inline bool rho_cols_spill(int arrays, int rank, int D) { return (size_t)arrays * rank * D * sizeof(float2) + 128 > RHO_LDS_MAX; }

constexpr RhoLayout make_rho_layout(int D, int rank, int B, int T, int flags) {
    RhoLayout L{};
    const size_t DP = (size_t)padded_D(D), N = (size_t)(T - 1), r = (size_t)rank;
    L.rank = rank;
    L.slab_floats = psi_slab_floats(DP) + 2 * r * DP;
    size_t o = 0;
    L.off_phi0 = o; o = align256(o + r * DP * sizeof(float2));
    L.off_stash = L.off_scal = L.off_slabs = L.off_sums = o;
    if (flags & WS_TRAIN) {
        L.off_stash = o; o = align256(o + rho_stash_bytes(D, DP, B, N, r));
        L.off_scal = o;  o = align256(o + scal_bytes(B, N));
        L.off_slabs = o; o = align256(o + (size_t)B * L.slab_floats * sizeof(float));
        L.off_sums = o;  o = align256(o + sums_bytes(L.slab_floats));
        // D <= 32: sum_k 2 ebar_k Y^T Y (real 64 x 64 form, four C/D tiles per clip), accumulated by k_fwd_rho_mfma for the reverse scan
        L.off_p1 = o;    if (D <= 32) o = align256(o + (size_t)B * 4096 * sizeof(float));
        L.off_wslabs = L.off_wsums = o;
        if (D <= 32) {
            const size_t psl = psi_slab_floats(DP);
            L.off_wslabs = o; o = align256(o + (size_t)B * r * psl * sizeof(float));
            L.off_wsums = o;  o = align256(o + sums_bytes(psl));
        }
    }
    // column arrays of the block kernels when they do not fit into LDS: [B][4][rank][D] float2 (forward 2, sampler 3, reverse 4)
    L.off_cols = o;
    if (r * (size_t)D > RHO_LDS_COLS_MAX) o = align256(o + (size_t)B * 4 * r * D * sizeof(float2));
    L.vrank = 0;
    if (rho_wide_ok(D, rank, flags)) {
        const size_t vr = (size_t)((rank + 1) / 2 * 2), vB = (size_t)B * vr, vp = vB / 2;
        L.vrank = (int)vr;
        L.vslab_floats = psi_slab_floats(DP);
        L.off_vphi = o;   o = align256(o + vr * DP * sizeof(float2));
        L.off_vstash = o; o = align256(o + wide_stash_bytes(vp, N, DP));             // [virtual pair][step][y | H y][4 DP]
        L.off_vgops = o;  o = align256(o + wide_ybar_bytes(vp, N, DP));              // ybar rows
        L.off_vopmax = o; o = align256(o + vp * sizeof(float));
        L.off_vscal = o;  o = align256(o + scal_bytes(vB, N));                       // (|y|^2 of the clip, e of the clip) per virtual clip
        L.off_rscal = o;  o = align256(o + scal_bytes(B, N));                        // the same per real clip
        L.off_vslabs = o; o = align256(o + vp * L.vslab_floats * sizeof(float));
        L.off_vsums = o;  o = align256(o + sums_bytes(L.vslab_floats));
        L.off_vaudio = o; o = align256(o + vB * (size_t)T * sizeof(float));
        L.off_gphi = o;   o = align256(o + vB * 2 * DP * sizeof(float));
    }
    L.total = o;
    return L;
}

struct RhoDev {
    int rank;
    int stash_layout;    // a RhoStashLayout
    float* wslabs; float* wsums;   // D <= 32: the wave reverse scan's slabs, one per (clip, column), and their reduction buffer
    int vrank;           // rank rounded up to even when the wide path's sections exist (else 0)
    float2* vphi;        // [vrank][DP]
    float* vstash; float* vgops; float* vopmax; float* vscal; float* rscal; float* vslabs; float* vsums; float* vaudio; float* gphi;
    size_t vslab_floats;
    float* scal;         // [B][NC][2][64]: tr rho'_k and e_k, one step per lane (wave kernels)
    float* p1;           // [B][4][16][64]: the forward's part of Rbar (cmps_rho_mfma.hip), raw C/D tiles
    const float2* phi0;  // [rank][DP]
    float2* cols;        // [cols_blocks][4][rank][D] column arrays of the block kernels when rank * D exceeds the LDS (else null)
    int cols_blocks;
    float2* stash;       // [B][N][rank][DP]
    float* slabs;        // [B][slab]
    float* sums;         // [slab]
    size_t slab_floats;
};

// bank_view for the one kernel instance that reads Dev::phi0, k_bwd_wave2w<false> on RhoCMPS's virtual clips: the columns lie in the
// member's region too and move with it (null, a pure-state model: stays null).  Kept out of bank_view itself: with the move inside it
// the compiler laid out k_bwd_wave2w<true>, the flagship's reverse scan, which never has columns, differently, and bench.py's bwd_ms
// rose by 0.6 % in six interleaved A/B runs; this way that instance's code is the parent's, byte for byte.
__host__ __device__ __forceinline__ Dev bank_view_phi(Dev P, unsigned member) {
    const float2* phi0 = P.phi0 ? bank_shift(P.phi0, (size_t)member * P.bank_stride) : nullptr;
    P = bank_view(P, member);
    P.phi0 = phi0;
    return P;
}

// A bank of RhoCMPS models (cmps_rho_bank_*) has ONE workspace: member m's region is the plain main layout (tables only) followed by
// the plain rho layout, Dev::bank_stride bytes behind member m - 1's, so that the virtual-clip reverse sweep's Dev -- which takes
// R, Q, rho, the time tables and Adev from the main part and the stash, the scalars, the slabs and phi0 from the rho part -- moves
// by the one stride bank_view knows.  The RhoDev of a member: every section moved by `bytes` = member * Dev::bank_stride; sections
// a workspace does not have stay null.  (`cols` is null in a bank's scope, rank * D <= 1024; the wide path's v* sections do not exist
// at D <= 32.)  0 bytes (every plain launch) is the RhoDev as it was handed in.
__host__ __device__ __forceinline__ RhoDev rho_bank_view(RhoDev W, size_t bytes) {
    W.phi0 = bank_shift(W.phi0, bytes);
    if (W.stash) W.stash = bank_shift(W.stash, bytes);
    if (W.scal) W.scal = bank_shift(W.scal, bytes);
    if (W.p1) W.p1 = bank_shift(W.p1, bytes);
    if (W.slabs) W.slabs = bank_shift(W.slabs, bytes);
    if (W.sums) W.sums = bank_shift(W.sums, bytes);
    if (W.wslabs) W.wslabs = bank_shift(W.wslabs, bytes);
    if (W.wsums) W.wsums = bank_shift(W.wsums, bytes);
    return W;
}

// ---- host-side dispatch of a run-time value to a template argument, written once for every launcher ----
// f(std::integral_constant<int, PD>{}) for the padded bond dimension of the MFMA / wide kernels (64, 96 or 128)
template <typename F>
inline hipError_t dispatch_pd(int DP, F&& f) {
    if (DP == 128) return f(std::integral_constant<int, 128>{});
    if (DP == 96) return f(std::integral_constant<int, 96>{});
    if (DP == 64) return f(std::integral_constant<int, 64>{});
    return hipErrorInvalidValue;
}
// f(std::true_type{}) or f(std::false_type{})
template <typename F>
inline hipError_t dispatch_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}
// f(std::integral_constant<int, NT>{}): threads per workgroup of the block-per-clip forward scans and samplers (one per component)
template <typename F>
inline hipError_t dispatch_block_nt(int D, F&& f) {
    if (D <= 64) return f(std::integral_constant<int, 64>{});
    return f(std::integral_constant<int, 128>{});
}
// the same for the block-per-clip reverse scans, whose threads each own BLOCK_EPT elements of Rbar and Qbar (NT * BLOCK_EPT >= D * D)
constexpr int BLOCK_EPT = 16;
template <typename F>
inline hipError_t dispatch_block_bwd(int D, F&& f) {
    if (D <= 32) return f(std::integral_constant<int, 64>{});
    if (D <= 64) return f(std::integral_constant<int, 256>{});
    return f(std::integral_constant<int, 1024>{});
}
// f(std::integral_constant<int, MODE>{}) for the rank-1 sums of k_bwd_wave (CMPS_RANK1_*: 0, 1, 3; every other value runs 2)
template <typename F>
inline hipError_t dispatch_rank1(int mode, F&& f) {
    if (mode == 0) return f(std::integral_constant<int, 0>{});
    if (mode == 1) return f(std::integral_constant<int, 1>{});
    if (mode == 3) return f(std::integral_constant<int, 3>{});
    return f(std::integral_constant<int, 2>{});
}

// a kernel's dynamic LDS above the 64 KB every kernel may ask for without saying so
template <typename K>
inline hipError_t lds_attr(K kernel, size_t shm) {
    if (shm <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
}
inline int round_up64(int d) { return (d + 63) / 64 * 64; }   // whole waves for d threads

// ---- launchers (each returns the hipError_t of its launches) ----
// (M > 1, cmps_rho_bank_set_state_dev: member m's columns lie 2 rank D floats behind member m - 1's, its phi0 P.bank_stride bytes)
hipError_t launch_pack_phi(const Dev& P, const RhoDev& W, const float* re, const float* im, hipStream_t s, int M = 1);
hipError_t launch_fwd_rho(const Dev& P, const RhoDev& W, const float* audio, float* loss, bool save, hipStream_t s);
hipError_t launch_bwd_rho(const Dev& P, const RhoDev& W, const float* audio, hipStream_t s);
hipError_t launch_finalize_rho(const Dev& P, const RhoDev& W, float* grad_out, hipStream_t s);
hipError_t launch_states_rho(const Dev& P, const RhoDev& W, int B, int steps, float* rho_out, float* purity_out,
                             hipStream_t s);
hipError_t launch_update_ancilla_rho(const Dev& P, const float* rho_in, const float* signal, float t, int B,
                                     float* rho_out, hipStream_t s);
// ---- the samplers: every launcher takes one SampleDev; PrimeDev, StreamDev and ScoreDev inside it are what the kernels take by value ----
// PR (cmps_*_sample_primed): PF = prime_T - 1 teacher-forced steps on prime[path * stride + k] (stride 0: one shared clip) in front of the
// `length` sampled ones; pred [n][PF] may be null.  ST (cmps_*_stream): one segment of a resumable scan -- the primed arguments with PF =
// forced (either count may be 0, not both), on table rows k0 .. k0 + PF + length - 1; the state a kernel carries from one step into the
// next is read from `in` (null: the start of a scan, psi_0 or the columns of cmps_rho_set_state) and written to `out` (null: not kept),
// `rec` floats per path.  in == out is allowed: a path reads its record before it writes it.  SC (cmps_{psi,rho}_stream_score): a stream
// segment of PF forced steps that also gives the loss increment of every step.
// Whoever fills the record zeroes what its mode does not use (unprimed: PR; scored: noise, length, out); a null ST / SC reaches the kernel as zeros.
struct PrimeDev {
    const float* prime;
    int stride, PF;
    float* pred;
};
struct StreamDev {
    const float* in;
    float* out;
    int k0;
    int rec;
};
struct ScoreDev {
    float* nll;       // every step's loss increment [path][step], or null
    float* loss;      // the running loss per path: read when the segment resumes a scan (StreamDev::in set), written behind the last step
};
// MB (cmps_bank_stream*): the launch runs M members of a bank, member m = blockIdx.y on bank_view(P, m), n paths each.  What a path writes
// or carries (out, pred, nll, the running loss, the state records) is one array over the global paths g = m n + b; the audio and the noise
// of member m lie `audio` / `noise` floats behind member m - 1's (0: every member reads the same rows).  M = 0: a plain launch.
struct MemberDev {
    int M = 0;
    size_t audio = 0, noise = 0;
};
struct SampleDev {
    const float* noise;     // [n][length]
    int n, length;
    float* out;             // [n][length]
    PrimeDev PR;
    const StreamDev* ST;    // null: not a stream segment
    const ScoreDev* SC;     // null: not scored
    MemberDev MB{};         // M == 0: not a bank's launch
};
// What the BANK instances of the sampler kernels take at entry: the member's Dev and the global number of path b of n (the plain instances:
// the Dev and the path as they were handed in, no code)
template <bool BANK>
__device__ __forceinline__ Dev member_view(const Dev& P) {
    if constexpr (BANK) return bank_view(P, blockIdx.y);
    else return P;
}
template <bool BANK>
__device__ __forceinline__ size_t member_path(int n, int b) {
    if constexpr (BANK) return (size_t)blockIdx.y * (size_t)n + (size_t)b;
    else return (size_t)b;
}
inline StreamDev stream_of(const SampleDev& S) { return S.ST ? *S.ST : StreamDev{}; }
inline ScoreDev score_of(const SampleDev& S) { return S.SC ? *S.SC : ScoreDev{}; }
// The mode of a launch, stated once (ST first: a stream segment with forced == 0 has PR.prime == nullptr and is still SAMPLE_STREAM).  A
// kernel's PRIMED, STREAM, SCORE (mode >= SAMPLE_PRIMED, >= SAMPLE_STREAM, == SAMPLE_SCORE) and its KScope name follow from it.
// dispatch_sample_mode: f(std::integral_constant<int, MODE>{})
enum SampleMode { SAMPLE_PLAIN, SAMPLE_PRIMED, SAMPLE_STREAM, SAMPLE_SCORE };
inline SampleMode sample_mode(const SampleDev& S) { return S.ST ? (S.SC ? SAMPLE_SCORE : SAMPLE_STREAM) : S.PR.prime ? SAMPLE_PRIMED : SAMPLE_PLAIN; }
template <typename F>
inline hipError_t dispatch_sample_mode(SampleMode mode, F&& f) {
    if (mode == SAMPLE_SCORE) return f(std::integral_constant<int, SAMPLE_SCORE>{});
    if (mode == SAMPLE_STREAM) return f(std::integral_constant<int, SAMPLE_STREAM>{});
    if (mode == SAMPLE_PRIMED) return f(std::integral_constant<int, SAMPLE_PRIMED>{});
    return f(std::integral_constant<int, SAMPLE_PLAIN>{});
}
// floats of one path's record of the RhoCMPS samplers, a multiple of 4: k_sample_rho_mfma the rows a < rank of U [rank][64], running sum |
// k_sample_rho the columns S [rank][D] float2, running sum
inline int stream_rec_rho_mfma(int rank) { return 64 * rank + 4; }
inline int stream_rec_rho(int rank, int D) { return (2 * rank * D + 1 + 3) / 4 * 4; }
hipError_t launch_sample_rho(const Dev& P, const RhoDev& W, const SampleDev& S, bool save, hipStream_t s);
hipError_t launch_fwd_legacy_wave(const Dev& P, const float* audio, float* loss, bool save, hipStream_t s);
hipError_t launch_bwd_legacy_wave(const Dev& P, const float* audio, int rank1_mode, hipStream_t s);
hipError_t launch_legacy_tables(const Dev& P, float2* psi0, float* dtk, float2* rho, hipStream_t s);
hipError_t launch_fwd_rho_wave(const Dev& P, const RhoDev& W, const float* audio, float* loss, bool save, hipStream_t s, int M = 1);
hipError_t launch_fwd_rho_mfma(const Dev& P, const RhoDev& W, const float* audio, float* loss, bool save, bool f16, bool grad1, hipStream_t s,
                               int M = 1);
hipError_t launch_bwd_rho_mfma(const Dev& P, const RhoDev& W, const float* audio, hipStream_t s);
hipError_t launch_sample_rho_mfma(const Dev& P, const RhoDev& W, const SampleDev& S, bool save, bool f16, hipStream_t s);
hipError_t launch_bwd_rho_wave(const Dev& P, const RhoDev& W, const float* audio, hipStream_t s);
hipError_t launch_prep(const Dev& P, const float* R_re, const float* R_im, const float* freqs,
                       const float* psi0_re, const float* psi0_im, float dt, bool rebuild_ttab,
                       float* ttab, float* dtk, float2* R, float2* RT, float2* Q, float2* psi0,
                       float* freqs_out, float2* rho, double2* rfix, hipStream_t s, int M = 1, size_t par_stride = 0);

// (M: the members of a bank, the kernels' second grid dimension -- Dev::bank_*; the plain entry points launch one)
hipError_t launch_fwd_block(const Dev& P, const float* audio, float* loss, bool save, hipStream_t s, int M = 1);
hipError_t launch_bwd_block(const Dev& P, const float* audio, hipStream_t s, int M = 1);
hipError_t launch_bwd_wave(const Dev& P, const float* audio, int rank1_mode, hipStream_t s);
hipError_t launch_bwd_wave2w(const Dev& P, const float* audio, hipStream_t s, int M = 1);    // cmps_wave_bwd2.hip: two waves per clip (F16X2 sums)
hipError_t launch_fwd_wave2(const Dev& P, const float* audio, float* loss, bool save, bool hf16, bool norm_rows, hipStream_t s, int M = 1);
hipError_t launch_fwd_wave16(const Dev& P, const float* audio, float* loss, bool save, hipStream_t s, int M = 1);
hipError_t launch_bwd_wave16(const Dev& P, const float* audio, hipStream_t s, int M = 1);
hipError_t launch_fwd_pair(const Dev& P, const float* audio, float* loss, bool save, hipStream_t s);
hipError_t launch_bwd_pair(const Dev& P, const float* audio, hipStream_t s);
hipError_t launch_grad_pair(const Dev& P, const float* audio, hipStream_t s);
hipError_t launch_fwd_wide(const Dev& P, const float* audio, float* loss, bool save, bool hy_f16, bool chain_mfma, hipStream_t s);
hipError_t launch_fwd_wide_legacy(const Dev& P, const float* audio, float* loss, bool save, bool hy_f16, hipStream_t s);
hipError_t launch_bwd_wide_legacy(const Dev& P, const float* audio, hipStream_t s);
hipError_t launch_grad_wide_legacy(const Dev& P, const float* audio, bool f16, hipStream_t s);
hipError_t launch_bwd_rho_virtual_wave(const Dev& P, const RhoDev& W, const float* audio, const float* loss, float* grad_out, int rank1_mode, int bwd_waves,
                                       hipStream_t s, int M = 1);
hipError_t launch_fwd_rho_wide(const Dev& P, const RhoDev& W, const float* audio, float* loss, bool hy_f16, hipStream_t s);
hipError_t launch_bwd_rho_wide(const Dev& P, const RhoDev& W, const float* loss, float* grad_out, int pieces, hipStream_t s);
hipError_t launch_fwd_chain16(const Dev& P, const float* audio, hipStream_t s);
hipError_t launch_bwd_chain16(const Dev& P, const float* audio, hipStream_t s);    // cmps_pair.hip: the wide family's chain on the matrix cores
hipError_t launch_bwd_wide(const Dev& P, const float* audio, hipStream_t s);
hipError_t launch_grad_wide(const Dev& P, const float* audio, int pieces, hipStream_t s);
hipError_t launch_finalize_only(const Dev& P, const float* loss, float* grad_out, hipStream_t s, int M = 1);
hipError_t launch_reduce_finalize(const Dev& P, const float* loss, float* grad_out, hipStream_t s, int M = 1);
hipError_t launch_reduce_finalize_weighted(const Dev& P, const float* loss, float* grad_out, const float* weight, long long ldw,
                                           hipStream_t s, int M);
hipError_t launch_update_ancilla(const Dev& P, const float* psi_in, const float* signal, float t,
                                 int B, float* psi_out, hipStream_t s);
hipError_t launch_states(const Dev& P, int B, float* psi_out, hipStream_t s);
hipError_t launch_reduce_only(const Dev& P, hipStream_t s, int M = 1);
hipError_t launch_pack_legacy(const Dev& P, const float* Rr, const float* Qre, const float* Qim, float2* R,
                              float2* RT, float2* Q, float2* QT, hipStream_t s);
hipError_t launch_fwd_legacy(const Dev& P, const float* audio, float* loss, bool save, hipStream_t s);
hipError_t launch_bwd_legacy(const Dev& P, const float* audio, hipStream_t s);
hipError_t launch_finalize_legacy(const Dev& P, const float* loss, float* grad_out, hipStream_t s);
hipError_t launch_sample_wave(const Dev& P, const SampleDev& S, hipStream_t s);
hipError_t launch_sample_wide(const Dev& P, const SampleDev& S, hipStream_t s);
hipError_t launch_sample_block(const Dev& P, const SampleDev& S, hipStream_t s);
// cmps_noise.hip: noise[b * length + j] = stddev * z(seed, first_path + b, first_step + j), the counter-based normals of include/cmps.h
hipError_t launch_noise_philox(unsigned long long seed, unsigned long long first_step, unsigned first_path, int n, int length, float stddev,
                               float* noise, hipStream_t s);
// cmps_data.hip: audio[b * T + j] = data[index[b] * clip_len + offset[b] + j] (a row out of range: quiet NaNs), and clips first_clip ..
// first_clip + B - 1 of the synthetic damped-sine sequence of include/cmps.h
hipError_t launch_batch_gather(const float* data, long long n_clips, long long clip_len, const int* index, const int* offset, int B, int T,
                               float* audio, hipStream_t s);
hipError_t launch_damped_sine(unsigned long long seed, unsigned long long first_clip, int B, int T, double delta_t, float* audio, hipStream_t s);
// ... and the gather out of an int16 dataset: audio[b * T + j] = (float)data[...] * scale
hipError_t launch_batch_gather_i16(const short* data, long long n_clips, long long clip_len, const int* index, const int* offset, int B, int T,
                                   float scale, float* audio, hipStream_t s);
// cmps_eval.hip: loss[0 .. B), clip ids first_id + b, folded into the 64-byte record of include/cmps.h (reset: in place of what it held)
hipError_t launch_loss_stats(const float* loss, int B, long long first_id, int reset, void* stats, hipStream_t s);
// ... and loss[m * ld + b] of a bank forward judged as a classifier, into the record of cmps_bank_classify_stats (best[b]: the decision)
constexpr int CLASSIFY_MAX_M = 1024;
constexpr size_t CLASSIFY_HEAD_BYTES = 72;
hipError_t launch_classify_stats(const float* loss, int M, int B, long long ld, const int* label, long long first_id, int reset, void* stats,
                                 int* best, hipStream_t s);
// ... and turned into weight[m * ldw + b], the cotangents of the cross-entropy objective of cmps_bank_classify_weights, and its 40-byte record
hipError_t launch_classify_weights(const float* loss, int M, int B, long long ld, const int* label, double inv_temp, double gen_weight,
                                   double disc_weight, int reset, float* weight, long long ldw, void* record, hipStream_t s);
// ... and nll[(m * n + g) * steps + k] of a scored bank stream folded into running totals and the posterior over the members after every
// step (cmps_bank_posterior); a bank of more than POSTERIOR_WIDE_M members goes by in chunks of 32 steps instead of 64
constexpr int POSTERIOR_WIDE_M = 512;
constexpr int POSTERIOR_PREFETCH_M = 256;      // up to here a thread holds the next chunk's loads in registers while it works on this one
hipError_t launch_bank_posterior(const float* nll, int M, int n, int steps, const float* total_in, const double* log_prior, double inv_temp,
                                 float* total_out, float* post, int* best, float* conf, double threshold, long long first_step, int reset,
                                 void* decision, hipStream_t s);
// ... and the [M][N] losses of a held-out set fitted for the temperature and the prior (cmps_bank_calibrate): one iteration is a pass over
// the clips (many workgroups, their sums into rows of the scratch buffer) and an update (one workgroup: adds the rows, decides, moves theta)
size_t calib_scratch_bytes(int M, long long N);
hipError_t launch_calib_pass(const float* loss, int M, long long N, long long ld, const int* label, const double* theta, void* scratch,
                             int first, hipStream_t s);
hipError_t launch_calib_update(double* theta, void* record, void* scratch, int M, long long N, int fit, int max_iter, double tol,
                               double kappa_min, double kappa_max, int first, hipStream_t s);
// floats of one path's stream record (StreamDev::rec), a multiple of 4: wave u, |y|^2 partial per lane, running sum | wide ut [2 DP], |y|^2
// partial per wave [DP / 16], running sum | block u [2 D], running sum
constexpr int STREAM_REC_WAVE = 132;
inline int stream_rec_wide(int DP) { return (2 * DP + DP / 16 + 1 + 3) / 4 * 4; }
inline int stream_rec_block(int D) { return (2 * D + 1 + 3) / 4 * 4; }

size_t apply_step_scratch_bytes(int D);
hipError_t launch_apply_step(int D, bool apply, double inv_batch, double lr_t, double beta1, double beta2, double eps, double h_reg,
                             double r_reg, double c_r, double c_h, bool with_reg, float* vars, float* am, float* av,
                             const float* grad_sums, float* params_out, float* losses_out, double* scratch, hipStream_t s);
// cmps_bank_apply_step: M members' steps in one launch; hyper [M][5] = (learning_rate, h_reg, r_reg, c_r, c_h) per member, on the device
hipError_t launch_bank_apply_step(int D, int M, bool apply, double inv_batch, double bias_num, double bias_den, double beta1, double beta2,
                                  double eps, const double* hyper, bool with_reg, float* vars, float* am, float* av, const float* grad_sums,
                                  float* params_out, float* losses_out, double* scratch, hipStream_t s);
// cmps_rho_apply_step: the same step for RhoCMPS's variables (Wx, Wy [rank, D] in place of psi_x, psi_y); phi_out = the next columns
size_t rho_apply_step_scratch_bytes(int D, int rank);
hipError_t launch_rho_apply_step(int D, int rank, bool apply, double inv_batch, double lr_t, double beta1, double beta2, double eps,
                                 double h_reg, double r_reg, double c_r, double c_h, bool with_reg, float* vars, float* am, float* av,
                                 const float* grad_sums, float* params_out, float* phi_out, float* losses_out, double* scratch,
                                 hipStream_t s);
// cmps_rho_bank_apply_step: M members' RhoCMPS steps in one launch; hyper as for launch_bank_apply_step
hipError_t launch_rho_bank_apply_step(int D, int rank, int M, bool apply, double inv_batch, double bias_num, double bias_den, double beta1,
                                      double beta2, double eps, const double* hyper, bool with_reg, float* vars, float* am, float* av,
                                      const float* grad_sums, float* params_out, float* phi_out, float* losses_out, double* scratch,
                                      hipStream_t s);

// model.A (model.py:19) as the kernels see it: a launch argument, or -- device-resident training -- a word of device memory
__device__ __forceinline__ float dev_A(const Dev& P) { return P.Adev ? *P.Adev : P.A; }

// ---- small complex helpers (device) ----
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cmul_conj_a(float2 a, float2 b) {  // conj(a) * b
    return make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 c) {  // a*b + c
    return make_float2(fmaf(a.x, b.x, fmaf(-a.y, b.y, c.x)), fmaf(a.x, b.y, fmaf(a.y, b.x, c.y)));
}
__device__ __forceinline__ float2 cfma_conj_a(float2 a, float2 b, float2 c) {  // conj(a)*b + c
    return make_float2(fmaf(a.x, b.x, fmaf(a.y, b.y, c.x)), fmaf(a.x, b.y, fmaf(-a.y, b.x, c.y)));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 cscale(float s, float2 a) { return make_float2(s * a.x, s * a.y); }

}  // namespace cmps
