// C ABI of libcmps.so (see include/cmps.h for the contract and the reference lines each entry replaces).
#include "../../include/cmps.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "cmps_internal.h"
#include "cmps_stash_layout_check.h"   // compile-time checks of the stash, ybar-row and scalar-row layouts (this host pass only)

using namespace cmps;

namespace cmps { thread_local KTimer* g_ktimer = nullptr; }

// What the last forward (or the rho sampler) left in the stash of ONE workspace: the reverse and the states entries of that workspace check
// their arguments against it and read its layout.  The main workspace (psi and legacy entries) and the rho workspace have one each.
struct Saved {
    bool valid = false;            // the stash holds the rows of B clips x `steps` steps
    int B = 0, steps = 0;
    const float* audio = nullptr;
    float* loss = nullptr;
    int layout = 0;                // the StashLayout (main workspace) / RhoStashLayout (rho workspace) that was written
    bool bwd_ok = false;           // rho: written by cmps_rho_loss_fwd (not by the sampler), a reverse pass may follow
    bool grad1 = false;            // rho: the GEMM forward accumulated RhoDev::p1
    int k0 = 0;                    // rho: the table row of the first saved step (a cmps_rho_stream segment; else 0)
    int M = 0, n_audio = 0;        // written by cmps_bank_loss_fwd (main) / cmps_rho_bank_loss_fwd (rho) for M members from n_audio batches (0: a plain forward)
};

// What a handle is configured for: nothing yet (or a setter failed half-way), one PsiCMPS model (cmps_set_params*; the RhoCMPS entries
// after cmps_rho_set_state on top of it), the legacy AudioMPS arithmetic (cmps_legacy_set_params), a bank of PsiCMPS models
// (cmps_bank_set_params_dev), or a bank of RhoCMPS models (cmps_rho_bank_set_state_dev: every member's region is the main layout, tables
// only, followed by the rho layout; W is member 0's)
enum Mode { MODE_NONE, MODE_PSI, MODE_LEGACY, MODE_PSI_BANK, MODE_RHO_BANK };

struct cmps_handle_s {
    int D = 0;
    int variant_req = CMPS_VARIANT_AUTO;
    int rank1_mode = CMPS_RANK1_DEFAULT;
    int wide_chain = CMPS_WIDE_CHAIN_MFMA;
    int f16_shift = 0;         // CMPS_OPT_F16_SCALE_SHIFT (diagnostic)
    int bwd_waves = 2;             // CMPS_OPT_BWD_WAVES
    bool rho_virtual_bwd = true;   // CMPS_OPT_RHO_BWD: the RhoCMPS GEMM forward's reverse sweep on virtual clips of k_bwd_wave (else k_bwd_rho_mfma)
    // What the tables of the workspace hold, and so which entries may run.  Two invariants, kept by every setter (the four that install a
    // mode, cmps_rho_set_state and unconfigure()):  bank_M > 0 exactly in the two bank modes;  rho_set only in MODE_PSI.
    Mode mode = MODE_NONE;
    int bank_M = 0;            // the members of the bank (cmps_bank_set_params_dev / cmps_rho_bank_set_state_dev)
    Saved main, rho;           // the stash of the main workspace (cmps_psi_* / cmps_legacy_* entries) and of the rho workspace
    Layout L{};
    Dev P{};                   // (stash_layout stays 0 here: main_dev() fills it from `main` for the kernels that read the stash)
    char* ws = nullptr;
    // time-table cache key: the table is rebuilt only when (workspace, N, dt) changes
    char* tt_ws = nullptr;
    int tt_N = -1;
    float tt_dt = 0.f;
    // RhoCMPS state (cmps_rho_set_state)
    bool rho_set = false;
    int rho_B = 0, rho_T = 0, rho_flags = 0;
    RhoLayout RL{};
    RhoDev W{};
    cmps::KTimer* ktimer = nullptr;   // non-null: CMPS_OPT_KERNEL_EVENTS is on
    std::string err;
};

namespace {

int fail(cmps_handle_t h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

void ktimer_free(cmps::KTimer* t) {
    for (auto& r : t->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : t->pool) (void)hipEventDestroy(e);
    delete t;
}
// sets the thread-local timer for the duration of one C ABI call
struct KBind {
    explicit KBind(cmps_handle_t h) { cmps::g_ktimer = h ? h->ktimer : nullptr; }
    ~KBind() { cmps::g_ktimer = nullptr; }
};

int fail_hip(cmps_handle_t h, hipError_t e, const char* where) {
    if (h) {
        h->err = std::string(where) + ": " + hipGetErrorString(e);
    }
    return CMPS_ERR_HIP;
}

int resolve_variant(const cmps_handle_s* h) {
    if (h->variant_req == CMPS_VARIANT_BLOCK) return CMPS_VARIANT_BLOCK;
    if (h->variant_req == CMPS_VARIANT_WAVE) return h->D <= 32 ? CMPS_VARIANT_WAVE : CMPS_VARIANT_BLOCK;
    if (h->variant_req == CMPS_VARIANT_WAVE32) return h->D <= 32 ? CMPS_VARIANT_WAVE32 : CMPS_VARIANT_BLOCK;
    if (h->variant_req == CMPS_VARIANT_PAIR) return h->D > 32 ? CMPS_VARIANT_PAIR : CMPS_VARIANT_BLOCK;
    if (h->variant_req == CMPS_VARIANT_WIDE) return h->D > 32 ? CMPS_VARIANT_WIDE : CMPS_VARIANT_BLOCK;
    // AUTO: the reference's float32 arithmetic at every D (fp32-faithful products, see cmps.h); the bf16-operand MFMA kernels
    // of 32 < D <= 128 are opt-in (they change the arithmetic)
    return h->D <= 32 ? CMPS_VARIANT_WAVE : CMPS_VARIANT_WIDE;
}

// CMPS_OPT_RANK1 as the wave-per-clip reverse scans understand it: exact fp32, two bf16 pieces, two fp16 pieces (the 32-row kernel of
// the PsiCMPS arithmetic; the legacy mode maps it to three bf16 pieces), or (every other value) three bf16 pieces
int wave_rank1(int mode) {
    if (mode == CMPS_RANK1_DEFAULT) return CMPS_RANK1_F16X2;
    return mode == CMPS_RANK1_EXACT_F32 || mode == CMPS_RANK1_BF16X2 || mode == CMPS_RANK1_F16X2 ? mode : CMPS_RANK1_BF16X3;
}
// the same option where there is only an fp16 and a bf16 form (loss products, samplers, the legacy gradient GEMM): true for two fp16 pieces
bool rank1_f16(int mode) { return mode == CMPS_RANK1_DEFAULT || mode == CMPS_RANK1_F16X2; }
// whether the 32-row family's reverse scan of this handle is the two-wave kernel (k_bwd_wave2w: F16X2 sums only)
bool bwd_two_wave(const cmps_handle_s* h) { return h->bwd_waves == 2 && rank1_f16(h->rank1_mode) && h->f16_shift == 0; }
// Diagnostic builds only (-DCMPS_DIAG -DCMPS_DIAG_YHY_ROWS, scripts/ablate.py): the forward keeps writing (y, H y) rows, so the two-wave
// reverse scan runs its (y, H y) instance -- the behaviour before the normalised rows, for A/B timing.
#if defined(CMPS_DIAG) && defined(CMPS_DIAG_YHY_ROWS)
#undef CMPS_DIAG_YHY_ROWS
#define CMPS_DIAG_YHY_ROWS 1
#else
#define CMPS_DIAG_YHY_ROWS 0
#endif
// ... and as the wide kernels' gradient GEMM takes it: -2 two fp16 pieces, 2 two bf16 pieces, 3 three bf16 pieces
int rank1_wide_pieces(int mode) { return rank1_f16(mode) ? -2 : mode == CMPS_RANK1_BF16X2 ? 2 : 3; }

// The pure-state sampler kernel of a handle (cmps_psi_sample and cmps_psi_sample_primed): wave-per-path for D <= 32, the wide chain's
// sampling mode for 32 < D <= 128 (float32; also what the bf16 pair variant samples with: sampling has no reduced-precision form),
// the block kernel otherwise
enum { SAMPLER_BLOCK, SAMPLER_WAVE, SAMPLER_WIDE };
int sampler_family(const cmps_handle_s* h) {
    const int sv = resolve_variant(h);
    return (sv == CMPS_VARIANT_WAVE || sv == CMPS_VARIANT_WAVE32) ? SAMPLER_WAVE
         : (sv == CMPS_VARIANT_WIDE || sv == CMPS_VARIANT_PAIR)   ? SAMPLER_WIDE : SAMPLER_BLOCK;
}

// The sections of a workspace as the kernels see them: everything a Dev takes from the Layout alone.  The callers add what is their
// own (the scalars; the time table, which the legacy mode does not have).
Dev bind_workspace(const Layout& L, char* ws) {
    const bool train = (L.flags & CMPS_WS_TRAIN) != 0, big = train && L.D > 32;
    Dev P{};
    P.D = L.D; P.DP = L.DP; P.B = L.B; P.T = L.T; P.N = L.N;
    P.R = reinterpret_cast<float2*>(ws + L.off_R);
    P.RT = reinterpret_cast<float2*>(ws + L.off_RT);
    P.Q = reinterpret_cast<float2*>(ws + L.off_Q);
    P.QT = reinterpret_cast<float2*>(ws + L.off_QT);
    P.psi0 = reinterpret_cast<float2*>(ws + L.off_psi0);
    P.freqs = reinterpret_cast<float*>(ws + L.off_freqs);
    P.qflag = reinterpret_cast<unsigned*>(ws + L.off_qflag);
    P.dtk = reinterpret_cast<float*>(ws + L.off_dtk);
    P.rho = reinterpret_cast<float2*>(ws + L.off_rho);
    P.stash = train ? reinterpret_cast<float2*>(ws + L.off_stash) : nullptr;
    P.hst = train ? reinterpret_cast<float*>(ws + L.off_hst) : nullptr;
    P.scal = train ? reinterpret_cast<float*>(ws + L.off_scal) : nullptr;
    P.gops = big ? static_cast<void*>(ws + L.off_gops) : nullptr;
    P.opmax = big ? reinterpret_cast<float*>(ws + L.off_opmax) : nullptr;
    P.slabs = train ? reinterpret_cast<float*>(ws + L.off_slabs) : nullptr;
    P.sums = train ? reinterpret_cast<float*>(ws + L.off_sums) : nullptr;
    P.status = train ? reinterpret_cast<unsigned*>(ws + L.off_status) : nullptr;
    P.slab_floats = L.slab_floats;
    return P;
}

// The sections of a rho workspace as the kernels see them (cmps_rho_set_state; cmps_rho_bank_set_state_dev: member 0's)
RhoDev bind_rho_workspace(int D, const RhoLayout& RL, char* ws, int flags, int B_max) {
    const size_t rD = (size_t)RL.rank * D;
    RhoDev W{};
    W.rank = RL.rank;
    W.phi0 = reinterpret_cast<float2*>(ws + RL.off_phi0);
    const bool train = (flags & CMPS_WS_TRAIN) != 0;
    W.stash = train ? reinterpret_cast<float2*>(ws + RL.off_stash) : nullptr;
    W.scal = train ? reinterpret_cast<float*>(ws + RL.off_scal) : nullptr;
    W.p1 = (train && D <= 32) ? reinterpret_cast<float*>(ws + RL.off_p1) : nullptr;
    W.stash_layout = RHO_STASH_BLOCK;                            // (stays: rho_dev() fills it from the record for the kernels that read the stash)
    W.cols = rD > RHO_LDS_COLS_MAX ? reinterpret_cast<float2*>(ws + RL.off_cols) : nullptr;
    W.cols_blocks = B_max;
    W.slabs = train ? reinterpret_cast<float*>(ws + RL.off_slabs) : nullptr;
    W.sums = train ? reinterpret_cast<float*>(ws + RL.off_sums) : nullptr;
    W.slab_floats = RL.slab_floats;
    W.wslabs = (train && D <= 32) ? reinterpret_cast<float*>(ws + RL.off_wslabs) : nullptr;
    W.wsums = (train && D <= 32) ? reinterpret_cast<float*>(ws + RL.off_wsums) : nullptr;
    W.vrank = RL.vrank;                                          // > 0: the sections of the wide (virtual-clip) path exist
    if (RL.vrank) {
        W.vphi = reinterpret_cast<float2*>(ws + RL.off_vphi);
        W.vstash = reinterpret_cast<float*>(ws + RL.off_vstash);
        W.vgops = reinterpret_cast<float*>(ws + RL.off_vgops);
        W.vopmax = reinterpret_cast<float*>(ws + RL.off_vopmax);
        W.vscal = reinterpret_cast<float*>(ws + RL.off_vscal);
        W.rscal = reinterpret_cast<float*>(ws + RL.off_rscal);
        W.vslabs = reinterpret_cast<float*>(ws + RL.off_vslabs);
        W.vsums = reinterpret_cast<float*>(ws + RL.off_vsums);
        W.vaudio = reinterpret_cast<float*>(ws + RL.off_vaudio);
        W.gphi = reinterpret_cast<float*>(ws + RL.off_gphi);
        W.vslab_floats = RL.vslab_floats;
    }
    return W;
}

// The Dev / RhoDev of a call that reads a stash: B clips, the layout from the workspace's record
Dev main_dev(const cmps_handle_s* h, int B) {
    Dev P = h->P;
    P.B = B;
    P.stash_layout = h->main.layout;
    return P;
}
RhoDev rho_dev(const cmps_handle_s* h) {
    RhoDev W = h->W;
    W.stash_layout = h->rho.layout;
    return W;
}

// The one call-order check: entry `who` runs in the modes of the set `accepted` (bits 1 << Mode), and only where `also` holds (what the
// entry needs beside the mode: cmps_rho_set_state, a saved forward, a CMPS_WS_TRAIN workspace).  Otherwise the message is `who` and the
// refusal (in up to three pieces, so that an accepted call builds no string).
constexpr unsigned in(Mode m) { return 1u << m; }
constexpr unsigned BANKS = in(MODE_PSI_BANK) | in(MODE_RHO_BANK);
int need_mode(cmps_handle_t h, const char* who, unsigned accepted, bool also, const char* refusal, const char* r2 = "", const char* r3 = "") {
    if ((accepted & in(h->mode)) && also) return CMPS_OK;
    return fail(h, CMPS_ERR_STATE, std::string(who) + refusal + r2 + r3);
}
// What a setter leaves behind when a launch fails after it has begun to overwrite the tables
void unconfigure(cmps_handle_t h) {
    h->mode = MODE_NONE;
    h->bank_M = 0;
    h->rho_set = false;
    h->main.valid = h->rho.valid = false;
    h->tt_ws = nullptr;                  // (the time table may be half written)
}

// The argument checks of every *_loss_fwd entry (h non-null): `modes` and `also` are the entry's call-order condition (need_mode),
// T_set / B_max / ws_flags what `setter` was given.  CMPS_OK, or the code to return with the message set.
int check_fwd(cmps_handle_t h, const char* who, unsigned modes, bool also, const char* setter, const void* audio, const void* loss, int B, int T,
              int T_set, int B_max, int save, int ws_flags) {
    const std::string w(who);
    if (const int rc = need_mode(h, who, modes, also, ": call ", setter, " first")) return rc;
    if (!audio || !loss) return fail(h, CMPS_ERR_BAD_ARG, w + ": null pointer");
    if (T != T_set) return fail(h, CMPS_ERR_BAD_ARG, w + ": T differs from " + setter);
    if (B < 1 || B > B_max) return fail(h, CMPS_ERR_BAD_ARG, w + ": B outside [1, B_max] of " + setter);
    if (save && !(ws_flags & CMPS_WS_TRAIN)) return fail(h, CMPS_ERR_WORKSPACE, w + ": save_for_bwd needs a CMPS_WS_TRAIN workspace in " + setter);
    return CMPS_OK;
}
// ... and of every *_loss_bwd entry, against the record S of the forward `fwd` it follows
int check_bwd(cmps_handle_t h, const char* who, unsigned modes, bool also, const char* fwd, const Saved& S, const void* audio, const void* grad,
              int B, int T) {
    const std::string w(who);
    if (const int rc = need_mode(h, who, modes, also && S.valid, ": needs ", fwd, "(save_for_bwd=1) first")) return rc;
    if (!audio || !grad) return fail(h, CMPS_ERR_BAD_ARG, w + ": null pointer");
    if (B != S.B || T != S.steps + 1 || audio != S.audio) return fail(h, CMPS_ERR_STATE, w + ": audio / B / T differ from the forward call");
    return CMPS_OK;
}
// What the four *_apply_step entries ask of an update (grad_sums non-null) and of their double-precision buffers (hyper: the bank entries')
int check_apply_step(cmps_handle_t h, const char* who, const float* grad_sums, const float* adam_m, const float* adam_v, const float* losses,
                     const void* scratch, double global_batch, const double* hyper = nullptr) {
    const std::string w(who);
    if (grad_sums && (!adam_m || !adam_v || !losses || !scratch || !(global_batch > 0.0)))
        return fail(h, CMPS_ERR_BAD_ARG, w + ": an update needs the Adam slots, losses_dev, scratch_dev and a positive batch");
    if (((uintptr_t)scratch & 7) != 0) return fail(h, CMPS_ERR_BAD_ARG, w + ": scratch_dev must be 8-byte aligned");
    if (((uintptr_t)hyper & 7) != 0) return fail(h, CMPS_ERR_BAD_ARG, w + ": hyper_dev must be 8-byte aligned");
    return CMPS_OK;
}
// The member strides of a bank launch, in floats: between two members' batches (0: one shared batch), loss rows and gradient rows
void bank_strides(Dev& P, int n_audio, int B, int T, size_t grad = 0) {
    P.bank_audio = n_audio == 1 ? 0 : (size_t)B * T;
    P.bank_loss = (size_t)B;
    P.bank_grad = grad;                  // (a forward: 0, the value h->P holds anyway; no forward kernel reads it)
}
// What every plain entry outside a bank's scope (samplers, streams, state read-outs, ancilla updates, cmps_rho_set_state,
// cmps_psi_grad_status) answers while the workspace holds a bank: its tables would be member 0's alone.  A member is taken out as a plain model.
int check_not_bank(cmps_handle_t h, const char* who) {
    return need_mode(h, who, ~BANKS, true, ": the handle holds a bank (cmps_bank_set_params_dev / cmps_rho_bank_set_state_dev); call cmps_set_params for one model first");
}
// ... and then its own call-order check
int need_plain(cmps_handle_t h, const char* who, unsigned accepted, bool also, const char* refusal) {
    if (const int rc = check_not_bank(h, who)) return rc;
    return need_mode(h, who, accepted, also, refusal);
}

// The small argument checks of the entries that need nothing of the handle but its error string: chained, the first that fails speaks
// (CMPS_ERR_BAD_ARG, in rc), the ones behind it do nothing; a passing check builds no string
struct Args {
    cmps_handle_t h;
    const char* who;
    int rc = CMPS_OK;
    Args& need(bool ok, std::initializer_list<const char*> sentence) {
        if (rc || ok) return *this;
        std::string msg = std::string(who) + ": ";
        for (const char* piece : sentence) msg += piece;
        rc = fail(h, CMPS_ERR_BAD_ARG, msg);
        return *this;
    }
    Args& need(bool ok, const char* sentence) { return need(ok, {sentence}); }
    Args& ptr(const char* name, const void* p) { return need(p != nullptr, {name, " is a null pointer"}); }
    Args& align8(const char* name, const void* p) { return need(((uintptr_t)p & 7) == 0, {name, " must be 8-byte aligned"}); }
    Args& min1(const char* name, long long v) { return need(v >= 1, {"need ", name, " >= 1"}); }
    Args& members(int M) { return need(M >= 1 && M <= CLASSIFY_MAX_M, "need 1 <= M <= 1024"); }
    Args& ld(const char* name, long long ld, int B) { return need(ld >= (long long)B, {name, " must be at least B"}); }
    Args& positive(const char* name, double v) { return need(std::isfinite(v) && v > 0.0, {name, " must be finite and positive"}); }
    Args& not_negative(const char* name, double v) { return need(std::isfinite(v) && v >= 0.0, {name, " must be finite and not negative"}); }
    // `count` consecutive ids or steps from `first` on stay below 2^63 (`a_thing`: "an id", "a step"; count >= 1 was checked before)
    Args& range63(const char* first_name, long long first, const char* count_name, long long count, const char* a_thing) {
        return need(rc || (first >= 0 && first <= 9223372036854775807ll - count),
                    {"need ", first_name, " >= 0 and ", first_name, " + ", count_name, " below 2^63 (", a_thing, " is a signed 64-bit integer)"});
    }
};

// The tail of an entry that is one launch: bind the handle's kernel-event record, time the launch under the name `kernel`, and turn a HIP
// error into the entry's code and message (`where` names the entry)
template <class Launch>
int run_kernel(cmps_handle_t h, const char* where, const char* kernel, void* stream, Launch&& launch) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    KBind kb(h);
    KScope ks(kernel, s);
    const hipError_t e = launch(s);
    return e == hipSuccess ? CMPS_OK : fail_hip(h, e, where);
}

// the end of a reverse pass whose slabs hold one PAIR of clips each (pair and wide kernels): reduce over (B + 1) / 2 slabs, closing terms
hipError_t reduce_pairs_finalize(Dev P, int abar_fix, const float* loss, float* grad_out, hipStream_t s) {
    Dev Pp = P;
    Pp.B = (P.B + 1) / 2;
    KScope ks("reduce + finalize", s);
    hipError_t e = launch_reduce_only(Pp, s);
    P.abar_fix = abar_fix;
    if (e == hipSuccess) e = launch_finalize_only(P, loss, grad_out, s);
    return e;
}

}  // namespace

extern "C" {

int cmps_version(void) { return 500; }

int cmps_create(int D, cmps_handle_t* out) {
    if (!out) return CMPS_ERR_BAD_ARG;
    *out = nullptr;
    if (D < 1 || D > 128) return CMPS_ERR_UNSUPPORTED_D;
    cmps_handle_s* h = new (std::nothrow) cmps_handle_s();
    if (!h) return CMPS_ERR_BAD_ARG;
    h->D = D;
    *out = h;
    return CMPS_OK;
}

int cmps_destroy(cmps_handle_t h) {
    if (h && h->ktimer) ktimer_free(h->ktimer);
    delete h;
    return CMPS_OK;
}

const char* cmps_last_error(cmps_handle_t h) { return h ? h->err.c_str() : "null handle"; }

int cmps_set_variant(cmps_handle_t h, int variant) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (variant < CMPS_VARIANT_AUTO || variant > CMPS_VARIANT_WIDE)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_variant: unknown variant");
    if ((variant == CMPS_VARIANT_PAIR || variant == CMPS_VARIANT_WIDE) && h->D <= 32)
        return fail(h, CMPS_ERR_UNSUPPORTED_D, "cmps_set_variant: the pair (bf16 MFMA) and wide (float32) variants are for 32 < D <= 128");
    if ((variant == CMPS_VARIANT_WAVE || variant == CMPS_VARIANT_WAVE32) && h->D > 32)
        return fail(h, CMPS_ERR_UNSUPPORTED_D, "cmps_set_variant: the wave variant needs D <= 32");
    h->variant_req = variant;
    return CMPS_OK;
}

int cmps_get_variant(cmps_handle_t h) { return h ? resolve_variant(h) : 0; }

int cmps_set_option(cmps_handle_t h, int option, int value) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (option == CMPS_OPT_RANK1) {
        if (value < CMPS_RANK1_EXACT_F32 || value > CMPS_RANK1_DEFAULT)
            return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: unknown value for CMPS_OPT_RANK1");
        h->rank1_mode = value;
        return CMPS_OK;
    }
    if (option == CMPS_OPT_WIDE_CHAIN) {
        if (value < CMPS_WIDE_CHAIN_VALU || value > CMPS_WIDE_CHAIN_MFMA_FWD)
            return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: unknown value for CMPS_OPT_WIDE_CHAIN");
        h->wide_chain = value;
        return CMPS_OK;
    }
    if (option == CMPS_OPT_BWD_WAVES) {
        if (value != 1 && value != 2) return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: CMPS_OPT_BWD_WAVES takes 1 or 2");
        h->bwd_waves = value;
        return CMPS_OK;
    }
    if (option == CMPS_OPT_RHO_BWD) {
        if (value != CMPS_RHO_BWD_VIRTUAL && value != CMPS_RHO_BWD_GEMM) return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: unknown value for CMPS_OPT_RHO_BWD");
        h->rho_virtual_bwd = value == CMPS_RHO_BWD_VIRTUAL;
        return CMPS_OK;
    }
    if (option == CMPS_OPT_F16_SCALE_SHIFT) {
        if (value < -40 || value > 40) return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: CMPS_OPT_F16_SCALE_SHIFT takes -40 .. 40");
        h->f16_shift = value;
        return CMPS_OK;
    }
    if (option == CMPS_OPT_KERNEL_EVENTS) {
        if (value != 0 && value != 1) return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: CMPS_OPT_KERNEL_EVENTS takes 0 or 1");
        if (value && !h->ktimer) h->ktimer = new cmps::KTimer();
        if (!value && h->ktimer) { ktimer_free(h->ktimer); h->ktimer = nullptr; }
        return CMPS_OK;
    }
    if (option == CMPS_OPT_SAVED_ROWS) return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: CMPS_OPT_SAVED_ROWS is read-only");
    return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_option: unknown option");
}

int cmps_get_option(cmps_handle_t h, int option) {
    if (!h) return -1;
    if (option == CMPS_OPT_RANK1) return h->rank1_mode;
    if (option == CMPS_OPT_KERNEL_EVENTS) return h->ktimer ? 1 : 0;
    if (option == CMPS_OPT_WIDE_CHAIN) return h->wide_chain;
    if (option == CMPS_OPT_F16_SCALE_SHIFT) return h->f16_shift;
    if (option == CMPS_OPT_BWD_WAVES) return h->bwd_waves;
    if (option == CMPS_OPT_RHO_BWD) return h->rho_virtual_bwd ? CMPS_RHO_BWD_VIRTUAL : CMPS_RHO_BWD_GEMM;
    if (option == CMPS_OPT_SAVED_ROWS) return h->main.valid && h->main.layout == STASH_WAVE32N ? 1 : 0;
    return -1;
}

size_t cmps_workspace_bytes(int D, int B, int T, int flags) {
    if (D < 1 || D > 128 || B < 1 || T < 2) return 0;
    return make_layout(D, B, T, flags & ~(CMPS_WS_FRESH | CMPS_WS_REUSE_TABLES)).total;
}

static int set_params_impl(cmps_handle_t h, const float* R_re_dev, const float* R_im_dev,
                           const float* freqs_dev, const float* psi0_re_dev, const float* psi0_im_dev,
                           float A, const float* A_dev, double sigma, double delta_t, int T, int B_max, int flags,
                           void* workspace_dev, size_t workspace_bytes, void* stream, Mode mode = MODE_PSI, int M = 0, size_t rho_bytes = 0) {
    // `mode` is what the call installs; the entry of that mode speaks in the messages
    const std::string w(mode == MODE_RHO_BANK ? "cmps_rho_bank_set_state_dev" : mode == MODE_PSI_BANK ? "cmps_bank_set_params_dev" : "cmps_set_params");
    // MODE_PSI_BANK (cmps_bank_set_params_dev, which has checked its own arguments): M > 0, the parameter pointers are member 0's, member
    // m's lie m (2 D^2 + 3 D + 1) floats behind them, and member m's workspace is the plain layout at byte m * L.total.
    // MODE_RHO_BANK (cmps_rho_bank_set_state_dev, with the flags of a tables-only main layout): every member's rho layout of rho_bytes
    // bytes follows its main layout, and the stride is their sum; the caller packs the columns and fills W.
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!R_re_dev || !R_im_dev || !freqs_dev || !psi0_re_dev || !psi0_im_dev)
        return fail(h, CMPS_ERR_BAD_ARG, w + ": null parameter pointer");
    if (T < 2 || B_max < 1) return fail(h, CMPS_ERR_BAD_ARG, w + ": need T >= 2 and B_max >= 1");
    if (!workspace_dev) return fail(h, CMPS_ERR_WORKSPACE, w + ": null workspace");
    // the cached time table is trusted only when the caller says the workspace is untouched (and never with CMPS_WS_FRESH)
    const bool fresh = (flags & CMPS_WS_FRESH) != 0 || (flags & CMPS_WS_REUSE_TABLES) == 0;
    flags &= ~(CMPS_WS_FRESH | CMPS_WS_REUSE_TABLES);
    Layout L = make_layout(h->D, B_max, T, flags);
    const size_t members = M > 0 ? (size_t)M : 1, n_par = 2 * (size_t)h->D * h->D + 3 * (size_t)h->D + 1;
    const size_t stride = L.total + rho_bytes;
    if (workspace_bytes < members * stride) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: workspace has %zu bytes, needs %zu", w.c_str(), workspace_bytes,
                 members * stride);
        return fail(h, CMPS_ERR_WORKSPACE, buf);
    }
    if (((uintptr_t)workspace_dev & 255) != 0)
        return fail(h, CMPS_ERR_WORKSPACE, w + ": workspace must be 256-byte aligned");
    char* ws = static_cast<char*>(workspace_dev);
    Dev P = bind_workspace(L, ws);
    P.ttab = reinterpret_cast<float*>(ws + L.off_ttab);
    P.A = A;
    P.Adev = A_dev;
    // model.py:312: `- self.delta_t * self.sigma**2` is a Python float (double), cast to complex64,
    // multiplied in, then divided by 2. (exact halving)
    P.c_half = (float)(-delta_t * sigma * sigma) / 2.0f;
    const float dt = (float)delta_t;  // model.py:16
    P.dt = dt;
    if (M > 0) { P.bank_stride = stride; P.bank_adev = n_par; }
    // (a bank's members each have a time table: another member count or stride, or a change between bank and plain mode, moves or adds tables)
    const bool regrouped = h->bank_M != M || h->P.bank_stride != P.bank_stride;
    const bool rebuild = fresh || regrouped || !(h->tt_ws == ws && h->tt_N == L.N && h->tt_dt == dt);
    hipError_t e = launch_prep(P, R_re_dev, R_im_dev, freqs_dev, psi0_re_dev, psi0_im_dev, dt, rebuild,
                               const_cast<float*>(P.ttab), const_cast<float*>(P.dtk),
                               const_cast<float2*>(P.R), const_cast<float2*>(P.RT),
                               const_cast<float2*>(P.Q), const_cast<float2*>(P.psi0),
                               const_cast<float*>(P.freqs), const_cast<float2*>(P.rho),
                               reinterpret_cast<double2*>(ws + L.off_rfix), static_cast<hipStream_t>(stream), (int)members, M > 0 ? n_par : 0);
    if (e != hipSuccess) { unconfigure(h); return fail_hip(h, e, w.c_str()); }
    // a workspace this handle cannot vouch for, or flag words that moved: the layout puts them behind the stash and the slabs, so with
    // CMPS_WS_REUSE_TABLES and another T, B_max or TRAIN flag (or after another mode) their address holds something else -- the flag
    // words start at zero
    if (P.status && (fresh || h->ws != ws || h->mode != mode || regrouped || h->P.status != P.status)) {
        // (every member's pair of words, one workspace apart: one strided fill)
        e = M > 0 ? hipMemset2DAsync(P.status, stride, 0, 2 * sizeof(unsigned), members, static_cast<hipStream_t>(stream))
                  : hipMemsetAsync(P.status, 0, 2 * sizeof(unsigned), static_cast<hipStream_t>(stream));
        if (e != hipSuccess) { unconfigure(h); return fail_hip(h, e, (w + " (status words)").c_str()); }
    }
    h->tt_ws = ws; h->tt_N = L.N; h->tt_dt = dt;
    h->L = L; h->P = P; h->ws = ws;
    h->mode = mode;
    h->bank_M = M;
    h->main.valid = false;
    h->rho_set = false;               // the columns of rho_0 are handed over again after every parameter change
    h->rho.valid = false;
    return CMPS_OK;
}

int cmps_set_params(cmps_handle_t h, const float* R_re_dev, const float* R_im_dev,
                    const float* freqs_dev, const float* psi0_re_dev, const float* psi0_im_dev,
                    float A, double sigma, double delta_t, int T, int B_max, int flags,
                    void* workspace_dev, size_t workspace_bytes, void* stream) {
    return set_params_impl(h, R_re_dev, R_im_dev, freqs_dev, psi0_re_dev, psi0_im_dev, A, nullptr, sigma, delta_t, T, B_max, flags,
                           workspace_dev, workspace_bytes, stream);
}

// set_params_impl on the packed buffer R_re | R_im | freqs | psi0_re | psi0_im | A that the apply-step entries write (a bank's: member 0's row)
static int set_params_packed(cmps_handle_t h, const float* params_dev, double sigma, double delta_t, int T, int B_max, int flags,
                             void* workspace_dev, size_t workspace_bytes, void* stream, Mode mode = MODE_PSI, int M = 0, size_t rho_bytes = 0) {
    const size_t DD = (size_t)h->D * h->D, D = (size_t)h->D;
    return set_params_impl(h, params_dev, params_dev + DD, params_dev + 2 * DD, params_dev + 2 * DD + D, params_dev + 2 * DD + 2 * D,
                           0.f, params_dev + 2 * DD + 3 * D, sigma, delta_t, T, B_max, flags, workspace_dev, workspace_bytes, stream, mode, M,
                           rho_bytes);
}

int cmps_set_params_dev(cmps_handle_t h, const float* params_dev, double sigma, double delta_t, int T, int B_max, int flags,
                        void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!params_dev) return fail(h, CMPS_ERR_BAD_ARG, "cmps_set_params_dev: null parameter buffer");
    return set_params_packed(h, params_dev, sigma, delta_t, T, B_max, flags, workspace_dev, workspace_bytes, stream);
}

size_t cmps_apply_step_scratch_bytes(int D) { return (D < 1 || D > 128) ? 0 : apply_step_scratch_bytes(D); }

int cmps_psi_apply_step(cmps_handle_t h, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev,
                        double global_batch, double lr_t, double beta1, double beta2, double epsilon, double h_reg, double r_reg,
                        double c_r, double c_h, int with_reg, float* params_dev, float* losses_dev, void* scratch_dev,
                        void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!vars_dev || !params_dev) return fail(h, CMPS_ERR_BAD_ARG, "cmps_psi_apply_step: null variable / parameter buffer");
    if (const int rc = check_apply_step(h, "cmps_psi_apply_step", grad_sums_dev, adam_m_dev, adam_v_dev, losses_dev, scratch_dev, global_batch)) return rc;
    const bool apply = grad_sums_dev != nullptr;
    const hipError_t e = launch_apply_step(h->D, apply, apply ? 1.0 / global_batch : 0.0, lr_t, beta1, beta2, epsilon, h_reg, r_reg, c_r,
                                           c_h, with_reg != 0, vars_dev, adam_m_dev, adam_v_dev, grad_sums_dev, params_dev, losses_dev,
                                           static_cast<double*>(scratch_dev), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_psi_apply_step");
    return CMPS_OK;
}

size_t cmps_rho_apply_step_scratch_bytes(int D, int rank) {
    return (D < 1 || D > 128 || rank < 1 || rank > 128) ? 0 : rho_apply_step_scratch_bytes(D, rank);
}

int cmps_rho_apply_step(cmps_handle_t h, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev,
                        int rank, double global_batch, double lr_t, double beta1, double beta2, double epsilon, double h_reg,
                        double r_reg, double c_r, double c_h, int with_reg, float* params_dev, float* phi_dev, float* losses_dev,
                        void* scratch_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!vars_dev || !params_dev || !phi_dev)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_apply_step: null variable / parameter / column buffer");
    if (rank < 1 || rank > 128) return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_apply_step: rank outside [1, 128]");
    if (const int rc = check_apply_step(h, "cmps_rho_apply_step", grad_sums_dev, adam_m_dev, adam_v_dev, losses_dev, scratch_dev, global_batch)) return rc;
    const bool apply = grad_sums_dev != nullptr;
    const hipError_t e = launch_rho_apply_step(h->D, rank, apply, apply ? 1.0 / global_batch : 0.0, lr_t, beta1, beta2, epsilon, h_reg,
                                               r_reg, c_r, c_h, with_reg != 0, vars_dev, adam_m_dev, adam_v_dev, grad_sums_dev,
                                               params_dev, phi_dev, losses_dev, static_cast<double*>(scratch_dev),
                                               static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_rho_apply_step");
    return CMPS_OK;
}

// cmps_psi_loss_fwd (M = 0) and cmps_bank_loss_fwd (M members, n_audio batches) behind their argument checks
static int psi_fwd_run(cmps_handle_t h, const char* who, int M, int n_audio, const float* audio_dev, int B, int T, float* loss_dev,
                       int save_for_bwd, void* stream) {
    Dev P = h->P;
    P.B = B;
    const int Mk = M > 0 ? M : 1;
    if (M > 0) bank_strides(P, n_audio, B, T);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int variant = resolve_variant(h);
    KBind kb(h);
    // the kernel family, named by the stash layout it writes
    const bool wave = variant == CMPS_VARIANT_WAVE || variant == CMPS_VARIANT_WAVE32;
    const int family = variant == CMPS_VARIANT_WAVE && h->D <= 16 ? STASH_WAVE16 : wave ? STASH_WAVE32
                     : variant == CMPS_VARIANT_PAIR ? STASH_PAIR : variant == CMPS_VARIANT_WIDE ? STASH_WIDE : STASH_BLOCK;
    const bool save = save_for_bwd != 0, f16 = rank1_f16(h->rank1_mode);
    // The rows of the 32-row family are written normalised (STASH_WAVE32N) when the reverse pass of this handle will be k_bwd_wave2w:
    // decided from the options NOW and recorded; cmps_psi_loss_bwd follows the record.
    const bool norm_rows = save && family == STASH_WAVE32 && bwd_two_wave(h) && !CMPS_DIAG_YHY_ROWS;
    hipError_t e;
    switch (family) {
    case STASH_WAVE16: { KScope ks("k_fwd_wave16", s); e = launch_fwd_wave16(P, audio_dev, loss_dev, save, s, Mk); } break;
    // the loss product's pieces follow CMPS_OPT_RANK1 like the reverse scan's rank-1 sums: two fp16 pieces for F16X2 / DEFAULT
    case STASH_WAVE32: { KScope ks("k_fwd_wave2", s); e = launch_fwd_wave2(P, audio_dev, loss_dev, save, f16, norm_rows, s, Mk); } break;
    case STASH_PAIR: { KScope ks("k_fwd_pair", s); e = launch_fwd_pair(P, audio_dev, loss_dev, save, s); } break;
    // k_fwd_wide, k_hy_wide, k_loss_wide (scopes inside); the loss product's pieces follow CMPS_OPT_RANK1 like the gradient GEMM's
    case STASH_WIDE: e = launch_fwd_wide(P, audio_dev, loss_dev, save, f16, h->wide_chain != CMPS_WIDE_CHAIN_VALU, s); break;
    default: { KScope ks("k_fwd_block", s); e = launch_fwd_block(P, audio_dev, loss_dev, save, s, Mk); } break;
    }
    if (e != hipSuccess) return fail_hip(h, e, who);
    h->main = Saved{save, B, T - 1, audio_dev, loss_dev, norm_rows ? (int)STASH_WAVE32N : family};
    h->main.M = M; h->main.n_audio = M > 0 ? n_audio : 0;
    return CMPS_OK;
}

int cmps_psi_loss_fwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* loss_dev,
                      int save_for_bwd, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_fwd(h, "cmps_psi_loss_fwd", in(MODE_PSI), true, "cmps_set_params", audio_dev, loss_dev, B, T, h->L.T, h->L.B,
                                 save_for_bwd, h->L.flags)) return rc;
    return psi_fwd_run(h, "cmps_psi_loss_fwd", 0, 0, audio_dev, B, T, loss_dev, save_for_bwd, stream);
}

// cmps_psi_loss_bwd (M = 0) and cmps_bank_loss_bwd behind their argument checks
// (weight non-null, cmps_bank_loss_bwd_weighted: the same reverse scan, the cross-clip reduction weighted by weight[m * ldw + b])
static int psi_bwd_run(cmps_handle_t h, const char* who, int M, int n_audio, const float* audio_dev, int B, int T, float* grad_dev, void* stream,
                       const float* weight = nullptr, long long ldw = 0) {
    const auto failed = [&](hipError_t e, const char* stage) { return fail_hip(h, e, (std::string(who) + stage).c_str()); };
    Dev P = main_dev(h, B);
    const int Mk = M > 0 ? M : 1;
    if (M > 0) bank_strides(P, n_audio, B, T, 2 * (size_t)h->D * h->D + 3 * (size_t)h->D + 2);
    P.f16_shift = h->f16_shift;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the reverse kernels belong to the family whose forward wrote the stash
    const int layout = h->main.layout;
    float* const loss = h->main.loss;
    KBind kb(h);
    if (layout == STASH_PAIR) {
        // reverse scan, then the gradient GEMM over the rows both scans left behind; one slab per PAIR of clips
        hipError_t e;
        { KScope ks("k_bwd_pair", s); e = launch_bwd_pair(P, audio_dev, s); }
        if (e == hipSuccess) { KScope ks("k_grad_gemm<1>", s); e = launch_grad_pair(P, audio_dev, s); }
        if (e != hipSuccess) return failed(e, " (pair scan)");
        e = reduce_pairs_finalize(P, 0, loss, grad_dev, s);
        if (e != hipSuccess) return failed(e, " (pair reduce)");
        return CMPS_OK;
    }
    if (layout == STASH_WIDE) {
        // float32 reverse scan, then the gradient GEMM (operands split into bf16 pieces on the fly); one slab per PAIR of clips
        hipError_t e;
        if (h->wide_chain == CMPS_WIDE_CHAIN_MFMA) { KScope ks("k_bwd_chain16", s); e = launch_bwd_chain16(P, audio_dev, s); }
        else { KScope ks("k_bwd_wide", s); e = launch_bwd_wide(P, audio_dev, s); }
        if (e == hipSuccess) {
            const int pieces = rank1_wide_pieces(h->rank1_mode);
            KScope ks(pieces == -2 ? "k_grad_gemm<f16x2>" : pieces == 2 ? "k_grad_gemm<2>" : "k_grad_gemm<3>", s);
            e = launch_grad_wide(P, audio_dev, pieces, s);
        }
        if (e != hipSuccess) return failed(e, " (wide scan)");
        // abar_fix: the merged mat-vec, k_finalize removes the Q part of sum Re(u^dagger (Q + s R^dagger) ybar)
        e = reduce_pairs_finalize(P, 1, loss, grad_dev, s);
        if (e != hipSuccess) return failed(e, " (wide reduce)");
        return CMPS_OK;
    }
    const bool w16 = layout == STASH_WAVE16, norm_rows = layout == STASH_WAVE32N, wave = w16 || layout == STASH_WAVE32 || norm_rows;
    hipError_t e;
    {
        // normalised rows have one reader, k_bwd_wave2w (the forward wrote them for it): options that changed since the forward do not
        // move the reverse pass of THAT forward to a kernel that would misread them
        const bool two = norm_rows || (wave && !w16 && bwd_two_wave(h));
        KScope ks(!wave ? "k_bwd_block" : w16 ? "k_bwd_wave16" : two ? "k_bwd_wave2w" : "k_bwd_wave", s);
        e = !wave ? launch_bwd_block(P, audio_dev, s, Mk) : w16 ? launch_bwd_wave16(P, audio_dev, s, Mk)
          : two ? launch_bwd_wave2w(P, audio_dev, s, Mk) : launch_bwd_wave(P, audio_dev, wave_rank1(h->rank1_mode), s);
    }
    if (e != hipSuccess) return failed(e, " (scan)");
    P.abar_fix = wave ? 1 : 0;
    KScope ks(weight ? "reduce + finalize (weighted)" : "reduce + finalize", s);
    e = weight ? launch_reduce_finalize_weighted(P, loss, grad_dev, weight, ldw, s, Mk) : launch_reduce_finalize(P, loss, grad_dev, s, Mk);
    if (e != hipSuccess) return failed(e, " (reduce)");
    return CMPS_OK;
}

int cmps_psi_loss_bwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* grad_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_bwd(h, "cmps_psi_loss_bwd", in(MODE_PSI), h->main.M == 0, "cmps_psi_loss_fwd", h->main, audio_dev, grad_dev, B, T))
        return rc;
    return psi_bwd_run(h, "cmps_psi_loss_bwd", 0, 0, audio_dev, B, T, grad_dev, stream);
}

int cmps_psi_grad_status(cmps_handle_t h, int* sticky_out, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_not_bank(h, "cmps_psi_grad_status")) return rc;
    if (sticky_out) *sticky_out = 0;
    if (const int rc = need_mode(h, "cmps_psi_grad_status", in(MODE_PSI), h->P.status != nullptr, ": needs cmps_set_params with a CMPS_WS_TRAIN workspace"))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned words[2] = {0u, 0u};
    hipError_t e = hipMemcpyAsync(words, h->P.status, sizeof words, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->P.status + 1, 0, sizeof(unsigned), s);        // the sticky word restarts
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail_hip(h, e, "cmps_psi_grad_status");
    if (sticky_out) *sticky_out = (int)words[1];
    if ((words[0] & 1u) && !(words[0] & 2u))
        return fail(h, CMPS_ERR_F16_RANGE,
                    "cmps_psi_grad_status: the gradient sums of the last cmps_psi_loss_bwd hold Inf / NaN although every per-clip loss is "
                    "finite: an fp16-split operand left its scaled range.  Fallback: CMPS_OPT_RANK1 = BF16X3, CMPS_OPT_WIDE_CHAIN = VALU, "
                    "then repeat cmps_psi_loss_fwd / _bwd");
    return CMPS_OK;
}

// ---- model bank: M same-shape PsiCMPS models per launch (include/cmps.h) ----

constexpr int BANK_MAX = 1024;

// What every bank entry that launches scans refuses before it looks at its arguments: the kernel families without a member dimension
// (wide / pair: AUTO above D = 32), the legacy tables, and the options that would select the one-wave k_bwd_wave or change its scales.
static int bank_check_mode(cmps_handle_t h, const char* who, bool tables) {
    const std::string w(who);
    if (h->D > 32 && resolve_variant(h) != CMPS_VARIANT_BLOCK)
        return fail(h, CMPS_ERR_UNSUPPORTED_D, w + ": a bank above D = 32 needs CMPS_VARIANT_BLOCK (the wide and pair kernels have no member dimension)");
    if (tables) if (const int rc = need_mode(h, who, ~in(MODE_LEGACY), true, ": not available in legacy mode")) return rc;
    if (h->rank1_mode != CMPS_RANK1_DEFAULT || h->bwd_waves != 2 || h->f16_shift != 0)
        return fail(h, CMPS_ERR_STATE, w + ": a bank runs with the default CMPS_OPT_RANK1, CMPS_OPT_BWD_WAVES and CMPS_OPT_F16_SCALE_SHIFT only");
    return CMPS_OK;
}
static int bank_check_M(cmps_handle_t h, const char* who, int M) {
    if (M < 1 || M > BANK_MAX) return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": M outside [1, 1024]");
    return CMPS_OK;
}
static int bank_check_shape(cmps_handle_t h, const char* who, int M, int B, int T) {
    const std::string w(who);
    if (B < 1 || T < 2) return fail(h, CMPS_ERR_BAD_ARG, w + ": need B >= 1 and T >= 2");
    if ((unsigned long long)M * (unsigned long long)B * (unsigned long long)T > 0x7fffffffull)
        return fail(h, CMPS_ERR_BAD_ARG, w + ": M * B * T overflows");
    return CMPS_OK;
}

size_t cmps_bank_workspace_bytes(int D, int M, int B, int T, int flags) {
    if (M < 1 || M > BANK_MAX) return 0;
    return (size_t)M * cmps_workspace_bytes(D, B, T, flags);
}

int cmps_bank_set_params_dev(cmps_handle_t h, int M, const float* params_dev, double sigma, double delta_t, int T, int B_max, int flags,
                             void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "cmps_bank_set_params_dev";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = bank_check_mode(h, who, false)) return rc;
    if (!params_dev) return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": null parameter buffer");
    if (const int rc = bank_check_M(h, who, M)) return rc;
    if (const int rc = bank_check_shape(h, who, M, B_max, T)) return rc;
    if (!workspace_dev) return fail(h, CMPS_ERR_WORKSPACE, std::string(who) + ": null workspace");
    return set_params_packed(h, params_dev, sigma, delta_t, T, B_max, flags, workspace_dev, workspace_bytes, stream, MODE_PSI_BANK, M);
}

int cmps_bank_loss_fwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* loss_dev, int save_for_bwd, void* stream) {
    const char* who = "cmps_bank_loss_fwd";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = bank_check_mode(h, who, true)) return rc;
    if (const int rc = check_fwd(h, who, in(MODE_PSI_BANK), true, "cmps_bank_set_params_dev", audio_dev, loss_dev, B, T, h->L.T, h->L.B,
                                 save_for_bwd, h->L.flags)) return rc;
    if (n_audio != 1 && n_audio != h->bank_M) return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": n_audio must be 1 (one shared batch) or M");
    return psi_fwd_run(h, who, h->bank_M, n_audio, audio_dev, B, T, loss_dev, save_for_bwd, stream);
}

int cmps_bank_loss_bwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* grad_dev, void* stream) {
    const char* who = "cmps_bank_loss_bwd";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = bank_check_mode(h, who, true)) return rc;
    if (const int rc = check_bwd(h, who, in(MODE_PSI_BANK), h->main.M == h->bank_M, "cmps_bank_loss_fwd", h->main, audio_dev, grad_dev, B, T)) return rc;
    if (n_audio != h->main.n_audio) return fail(h, CMPS_ERR_STATE, std::string(who) + ": n_audio differs from the forward call");
    return psi_bwd_run(h, who, h->bank_M, n_audio, audio_dev, B, T, grad_dev, stream);
}

// cmps_bank_loss_bwd with a cotangent per clip and member.  Its own two checks come first, so that they answer on any handle; then
// cmps_bank_loss_bwd's.  PsiCMPS banks only: a RhoCMPS bank's reverse pass runs `rank` virtual clips per clip and closes with kernels of its own.
int cmps_bank_loss_bwd_weighted(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, const float* weight_dev, long long ldw,
                                float* grad_dev, void* stream) {
    const char* who = "cmps_bank_loss_bwd_weighted";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = Args{h, who}.ptr("weight_dev", weight_dev).ld("ldw", ldw, B).rc) return rc;
    if (const int rc = bank_check_mode(h, who, true)) return rc;
    if (const int rc = need_mode(h, who, ~in(MODE_RHO_BANK), true,
                                 ": the handle holds a RhoCMPS bank; the weighted reverse pass is for PsiCMPS banks (cmps_bank_set_params_dev)")) return rc;
    if (const int rc = check_bwd(h, who, in(MODE_PSI_BANK), h->main.M == h->bank_M, "cmps_bank_loss_fwd", h->main, audio_dev, grad_dev, B, T)) return rc;
    if (n_audio != h->main.n_audio) return fail(h, CMPS_ERR_STATE, std::string(who) + ": n_audio differs from the forward call");
    return psi_bwd_run(h, who, h->bank_M, n_audio, audio_dev, B, T, grad_dev, stream, weight_dev, ldw);
}

size_t cmps_bank_apply_step_scratch_bytes(int D, int M) {
    return (M < 1 || M > BANK_MAX) ? 0 : (size_t)M * cmps_apply_step_scratch_bytes(D);
}

int cmps_bank_apply_step(cmps_handle_t h, int M, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev,
                         double global_batch, double bias_num, double bias_den, double beta1, double beta2, double epsilon,
                         const double* hyper_dev, int with_reg, float* params_dev, float* losses_dev, void* scratch_dev, void* stream) {
    const char* who = "cmps_bank_apply_step";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!vars_dev || !params_dev || !hyper_dev) return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": null variable / parameter / hyper-parameter buffer");
    if (const int rc = bank_check_M(h, who, M)) return rc;
    if (const int rc = check_apply_step(h, who, grad_sums_dev, adam_m_dev, adam_v_dev, losses_dev, scratch_dev, global_batch, hyper_dev)) return rc;
    const bool apply = grad_sums_dev != nullptr;
    const hipError_t e = launch_bank_apply_step(h->D, M, apply, apply ? 1.0 / global_batch : 0.0, bias_num, bias_den, beta1, beta2, epsilon,
                                                hyper_dev, with_reg != 0, vars_dev, adam_m_dev, adam_v_dev, grad_sums_dev, params_dev,
                                                losses_dev, static_cast<double*>(scratch_dev), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_bank_apply_step");
    return CMPS_OK;
}

int cmps_bank_grad_status(cmps_handle_t h, int* codes_out, int* sticky_out, void* stream) {
    const char* who = "cmps_bank_grad_status";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!codes_out) return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": null codes_out");
    if (const int rc = need_mode(h, who, in(MODE_PSI_BANK), h->P.status != nullptr, ": needs cmps_bank_set_params_dev with a CMPS_WS_TRAIN workspace"))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = h->bank_M;
    std::vector<unsigned> words(2 * (size_t)M, 0u);
    // the members' pairs of words lie one workspace apart: one strided copy, then the sticky words restart with one strided fill
    hipError_t e = hipMemcpy2DAsync(words.data(), 2 * sizeof(unsigned), h->P.status, h->P.bank_stride, 2 * sizeof(unsigned), (size_t)M,
                                    hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemset2DAsync(h->P.status + 1, h->P.bank_stride, 0, sizeof(unsigned), (size_t)M, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail_hip(h, e, "cmps_bank_grad_status");
    for (int m = 0; m < M; ++m) {
        const unsigned now = words[2 * m];
        codes_out[m] = ((now & 1u) && !(now & 2u)) ? CMPS_ERR_F16_RANGE : CMPS_OK;
        if (sticky_out) sticky_out[m] = (int)words[2 * m + 1];
    }
    return CMPS_OK;
}

int cmps_psi_update_ancilla(cmps_handle_t h, const float* psi_in_dev, const float* signal_dev, float t,
                            int B, float* psi_out_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_plain(h, "cmps_psi_update_ancilla", in(MODE_PSI) | in(MODE_LEGACY), true, ": call cmps_set_params first")) return rc;
    if (!psi_in_dev || !signal_dev || !psi_out_dev || B < 1)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_psi_update_ancilla: bad argument");
    hipError_t e = launch_update_ancilla(h->P, psi_in_dev, signal_dev, t, B, psi_out_dev,
                                         static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_psi_update_ancilla");
    return CMPS_OK;
}

int cmps_psi_states(cmps_handle_t h, int B, int T, float* psi_out_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_not_bank(h, "cmps_psi_states")) return rc;
    // (k_states rotates into the lab frame with freqs and the time table; neither exists after cmps_legacy_set_params)
    if (const int rc = need_mode(h, "cmps_psi_states", ~in(MODE_LEGACY), true, ": not available in legacy mode (no time table for the lab-frame phases)"))
        return rc;
    if (const int rc = need_mode(h, "cmps_psi_states", in(MODE_PSI), h->main.valid && h->main.M == 0, ": needs cmps_psi_loss_fwd(save_for_bwd=1) first"))
        return rc;
    if (!psi_out_dev || B != h->main.B || T != h->main.steps + 1)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_psi_states: bad argument");
    hipError_t e = launch_states(main_dev(h, B), B, psi_out_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_psi_states");
    return CMPS_OK;
}

// What cmps_psi_sample, cmps_psi_sample_primed and cmps_psi_stream share behind their own argument checks (the two checks also with
// their RhoCMPS counterparts).
// One row of the per-step tables per step, forced or sampled: the rows below `end` must exist (`what` names end + 1 in the caller's terms)
static int sample_check_rows(cmps_handle_t h, const char* who, const char* what, long long end) {
    if (end <= h->L.N) return CMPS_OK;
    char buf[240];
    snprintf(buf, sizeof buf, "%s: %s = %lld exceeds T = %d of cmps_set_params (the per-step tables): needs T >= %lld", who, what, end + 1,
             h->L.T, end + 1);
    return fail(h, CMPS_ERR_BAD_ARG, buf);
}
// a clip per path, or one clip shared by every path
static int sample_check_clips(cmps_handle_t h, const char* who, const char* name, int n_clips, int n) {
    if (n_clips == 1 || n_clips == n) return CMPS_OK;
    return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": " + name + " must be n, or 1 for one clip shared by every path");
}
// floats of one stream-state record of the handle's sampler family
static int stream_rec_floats(const cmps_handle_s* h) {
    const int family = sampler_family(h);
    return family == SAMPLER_WAVE ? STREAM_REC_WAVE : family == SAMPLER_WIDE ? stream_rec_wide(padded_D(h->D)) : stream_rec_block(h->D);
}
// What cmps_{psi,rho}_sample_primed check behind their state check, and the launch record of the call
static int primed_args(cmps_handle_t h, const char* who, const float* prime_dev, int n_prime, int prime_T, const float* noise_dev, int n, int length,
                       float* out_dev, float* pred_dev, SampleDev& S) {
    const std::string w(who);
    if (!prime_dev || !noise_dev || !out_dev) return fail(h, CMPS_ERR_BAD_ARG, w + ": null pointer");
    if (n < 1 || length < 1) return fail(h, CMPS_ERR_BAD_ARG, w + ": need n >= 1 and length >= 1");
    if (prime_T < 2) return fail(h, CMPS_ERR_BAD_ARG, w + ": need prime_T >= 2 (one increment at least)");
    if (int c = sample_check_clips(h, who, "n_prime", n_prime, n)) return c;
    const int PF = prime_T - 1;                                  // teacher-forced steps
    if (int c = sample_check_rows(h, who, "prime_T + length", (long long)PF + length)) return c;
    S = SampleDev{noise_dev, n, length, out_dev, PrimeDev{prime_dev, n_prime == 1 ? 0 : prime_T, PF, pred_dev}, nullptr, nullptr};
    return CMPS_OK;
}
// The launch record of one stream segment: S points to ST and, when the segment is scored, to SC (so a StreamCall is filled where it stands)
struct StreamCall {
    StreamDev ST{};
    ScoreDev SC{};
    SampleDev S{};
};
// A stream entry's rule for the row counts of its arrays: the signal's n_audio and the noise's n_noise (n where the segment samples
// nothing), for n paths and `steps` steps.  plain_rows is a plain handle's, bank_rows a bank's
using RowRule = int (*)(cmps_handle_t h, const char* who, int n_audio, int n_noise, int n, long long steps);
static int plain_rows(cmps_handle_t h, const char* who, int n_audio, int, int n, long long) { return sample_check_clips(h, who, "n_audio", n_audio, n); }
static int stream_check_state(cmps_handle_t h, const char* who, const void* state_in_dev, int k0) {
    if ((state_in_dev == nullptr) == (k0 == 0)) return CMPS_OK;
    return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": state_in_dev is NULL exactly at the start of a stream (k0 == 0)");
}
// What cmps_{psi,rho,bank}_stream check behind their state check, and the launch record of the call (`rec`: floats of one state record).
// The caller brings what a bank changes: the rule for the row counts, with the noise's rows, and the member strides.
static int stream_args(cmps_handle_t h, const char* who, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio,
                       int forced, const float* noise_dev, int n_noise, int length, int n, float* out_dev, float* pred_dev, int rec, RowRule rows,
                       const MemberDev& MB, StreamCall& C) {
    const std::string w(who);
    if (n < 1 || forced < 0 || length < 0 || (long long)forced + length < 1 || k0 < 0)
        return fail(h, CMPS_ERR_BAD_ARG, w + ": need n >= 1, forced >= 0, length >= 0, forced + length >= 1 and k0 >= 0");
    if (int c = stream_check_state(h, who, state_in_dev, k0)) return c;
    if (forced > 0 && !audio_dev) return fail(h, CMPS_ERR_BAD_ARG, w + ": forced > 0 needs audio_dev");
    if (length > 0 && (!noise_dev || !out_dev)) return fail(h, CMPS_ERR_BAD_ARG, w + ": length > 0 needs noise_dev and out_dev");
    if (int c = rows(h, who, n_audio, length > 0 ? n_noise : n, n, (long long)forced + length)) return c;
    if (int c = sample_check_rows(h, who, "k0 + forced + length + 1", (long long)k0 + forced + length)) return c;
    C.ST = StreamDev{static_cast<const float*>(state_in_dev), static_cast<float*>(state_out_dev), k0, rec};
    C.S = SampleDev{noise_dev, n, length, out_dev, PrimeDev{audio_dev, n_audio == 1 ? 0 : forced + 1, forced, pred_dev}, &C.ST, nullptr, MB};
    return CMPS_OK;
}
// The same for the three *_stream_score entries, whose every step is forced: `per` ends the sentence on what loss_dev holds one value for
static int score_args(cmps_handle_t h, const char* who, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio,
                      int forced, int n, float* nll_dev, float* loss_dev, float* pred_dev, int rec, const char* per, RowRule rows,
                      const MemberDev& MB, StreamCall& C) {
    const std::string w(who);
    if (n < 1 || forced < 1 || k0 < 0) return fail(h, CMPS_ERR_BAD_ARG, w + ": need n >= 1, forced >= 1 and k0 >= 0");
    if (int c = stream_check_state(h, who, state_in_dev, k0)) return c;
    if (!audio_dev) return fail(h, CMPS_ERR_BAD_ARG, w + ": needs audio_dev");
    if (!loss_dev) return fail(h, CMPS_ERR_BAD_ARG, w + ": needs loss_dev (the running loss per " + per + ")");
    if (int c = rows(h, who, n_audio, n, n, forced)) return c;
    if (int c = sample_check_rows(h, who, "k0 + forced + 1", (long long)k0 + forced)) return c;
    C.ST = StreamDev{static_cast<const float*>(state_in_dev), static_cast<float*>(state_out_dev), k0, rec};
    C.SC = ScoreDev{nll_dev, loss_dev};
    C.S = SampleDev{nullptr, n, 0, nullptr, PrimeDev{audio_dev, n_audio == 1 ? 0 : forced + 1, forced, pred_dev}, &C.ST, &C.SC, MB};
    return CMPS_OK;
}
// The kernel choice and the launch of one SampleDev
static int psi_sample_launch(cmps_handle_t h, const char* who, const SampleDev& S, void* stream) {
    const int family = sampler_family(h);
    static const char* const names[3][4] = {{"k_sample_block", "k_sample_block_primed", "k_sample_block_stream", "k_sample_block_score"},
                                            {"k_sample_wave", "k_sample_wave_primed", "k_sample_wave_stream", "k_sample_wave_score"},
                                            {"k_sample_wide", "k_sample_wide_primed", "k_sample_wide_stream", "k_sample_wide_score"}};   // [family][SampleMode]
    return run_kernel(h, who, names[family][sample_mode(S)], stream, [&](hipStream_t s) {
        return family == SAMPLER_WAVE ? launch_sample_wave(h->P, S, s)
             : family == SAMPLER_WIDE ? launch_sample_wide(h->P, S, s) : launch_sample_block(h->P, S, s);
    });
}

int cmps_psi_sample(cmps_handle_t h, const float* noise_dev, int n, int length, float* out_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_plain(h, "cmps_psi_sample", in(MODE_PSI) | in(MODE_LEGACY), true, ": call cmps_set_params first")) return rc;
    if (!noise_dev || !out_dev || n < 1 || length < 1)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_psi_sample: bad argument");
    if (length > h->L.N)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_psi_sample: length exceeds T - 1 of cmps_set_params (the per-step tables)");
    return psi_sample_launch(h, "cmps_psi_sample", SampleDev{noise_dev, n, length, out_dev, PrimeDev{}, nullptr, nullptr}, stream);
}

int cmps_psi_sample_primed(cmps_handle_t h, const float* prime_dev, int n_prime, int prime_T, const float* noise_dev, int n, int length,
                           float* out_dev, float* pred_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    // (the legacy tables carry no rotation and another step: nothing here would mean PsiCMPS.sample)
    if (const int rc = need_plain(h, "cmps_psi_sample_primed", in(MODE_PSI), true, ": call cmps_set_params first (not available in legacy mode)")) return rc;
    SampleDev S;
    if (int c = primed_args(h, "cmps_psi_sample_primed", prime_dev, n_prime, prime_T, noise_dev, n, length, out_dev, pred_dev, S)) return c;
    return psi_sample_launch(h, "cmps_psi_sample_primed", S, stream);
}

size_t cmps_psi_stream_state_bytes(cmps_handle_t h, int n) {
    if (!h || n < 1) return 0;
    return (size_t)n * stream_rec_floats(h) * sizeof(float);
}

int cmps_psi_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, int forced,
                    const float* noise_dev, int length, int n, float* out_dev, float* pred_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_plain(h, "cmps_psi_stream", in(MODE_PSI), true, ": call cmps_set_params first (not available in legacy mode)")) return rc;
    StreamCall C;
    if (int c = stream_args(h, "cmps_psi_stream", state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, noise_dev, n, length, n, out_dev, pred_dev,
                            stream_rec_floats(h), plain_rows, MemberDev{}, C))
        return c;
    return psi_sample_launch(h, "cmps_psi_stream", C.S, stream);
}

int cmps_psi_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, int forced,
                          int n, float* nll_dev, float* loss_dev, float* pred_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_plain(h, "cmps_psi_stream_score", in(MODE_PSI), true, ": call cmps_set_params first (not available in legacy mode)")) return rc;
    StreamCall C;
    if (int c = score_args(h, "cmps_psi_stream_score", state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, n, nll_dev, loss_dev, pred_dev,
                           stream_rec_floats(h), "path", plain_rows, MemberDev{}, C))
        return c;
    return psi_sample_launch(h, "cmps_psi_stream_score", C.S, stream);
}

// ---- a bank's streams: the STREAM / SCORE instances with the members as a second grid dimension (include/cmps.h) ----
// What cmps_bank_stream and cmps_bank_stream_score refuse before they look at their arguments
static int bank_stream_check_mode(cmps_handle_t h, const char* who) {
    if (const int rc = need_mode(h, who, in(MODE_PSI_BANK), true, ": needs a PsiCMPS bank (call cmps_bank_set_params_dev first)")) return rc;
    if (const int rc = bank_check_mode(h, who, true)) return rc;
    if (sampler_family(h) == SAMPLER_WIDE)               // (a variant set behind cmps_bank_set_params_dev)
        return fail(h, CMPS_ERR_STATE, std::string(who) + ": a bank samples with the wave and block kernels only");
    return CMPS_OK;
}
// The RowRule of a bank's streams: arrays the members may share, then M n `steps` (= forced + length): every index into the caller's
// arrays fits 31 bits (n >= 1 and steps >= 1 are checked before)
static int bank_rows(cmps_handle_t h, const char* who, int n_audio, int n_noise, int n, long long steps) {
    const std::string w(who);
    const long long Mn = (long long)h->bank_M * n;
    if (n_audio != 1 && n_audio != n && n_audio != Mn)
        return fail(h, CMPS_ERR_BAD_ARG, w + ": n_audio must be 1 (one signal for every path of every member), n (shared by the members) or M * n");
    if (n_noise != n && n_noise != Mn) return fail(h, CMPS_ERR_BAD_ARG, w + ": n_noise must be n (every member hears the same noise) or M * n");
    if ((unsigned long long)Mn * (unsigned long long)steps > 0x7fffffffull) return fail(h, CMPS_ERR_BAD_ARG, w + ": M * n * (forced + length) exceeds 2^31 - 1");
    return CMPS_OK;
}
// floats between two members' rows of an array with `rows` rows of `row` floats (1 or n rows: shared, 0)
static size_t bank_member_stride(const cmps_handle_s* h, long long rows, int n, size_t row) {
    return (h->bank_M > 1 && rows == (long long)h->bank_M * n) ? (size_t)n * row : 0;
}

size_t cmps_bank_stream_state_bytes(cmps_handle_t h, int n) {
    if (!h || n < 1 || h->mode != MODE_PSI_BANK) return 0;
    return (size_t)h->bank_M * (size_t)n * stream_rec_floats(h) * sizeof(float);
}

int cmps_bank_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, int forced,
                     const float* noise_dev, int n_noise, int length, int n, float* out_dev, float* pred_dev, void* stream) {
    const char* who = "cmps_bank_stream";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = bank_stream_check_mode(h, who)) return rc;
    const MemberDev MB{h->bank_M, audio_dev ? bank_member_stride(h, n_audio, n, (size_t)forced + 1) : 0,
                       length > 0 ? bank_member_stride(h, n_noise, n, (size_t)length) : 0};
    StreamCall C;
    if (int c = stream_args(h, who, state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, noise_dev, n_noise, length, n, out_dev, pred_dev,
                            stream_rec_floats(h), bank_rows, MB, C))
        return c;
    return psi_sample_launch(h, who, C.S, stream);
}

int cmps_bank_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, int forced,
                           int n, float* nll_dev, float* loss_dev, float* pred_dev, void* stream) {
    const char* who = "cmps_bank_stream_score";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = bank_stream_check_mode(h, who)) return rc;
    StreamCall C;
    if (int c = score_args(h, who, state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, n, nll_dev, loss_dev, pred_dev, stream_rec_floats(h),
                           "member and path", bank_rows,
                           MemberDev{h->bank_M, bank_member_stride(h, n_audio, n, (size_t)forced + 1), 0}, C))
        return c;
    return psi_sample_launch(h, who, C.S, stream);
}

// The samplers' noise drawn on the device: needs nothing of the handle but its error string and its kernel-event record
int cmps_noise_fill(cmps_handle_t h, unsigned long long seed, unsigned long long first_step, unsigned first_path, int n, int length,
                    float stddev, float* noise_dev, void* stream) {
    const char* who = "cmps_noise_fill";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = Args{h, who}.ptr("noise_dev", noise_dev).need(n >= 1 && length >= 1, "need n >= 1 and length >= 1")
                           .not_negative("stddev", stddev)
                           .need((unsigned long long)first_path + (unsigned long long)n <= (1ull << 32),
                                 "first_path + n exceeds 2^32 (a path is a 32-bit counter word)")
                           .need(first_step + (unsigned long long)length >= first_step, "first_step + length overflows 64 bits").rc) return rc;
    return run_kernel(h, who, "k_noise_philox", stream,
                      [&](hipStream_t s) { return launch_noise_philox(seed, first_step, first_path, n, length, stddev, noise_dev, s); });
}

// The input of a training step produced on the device: like cmps_noise_fill, both need nothing of the handle but its error string and
// its kernel-event record
static Args gather_args(cmps_handle_t h, const char* who, const void* data_dev, long long n_clips, long long clip_len, const int* index_dev, int B, int T,
                        const float* audio_dev) {
    return Args{h, who}.ptr("data_dev", data_dev).ptr("index_dev", index_dev).ptr("audio_dev", audio_dev)
        .need(B >= 1 && T >= 1, "need B >= 1 and T >= 1")
        .need(n_clips >= 1 && n_clips <= 2147483647ll, "need 1 <= n_clips <= 2^31 - 1 (an index is a 32-bit int)")
        .need(clip_len >= (long long)T, "clip_len must be at least T");
}

int cmps_batch_gather(cmps_handle_t h, const float* data_dev, long long n_clips, long long clip_len, const int* index_dev,
                      const int* offset_dev, int B, int T, float* audio_dev, void* stream) {
    const char* who = "cmps_batch_gather";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = gather_args(h, who, data_dev, n_clips, clip_len, index_dev, B, T, audio_dev).rc) return rc;
    return run_kernel(h, who, "k_batch_gather", stream,
                      [&](hipStream_t s) { return launch_batch_gather(data_dev, n_clips, clip_len, index_dev, offset_dev, B, T, audio_dev, s); });
}

int cmps_batch_gather_i16(cmps_handle_t h, const short* data_dev, long long n_clips, long long clip_len, const int* index_dev,
                          const int* offset_dev, int B, int T, float scale, float* audio_dev, void* stream) {
    const char* who = "cmps_batch_gather_i16";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = gather_args(h, who, data_dev, n_clips, clip_len, index_dev, B, T, audio_dev).positive("scale", scale).rc) return rc;
    return run_kernel(h, who, "k_batch_gather_i16", stream, [&](hipStream_t s) {
        return launch_batch_gather_i16(data_dev, n_clips, clip_len, index_dev, offset_dev, B, T, scale, audio_dev, s);
    });
}

// The per-clip losses of an evaluation pass folded into one record on the device: needs nothing of the handle either
int cmps_loss_stats(cmps_handle_t h, const float* loss_dev, int B, long long first_id, int reset, void* stats_dev, void* stream) {
    const char* who = "cmps_loss_stats";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = Args{h, who}.ptr("loss_dev", loss_dev).ptr("stats_dev", stats_dev).align8("stats_dev", stats_dev).min1("B", B)
                           .range63("first_id", first_id, "B", B, "an id").rc) return rc;
    return run_kernel(h, who, "k_loss_stats", stream, [&](hipStream_t s) { return launch_loss_stats(loss_dev, B, first_id, reset, stats_dev, s); });
}

// The [M][B] losses of a bank forward judged as a classifier, folded into one record on the device: needs nothing of the handle either
size_t cmps_bank_classify_stats_bytes(int M) {
    if (M < 1 || M > CLASSIFY_MAX_M) return 0;
    return CLASSIFY_HEAD_BYTES + sizeof(long long) * ((size_t)M * (size_t)M + (size_t)M);
}

int cmps_bank_classify_stats(cmps_handle_t h, const float* loss_dev, int M, int B, long long ld, const int* label_dev, long long first_id,
                             int reset, void* stats_dev, int* best_dev, void* stream) {
    const char* who = "cmps_bank_classify_stats";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = Args{h, who}.ptr("loss_dev", loss_dev).ptr("stats_dev", stats_dev).align8("stats_dev", stats_dev).members(M).min1("B", B)
                           .ld("ld", ld, B).range63("first_id", first_id, "B", B, "an id").rc) return rc;
    return run_kernel(h, who, "k_classify_stats", stream, [&](hipStream_t s) {
        return launch_classify_stats(loss_dev, M, B, ld, label_dev, first_id, reset, stats_dev, best_dev, s);
    });
}

// ... and turned into the cotangents of a cross-entropy step: needs nothing of the handle either
int cmps_bank_classify_weights(cmps_handle_t h, const float* loss_dev, int M, int B, long long ld, const int* label_dev, double inv_temp,
                               double gen_weight, double disc_weight, int reset, float* weight_dev, long long ldw, void* record_dev,
                               void* stream) {
    const char* who = "cmps_bank_classify_weights";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = Args{h, who}.ptr("loss_dev", loss_dev).ptr("label_dev", label_dev).ptr("weight_dev", weight_dev).ptr("record_dev", record_dev)
                           .align8("record_dev", record_dev).members(M).min1("B", B).ld("ld", ld, B).ld("ldw", ldw, B)
                           .positive("inv_temp", inv_temp).not_negative("gen_weight", gen_weight).not_negative("disc_weight", disc_weight).rc)
        return rc;
    return run_kernel(h, who, "k_classify_weights", stream, [&](hipStream_t s) {
        return launch_classify_weights(loss_dev, M, B, ld, label_dev, inv_temp, gen_weight, disc_weight, reset, weight_dev, ldw, record_dev, s);
    });
}

// The per-step losses of a scored bank stream folded into the posterior over the members after every step: needs nothing of the handle either
int cmps_bank_posterior(cmps_handle_t h, const float* nll_dev, int M, int n, int steps, const float* total_in_dev, const double* log_prior_dev,
                        double inv_temp, float* total_out_dev, float* post_dev, int* best_dev, float* conf_dev, double threshold,
                        long long first_step, int reset, void* decision_dev, void* stream) {
    const char* who = "cmps_bank_posterior";
    if (!h) return CMPS_ERR_BAD_ARG;
    Args a{h, who};
    a.ptr("nll_dev", nll_dev).members(M).min1("n", n).min1("steps", steps);
    a.need(a.rc || (long long)M * (long long)n <= 2147483647ll / (long long)steps, "need M * n * steps <= 2^31 - 1")
        .positive("inv_temp", inv_temp).align8("log_prior_dev", log_prior_dev).align8("decision_dev", decision_dev);
    if (decision_dev)
        a.need(std::isfinite(threshold) && threshold > 0.0 && threshold <= 1.0, "threshold must lie in (0, 1] where decision_dev is given")
            .range63("first_step", first_step, "steps", steps, "a step");
    if (a.rc) return a.rc;
    return run_kernel(h, who, "k_bank_posterior", stream, [&](hipStream_t s) {
        return launch_bank_posterior(nll_dev, M, n, steps, total_in_dev, log_prior_dev, inv_temp, total_out_dev, post_dev, best_dev, conf_dev,
                                     threshold, first_step, reset, decision_dev, s);
    });
}

// The [M][N] losses of a held-out set fitted for the temperature and the prior: needs nothing of the handle either.  max_iter + 1 pairs of
// launches go out without a look at the device; the pairs behind the one that finishes leave at their first branch
size_t cmps_bank_calibrate_scratch_bytes(int M, long long N) {
    if (M < 1 || M > CLASSIFY_MAX_M || N < 1 || N > (1ll << 62) / (long long)M) return 0;
    return calib_scratch_bytes(M, N);
}

int cmps_bank_calibrate(cmps_handle_t h, const float* loss_dev, int M, long long N, long long ld, const int* label_dev, int fit, int max_iter,
                        double tol, double kappa_min, double kappa_max, double* theta_dev, void* record_dev, void* scratch_dev,
                        size_t scratch_bytes, void* stream) {
    const char* who = "cmps_bank_calibrate";
    if (!h) return CMPS_ERR_BAD_ARG;
    Args a{h, who};
    a.ptr("loss_dev", loss_dev).ptr("label_dev", label_dev).ptr("theta_dev", theta_dev).align8("theta_dev", theta_dev)
        .ptr("record_dev", record_dev).align8("record_dev", record_dev).ptr("scratch_dev", scratch_dev).align8("scratch_dev", scratch_dev)
        .members(M);
    a.need(a.rc || (N >= 1 && ld <= (1ll << 62) / (long long)M), "need N >= 1 and M * ld <= 2^62")
        .need(ld >= N, "ld must be at least N")
        .need(fit >= 0 && fit <= 3, "fit is a set of CMPS_CALIB_TEMPERATURE | CMPS_CALIB_PRIOR: 0 .. 3")
        .need(max_iter >= 0 && max_iter <= 10000, "need 0 <= max_iter <= 10000")
        .positive("tol", tol).positive("kappa_min", kappa_min)
        .need(std::isfinite(kappa_max) && kappa_max >= kappa_min, "kappa_max must be finite and at least kappa_min");
    a.need(a.rc || scratch_bytes >= calib_scratch_bytes(M, N), "scratch_bytes is below cmps_bank_calibrate_scratch_bytes(M, N)");
    if (a.rc) return a.rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    KBind kb(h);
    for (int i = 0; i <= max_iter; ++i) {
        hipError_t e;
        {
            KScope ks("k_calib_pass", s);
            e = launch_calib_pass(loss_dev, M, N, ld, label_dev, theta_dev, scratch_dev, i == 0, s);
        }
        if (e == hipSuccess) {
            KScope ks("k_calib_update", s);
            e = launch_calib_update(theta_dev, record_dev, scratch_dev, M, N, fit, max_iter, tol, kappa_min, kappa_max, i == 0, s);
        }
        if (e != hipSuccess) return fail_hip(h, e, who);
    }
    return CMPS_OK;
}

int cmps_damped_sine_fill(cmps_handle_t h, unsigned long long seed, unsigned long long first_clip, int B, int T, double delta_t,
                          float* audio_dev, void* stream) {
    const char* who = "cmps_damped_sine_fill";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = Args{h, who}.ptr("audio_dev", audio_dev)
                           .need(B >= 1 && T >= 1 && T <= (1 << 24), "need B >= 1 and 1 <= T <= 2^24 (beyond that a sample index is not exact in float32)")
                           .positive("delta_t", delta_t)
                           .need(first_clip + (unsigned long long)B >= first_clip, "first_clip + B overflows 64 bits").rc) return rc;
    return run_kernel(h, who, "k_damped_sine", stream, [&](hipStream_t s) { return launch_damped_sine(seed, first_clip, B, T, delta_t, audio_dev, s); });
}

// ---------------------------------------------------------------------------------------------------
// legacy AudioMPS arithmetic
// ---------------------------------------------------------------------------------------------------
int cmps_legacy_set_params(cmps_handle_t h, const float* R_dev, const float* Q_re_dev, const float* Q_im_dev,
                           double delta_t, int T, int B_max, int flags, void* workspace_dev, size_t workspace_bytes,
                           void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!R_dev || !Q_re_dev || !Q_im_dev) return fail(h, CMPS_ERR_BAD_ARG, "cmps_legacy_set_params: null parameter pointer");
    if (T < 2 || B_max < 1) return fail(h, CMPS_ERR_BAD_ARG, "cmps_legacy_set_params: need T >= 2 and B_max >= 1");
    if (!workspace_dev) return fail(h, CMPS_ERR_WORKSPACE, "cmps_legacy_set_params: null workspace");
    Layout L = make_layout(h->D, B_max, T, flags);
    if (workspace_bytes < L.total) return fail(h, CMPS_ERR_WORKSPACE, "cmps_legacy_set_params: workspace too small");
    if (((uintptr_t)workspace_dev & 255) != 0)
        return fail(h, CMPS_ERR_WORKSPACE, "cmps_legacy_set_params: workspace must be 256-byte aligned");
    char* ws = static_cast<char*>(workspace_dev);
    // psi0 / dtk / rho: the tables of the pure-state wave kernels, which the D <= 32 legacy kernels share (cmps_wave2.hip /
    // cmps_wave.hip, LEGACY): rotation rho = 1, psi_0 = e_0, no time table
    Dev P = bind_workspace(L, ws);
    P.dt = (float)delta_t;
    P.A = 1.0f;
    hipError_t e = launch_pack_legacy(P, R_dev, Q_re_dev, Q_im_dev, const_cast<float2*>(P.R), const_cast<float2*>(P.RT),
                                      const_cast<float2*>(P.Q), const_cast<float2*>(P.QT), static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = launch_legacy_tables(P, const_cast<float2*>(P.psi0), const_cast<float*>(P.dtk), const_cast<float2*>(P.rho),
                                                  static_cast<hipStream_t>(stream));
    if (e != hipSuccess) { unconfigure(h); return fail_hip(h, e, "cmps_legacy_set_params"); }
    h->L = L; h->P = P; h->ws = ws;
    h->tt_ws = nullptr;               // the time table of the PsiCMPS mode is no longer valid for this workspace
    h->mode = MODE_LEGACY;
    h->bank_M = 0;
    h->main.valid = false;
    h->rho_set = false;
    return CMPS_OK;
}

int cmps_legacy_loss_fwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* loss_dev, int save_for_bwd,
                         void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_fwd(h, "cmps_legacy_loss_fwd", in(MODE_LEGACY), true, "cmps_legacy_set_params", audio_dev, loss_dev, B, T, h->L.T, h->L.B,
                                 save_for_bwd, h->L.flags)) return rc;
    Dev P = h->P;
    P.B = B;
    // D <= 32: the pure-state wave kernels in LEGACY mode (cmps_wave2.hip, cmps_wave.hip); above: the wide kernels in LEGACY mode
    // (cmps_wide.hip; round 5); CMPS_VARIANT_BLOCK: the general one-workgroup-per-clip kernels (cmps_legacy.hip), the cross-check
    const bool wave = h->D <= 32 && h->variant_req != CMPS_VARIANT_BLOCK;
    const bool wide = h->D > 32 && h->variant_req != CMPS_VARIANT_BLOCK;
    const bool f16 = rank1_f16(h->rank1_mode);
    KBind kb(h);
    hipError_t e = wave ? launch_fwd_legacy_wave(P, audio_dev, loss_dev, save_for_bwd != 0, static_cast<hipStream_t>(stream))
                 : wide ? launch_fwd_wide_legacy(P, audio_dev, loss_dev, save_for_bwd != 0, f16, static_cast<hipStream_t>(stream))
                        : launch_fwd_legacy(P, audio_dev, loss_dev, save_for_bwd != 0, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_legacy_loss_fwd");
    // the rows as the forward wrote them: the wave kernel's (y, H y) pairs, the wide kernels' rows, or k_fwd_legacy's [B][N][DP] float2
    h->main = Saved{save_for_bwd != 0, B, T - 1, audio_dev, loss_dev, wave ? STASH_WAVE32 : wide ? STASH_WIDE : STASH_BLOCK};
    return CMPS_OK;
}

int cmps_legacy_loss_bwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* grad_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_bwd(h, "cmps_legacy_loss_bwd", in(MODE_LEGACY), true, "cmps_legacy_loss_fwd", h->main, audio_dev, grad_dev, B, T))
        return rc;
    Dev P = main_dev(h, B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    KBind kb(h);
    hipError_t e;
    Dev Pr = P;                                                    // what the slab reduction runs over
    if (h->main.layout == STASH_WIDE) {
        // reverse chain, then the gradient GEMM over the rows both scans left behind; one slab per PAIR of clips
        { KScope ks("k_bwd_wide<legacy>", s); e = launch_bwd_wide_legacy(P, audio_dev, s); }
        if (e == hipSuccess) {
            KScope ks("k_grad_gemm<legacy>", s);
            e = launch_grad_wide_legacy(P, audio_dev, rank1_f16(h->rank1_mode), s);
        }
        Pr.B = (B + 1) / 2;
    } else {
        e = h->main.layout == STASH_WAVE32 ? launch_bwd_legacy_wave(P, audio_dev, wave_rank1(h->rank1_mode), s) : launch_bwd_legacy(P, audio_dev, s);
    }
    if (e != hipSuccess) return fail_hip(h, e, "cmps_legacy_loss_bwd (scan)");
    e = launch_reduce_only(Pr, s);
    if (e == hipSuccess) e = launch_finalize_legacy(P, h->main.loss, grad_dev, s);
    if (e != hipSuccess) return fail_hip(h, e, "cmps_legacy_loss_bwd (reduce)");
    return CMPS_OK;
}

// ---------------------------------------------------------------------------------------------------
// RhoCMPS (model.py:55-203)
// ---------------------------------------------------------------------------------------------------
size_t cmps_rho_workspace_bytes(int D, int rank, int B, int T, int flags) {
    if (D < 1 || D > 128 || rank < 1 || B < 1 || T < 2) return 0;
    return make_rho_layout(D, rank, B, T, flags).total;
}

int cmps_rho_set_state(cmps_handle_t h, const float* phi_re_dev, const float* phi_im_dev, int rank, int T, int B_max,
                       int flags, void* rho_workspace_dev, size_t rho_workspace_bytes, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_plain(h, "cmps_rho_set_state", in(MODE_PSI), true, ": call cmps_set_params first")) return rc;
    if (!phi_re_dev || !phi_im_dev || rank < 1 || B_max < 1 || T < 2)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_set_state: bad argument");
    if (T > h->L.T) return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_set_state: T exceeds T of cmps_set_params (the per-step tables)");
    if (rank > 128) return fail(h, CMPS_ERR_UNSUPPORTED_D, "cmps_rho_set_state: rank above 128");
    if (!rho_workspace_dev) return fail(h, CMPS_ERR_WORKSPACE, "cmps_rho_set_state: null workspace");
    if (((uintptr_t)rho_workspace_dev & 255) != 0)
        return fail(h, CMPS_ERR_WORKSPACE, "cmps_rho_set_state: workspace must be 256-byte aligned");
    RhoLayout RL = make_rho_layout(h->D, rank, B_max, T, flags);
    if (rho_workspace_bytes < RL.total) {
        char buf[160];
        snprintf(buf, sizeof buf, "cmps_rho_set_state: workspace has %zu bytes, needs %zu", rho_workspace_bytes, RL.total);
        return fail(h, CMPS_ERR_WORKSPACE, buf);
    }
    char* ws = static_cast<char*>(rho_workspace_dev);
    const RhoDev W = bind_rho_workspace(h->D, RL, ws, flags, B_max);
    hipError_t e = launch_pack_phi(h->P, W, phi_re_dev, phi_im_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_rho_set_state");
    h->RL = RL; h->W = W;
    h->rho_B = B_max; h->rho_T = T; h->rho_flags = flags;
    h->rho_set = true;
    h->rho.valid = h->rho.bwd_ok = false;
    return CMPS_OK;
}

// cmps_rho_loss_fwd (M = 0) and cmps_rho_bank_loss_fwd (M members, n_audio batches) behind their argument checks.  A bank comes here under
// the conditions of rho_bank_check_mode only, where the choice below is the wave family with the virtual-clip reverse sweep, never wide.
static int rho_fwd_run(cmps_handle_t h, const char* who, int M, int n_audio, const float* audio_dev, int B, int T, float* loss_dev, int save_for_bwd,
                       void* stream) {
    Dev P = h->P;
    P.B = B; P.T = T; P.N = T - 1;                               // (a bank's rho workspace has the T of its tables: the values h->P holds)
    const int Mk = M > 0 ? M : 1;
    if (M > 0) bank_strides(P, n_audio, B, T);
    // D <= 32 (and rank <= 32): one wavefront per clip, unless the block variant was asked for -- the forward as row-array
    // GEMMs on the matrix cores (cmps_rho_mfma.hip); CMPS_VARIANT_WAVE32 keeps the column-by-column kernel (cross-check)
    const bool wave = h->D <= 32 && h->W.rank <= 32 && h->variant_req != CMPS_VARIANT_BLOCK;
    // the row-array GEMM forward costs the same at every rank; with the virtual-clip reverse sweep behind it (3.75 + 0.11 rank ms at T = 1000,
    // B = 256 against 1.65 rank ms for the column kernels: scripts/bench_next_rows.py) it wins from rank 3, with k_bwd_rho_mfma from rank 9
    const bool mfma = wave && h->variant_req != CMPS_VARIANT_WAVE32 && h->W.rank > (h->rho_virtual_bwd && save_for_bwd ? 2 : 8);
    // 32 < D <= 128, training forward (round 5): the columns as virtual clips of the wide kernels (cmps_wide.hip), when the rho workspace
    // has the sections for it (cmps_rho_workspace_bytes: CMPS_WS_TRAIN and the column vectors fit the LDS); else the general kernels
    const bool wide = h->D > 32 && h->W.vrank > 0 && save_for_bwd != 0 && h->variant_req != CMPS_VARIANT_BLOCK;
    const bool save = save_for_bwd != 0, f16 = rank1_f16(h->rank1_mode);
    hipStream_t s = static_cast<hipStream_t>(stream);
    KBind kb(h);
    hipError_t e;
    if (wide) e = launch_fwd_rho_wide(P, h->W, audio_dev, loss_dev, f16, s);   // k_fwd_wide_rho, k_hy_wide, ... (scopes inside)
    else {
        KScope ks(mfma ? "k_fwd_rho_mfma" : wave ? "k_fwd_rho_wave" : "k_fwd_rho", s);
        e = mfma ? launch_fwd_rho_mfma(P, h->W, audio_dev, loss_dev, save, f16, !h->rho_virtual_bwd, s, Mk)
          : wave ? launch_fwd_rho_wave(P, h->W, audio_dev, loss_dev, save, s, Mk)
                 : launch_fwd_rho(P, h->W, audio_dev, loss_dev, save, s);
    }
    if (e != hipSuccess) return fail_hip(h, e, who);
    h->rho = Saved{save, B, T - 1, audio_dev, loss_dev, wide ? RHO_STASH_WIDE : mfma ? RHO_STASH_MFMA : wave ? RHO_STASH_WAVE : RHO_STASH_BLOCK,
                   save, mfma && !h->rho_virtual_bwd};      // grad1: the forward's part of Rbar exists (k_bwd_rho_mfma needs it)
    h->rho.M = M; h->rho.n_audio = M > 0 ? n_audio : 0;
    return CMPS_OK;
}

int cmps_rho_loss_fwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* loss_dev, int save_for_bwd,
                      void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_fwd(h, "cmps_rho_loss_fwd", in(MODE_PSI), h->rho_set, "cmps_rho_set_state (after cmps_set_params)", audio_dev, loss_dev, B, T,
                                 h->rho_T, h->rho_B, save_for_bwd, h->rho_flags)) return rc;
    return rho_fwd_run(h, "cmps_rho_loss_fwd", 0, 0, audio_dev, B, T, loss_dev, save_for_bwd, stream);
}

// cmps_rho_loss_bwd (M = 0) and cmps_rho_bank_loss_bwd behind their argument checks.  A saved bank forward wrote RHO_STASH_MFMA rows
// (rank >= 3) and rho_bank_check_mode holds, so a bank takes the virtual-clip branch.
static int rho_bwd_run(cmps_handle_t h, const char* who, int M, int n_audio, const float* audio_dev, int B, int T, float* grad_dev, void* stream) {
    const auto failed = [&](hipError_t e, const char* stage) { return fail_hip(h, e, (std::string(who) + stage).c_str()); };
    Dev P = h->P;
    P.B = B; P.T = T; P.N = T - 1;
    const RhoDev W = rho_dev(h);
    if (M > 0) bank_strides(P, n_audio, B, T, 2 * (size_t)h->D * h->D + 3 * (size_t)h->D + 2 + 2 * (size_t)W.rank * h->D);
    const int layout = h->rho.layout;
    float* const loss = h->rho.loss;
    // the reduction runs on the rho slabs (launch_bwd_rho_virtual_wave reads none of the three: it points its own copy at W.wslabs / W.wsums)
    P.slabs = W.slabs; P.sums = W.sums; P.slab_floats = W.slab_floats;
    hipStream_t s = static_cast<hipStream_t>(stream);
    KBind kb(h);
    if (layout == RHO_STASH_WIDE) {                                 // the wide kernels on virtual clips: reverse chain, GEMM, reduction, closing terms
        const hipError_t ew = launch_bwd_rho_wide(P, W, loss, grad_dev, rank1_wide_pieces(h->rank1_mode), s);
        return ew == hipSuccess ? CMPS_OK : failed(ew, " (wide)");
    }
    if (layout == RHO_STASH_MFMA && !h->rho_virtual_bwd && !h->rho.grad1)
        return fail(h, CMPS_ERR_STATE, std::string(who) + ": CMPS_OPT_RHO_BWD changed between the forward and the reverse call");
    if (layout == RHO_STASH_MFMA && h->rho_virtual_bwd) {
        // the row-array forward's rows through the pure-state wave reverse scan, one virtual clip per column (cmps_rho_wave.hip)
        const hipError_t ew = launch_bwd_rho_virtual_wave(P, W, audio_dev, loss, grad_dev, wave_rank1(h->rank1_mode), h->bwd_waves, s, M > 0 ? M : 1);
        return ew == hipSuccess ? CMPS_OK : failed(ew, " (virtual clips)");
    }
    hipError_t e = layout == RHO_STASH_MFMA ? launch_bwd_rho_mfma(P, W, audio_dev, s)
                 : layout == RHO_STASH_WAVE ? launch_bwd_rho_wave(P, W, audio_dev, s) : launch_bwd_rho(P, W, audio_dev, s);
    if (e != hipSuccess) return failed(e, " (scan)");
    P.abar_fix = layout == RHO_STASH_MFMA ? 1 : 0;   // the MFMA scan sums Re(u^dagger (Q + s R^dagger) ybar); k_finalize removes the Q part
    e = launch_reduce_finalize(P, loss, grad_dev, s);
    if (e == hipSuccess) e = launch_finalize_rho(P, W, grad_dev, s);
    if (e != hipSuccess) return failed(e, " (reduce)");
    return CMPS_OK;
}

int cmps_rho_loss_bwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* grad_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = check_bwd(h, "cmps_rho_loss_bwd", in(MODE_PSI), h->rho_set && h->rho.bwd_ok, "cmps_rho_loss_fwd", h->rho, audio_dev, grad_dev, B, T))
        return rc;
    return rho_bwd_run(h, "cmps_rho_loss_bwd", 0, 0, audio_dev, B, T, grad_dev, stream);
}

// ---- model bank of RhoCMPS members (include/cmps.h): the kernel set a plain handle picks at D <= 32, 3 <= rank <= 32 ----

constexpr int RHO_BANK_RANK_MIN = 3, RHO_BANK_RANK_MAX = 32, RHO_BANK_D_MAX = 32;
static bool rho_bank_shape_ok(int D, int rank) {
    return D >= 1 && D <= RHO_BANK_D_MAX && rank >= RHO_BANK_RANK_MIN && rank <= RHO_BANK_RANK_MAX;
}
// What every cmps_rho_bank_* entry that launches scans refuses before it looks at its other arguments: the shapes and the settings whose
// kernels have no member dimension (the block and wide families, the column-by-column wave kernels of CMPS_VARIANT_WAVE32 and of
// rank <= 2, k_bwd_rho_mfma, the one-wave k_bwd_wave)
static int rho_bank_check_mode(cmps_handle_t h, const char* who, int rank) {
    const std::string w(who);
    if (!rho_bank_shape_ok(h->D, rank))
        return fail(h, CMPS_ERR_UNSUPPORTED_D, w + ": a RhoCMPS bank needs D <= 32 and 3 <= rank <= 32");
    if (h->variant_req != CMPS_VARIANT_AUTO && h->variant_req != CMPS_VARIANT_WAVE)
        return fail(h, CMPS_ERR_STATE, w + ": a RhoCMPS bank runs under CMPS_VARIANT_AUTO or CMPS_VARIANT_WAVE only");
    if (!h->rho_virtual_bwd || h->rank1_mode != CMPS_RANK1_DEFAULT || h->bwd_waves != 2 || h->f16_shift != 0)
        return fail(h, CMPS_ERR_STATE, w + ": a RhoCMPS bank runs with the default CMPS_OPT_RHO_BWD, CMPS_OPT_RANK1, CMPS_OPT_BWD_WAVES and "
                                           "CMPS_OPT_F16_SCALE_SHIFT only");
    return CMPS_OK;
}

size_t cmps_rho_bank_workspace_bytes(int D, int rank, int M, int B, int T, int flags) {
    if (M < 1 || M > BANK_MAX || !rho_bank_shape_ok(D, rank)) return 0;
    flags &= ~(CMPS_WS_FRESH | CMPS_WS_REUSE_TABLES);
    const size_t a = cmps_workspace_bytes(D, B, T, CMPS_WS_FWD_ONLY), b = cmps_rho_workspace_bytes(D, rank, B, T, flags);
    return (a && b) ? (size_t)M * (a + b) : 0;
}

int cmps_rho_bank_set_state_dev(cmps_handle_t h, int M, const float* params_dev, const float* phi_dev, int rank, double sigma, double delta_t,
                                int T, int B_max, int flags, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "cmps_rho_bank_set_state_dev";
    const std::string w(who);
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = rho_bank_check_mode(h, who, rank)) return rc;
    if (!params_dev || !phi_dev) return fail(h, CMPS_ERR_BAD_ARG, w + ": null parameter / column buffer");
    if (const int rc = bank_check_M(h, who, M)) return rc;
    if (B_max < 1 || T < 2) return fail(h, CMPS_ERR_BAD_ARG, w + ": need B_max >= 1 and T >= 2");
    if ((unsigned long long)M * (unsigned long long)B_max * (unsigned long long)rank * (unsigned long long)T > 0x7fffffffull)
        return fail(h, CMPS_ERR_BAD_ARG, w + ": M * B_max * rank * T overflows");
    if (!workspace_dev) return fail(h, CMPS_ERR_WORKSPACE, w + ": null workspace");
    const int rflags = flags & ~(CMPS_WS_FRESH | CMPS_WS_REUSE_TABLES);
    const RhoLayout RL = make_rho_layout(h->D, rank, B_max, T, rflags);
    // every member's tables (the main layout without its training sections), the size and alignment checks of the whole workspace
    if (const int rc = set_params_packed(h, params_dev, sigma, delta_t, T, B_max, flags & ~CMPS_WS_TRAIN, workspace_dev, workspace_bytes, stream,
                                         MODE_RHO_BANK, M, RL.total)) return rc;
    // member 0's rho sections lie behind its main layout; rho_bank_view / bank_view / bank_view_phi move them by the one stride
    const RhoDev W = bind_rho_workspace(h->D, RL, h->ws + h->L.total, rflags, B_max);
    const hipError_t e = launch_pack_phi(h->P, W, phi_dev, phi_dev + (size_t)rank * h->D, static_cast<hipStream_t>(stream), M);
    if (e != hipSuccess) { unconfigure(h); return fail_hip(h, e, who); }
    h->RL = RL; h->W = W;
    h->rho_B = B_max; h->rho_T = T; h->rho_flags = rflags;
    h->rho.valid = h->rho.bwd_ok = false;
    return CMPS_OK;
}

int cmps_rho_bank_loss_fwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* loss_dev, int save_for_bwd, void* stream) {
    const char* who = "cmps_rho_bank_loss_fwd";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (h->mode == MODE_RHO_BANK) if (const int rc = rho_bank_check_mode(h, who, h->W.rank)) return rc;
    if (const int rc = check_fwd(h, who, in(MODE_RHO_BANK), true, "cmps_rho_bank_set_state_dev", audio_dev, loss_dev, B, T, h->rho_T, h->rho_B,
                                 save_for_bwd, h->rho_flags)) return rc;
    if (n_audio != 1 && n_audio != h->bank_M) return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": n_audio must be 1 (one shared batch) or M");
    return rho_fwd_run(h, who, h->bank_M, n_audio, audio_dev, B, T, loss_dev, save_for_bwd, stream);
}

int cmps_rho_bank_loss_bwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* grad_dev, void* stream) {
    const char* who = "cmps_rho_bank_loss_bwd";
    if (!h) return CMPS_ERR_BAD_ARG;
    const bool saved = h->rho.bwd_ok && h->rho.M == h->bank_M;     // (the options are judged only where a reverse pass could run)
    if (h->mode == MODE_RHO_BANK && saved) if (const int rc = rho_bank_check_mode(h, who, h->W.rank)) return rc;
    if (const int rc = check_bwd(h, who, in(MODE_RHO_BANK), saved, "cmps_rho_bank_loss_fwd", h->rho, audio_dev, grad_dev, B, T)) return rc;
    if (n_audio != h->rho.n_audio) return fail(h, CMPS_ERR_STATE, std::string(who) + ": n_audio differs from the forward call");
    return rho_bwd_run(h, who, h->bank_M, n_audio, audio_dev, B, T, grad_dev, stream);
}

size_t cmps_rho_bank_apply_step_scratch_bytes(int D, int rank, int M) {
    return (M < 1 || M > BANK_MAX || !rho_bank_shape_ok(D, rank)) ? 0 : (size_t)M * cmps_rho_apply_step_scratch_bytes(D, rank);
}

int cmps_rho_bank_apply_step(cmps_handle_t h, int M, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev, int rank,
                             double global_batch, double bias_num, double bias_den, double beta1, double beta2, double epsilon,
                             const double* hyper_dev, int with_reg, float* params_dev, float* phi_dev, float* losses_dev, void* scratch_dev,
                             void* stream) {
    const char* who = "cmps_rho_bank_apply_step";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (!rho_bank_shape_ok(h->D, rank)) return fail(h, CMPS_ERR_UNSUPPORTED_D, std::string(who) + ": a RhoCMPS bank needs D <= 32 and 3 <= rank <= 32");
    if (!vars_dev || !params_dev || !phi_dev || !hyper_dev)
        return fail(h, CMPS_ERR_BAD_ARG, std::string(who) + ": null variable / parameter / column / hyper-parameter buffer");
    if (const int rc = bank_check_M(h, who, M)) return rc;
    if (const int rc = check_apply_step(h, who, grad_sums_dev, adam_m_dev, adam_v_dev, losses_dev, scratch_dev, global_batch, hyper_dev)) return rc;
    const bool apply = grad_sums_dev != nullptr;
    const hipError_t e = launch_rho_bank_apply_step(h->D, rank, M, apply, apply ? 1.0 / global_batch : 0.0, bias_num, bias_den, beta1, beta2,
                                                    epsilon, hyper_dev, with_reg != 0, vars_dev, adam_m_dev, adam_v_dev, grad_sums_dev,
                                                    params_dev, phi_dev, losses_dev, static_cast<double*>(scratch_dev),
                                                    static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, who);
    return CMPS_OK;
}

int cmps_rho_update_ancilla(cmps_handle_t h, const float* rho_in_dev, const float* signal_dev, float t, int B,
                            float* rho_out_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_plain(h, "cmps_rho_update_ancilla", in(MODE_PSI), true, ": call cmps_set_params first")) return rc;
    if (!rho_in_dev || !signal_dev || !rho_out_dev || B < 1 || rho_in_dev == rho_out_dev)
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_update_ancilla: bad argument");
    hipError_t e = launch_update_ancilla_rho(h->P, rho_in_dev, signal_dev, t, B, rho_out_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_rho_update_ancilla");
    return CMPS_OK;
}

// The RhoCMPS sampler kernel of a handle (after cmps_rho_set_state).  D <= 32 (rank <= 32): the row-array GEMM sampler, one wavefront
// per path (cmps_rho_mfma.hip); CMPS_VARIANT_BLOCK keeps the general workgroup-per-path kernel (cross-check; 93 us per step at rank 32
// against 2 us)
static bool rho_sampler_mfma(const cmps_handle_s* h) { return h->D <= 32 && h->W.rank <= 32 && h->variant_req != CMPS_VARIANT_BLOCK; }
// floats of one stream-state record of that kernel
static int rho_stream_rec_floats(const cmps_handle_s* h) {
    return rho_sampler_mfma(h) ? stream_rec_rho_mfma(h->W.rank) : stream_rec_rho(h->W.rank, h->D);
}

// What cmps_rho_sample, cmps_rho_sample_primed, cmps_rho_stream and cmps_rho_stream_score do behind their own argument checks: the
// workspace checks, the kernel choice, the launch of one SampleDev and the record for cmps_rho_states.  The scan has S.PR.PF + S.length steps.
static int rho_sample_run(cmps_handle_t h, const char* who, const SampleDev& S, int save_states, void* stream) {
    const std::string w(who);
    const int n = S.n, steps = S.PR.PF + S.length;
    const bool mfma = rho_sampler_mfma(h);
    const SampleMode mode = sample_mode(S);
    static const char* const names[2][4] = {{"k_sample_rho", "k_sample_rho_primed", "k_sample_rho_stream", "k_sample_rho_score"},
                                            {"k_sample_rho_mfma", "k_sample_rho_mfma_primed", "k_sample_rho_mfma_stream",
                                             "k_sample_rho_mfma_score"}};   // [mfma][SampleMode]
    static const char* const steps_name[4] = {"length", "(prime_T-1+length)", "(forced+length)", "forced"};
    // (only when the SAMPLER's three column arrays exceed the LDS: the workspace section exists from a smaller rank * D on, for the
    // reverse scan's four -- ADVICE r3)
    if (!mfma && rho_cols_spill(3, h->W.rank, h->P.D) && n > h->rho_B)
        return fail(h, CMPS_ERR_WORKSPACE, w + ": at this rank * D the columns live in the workspace: n must not exceed B_max");
    if (save_states && (!(h->rho_flags & CMPS_WS_TRAIN) || (size_t)n * steps > (size_t)h->rho_B * (h->rho_T - 1)))
        return fail(h, CMPS_ERR_WORKSPACE, w + ": save_states needs a CMPS_WS_TRAIN rho workspace with B_max*(T-1) >= n*" + steps_name[mode]);
    hipStream_t s = static_cast<hipStream_t>(stream);
    KBind kb(mode != SAMPLE_PLAIN ? h : nullptr);                // (cmps_rho_sample records no kernel events, as before)
    KScope ks(names[mfma][mode], s);
    const hipError_t e = mfma ? launch_sample_rho_mfma(h->P, h->W, S, save_states != 0, rank1_f16(h->rank1_mode), s)
                              : launch_sample_rho(h->P, h->W, S, save_states != 0, s);
    if (e != hipSuccess) return fail_hip(h, e, who);
    if (S.MB.M > 0) return CMPS_OK;                              // (a bank's segment wrote no stash: a saved cmps_rho_bank_loss_fwd stays what it was)
    h->rho = Saved{save_states != 0, n, steps, nullptr, nullptr, mfma ? RHO_STASH_MFMA : RHO_STASH_BLOCK};   // (no reverse pass after a sampler)
    h->rho.k0 = S.ST ? S.ST->k0 : 0;                             // cmps_rho_states: the phases of the saved steps are ttab[k0 + k]
    return CMPS_OK;
}

int cmps_rho_sample(cmps_handle_t h, const float* noise_dev, int n, int length, float* out_dev, int save_states,
                    void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_mode(h, "cmps_rho_sample", in(MODE_PSI), h->rho_set, ": call cmps_set_params and cmps_rho_set_state first")) return rc;
    if (!noise_dev || !out_dev || n < 1 || length < 1) return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_sample: bad argument");
    if (length > h->L.N) return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_sample: length exceeds T - 1 of cmps_set_params");
    return rho_sample_run(h, "cmps_rho_sample", SampleDev{noise_dev, n, length, out_dev, PrimeDev{}, nullptr, nullptr}, save_states, stream);
}

int cmps_rho_sample_primed(cmps_handle_t h, const float* prime_dev, int n_prime, int prime_T, const float* noise_dev, int n, int length,
                           float* out_dev, float* pred_dev, int save_states, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_mode(h, "cmps_rho_sample_primed", in(MODE_PSI), h->rho_set,
                                 ": call cmps_set_params and cmps_rho_set_state first (not available in legacy mode)")) return rc;
    SampleDev S;
    if (int c = primed_args(h, "cmps_rho_sample_primed", prime_dev, n_prime, prime_T, noise_dev, n, length, out_dev, pred_dev, S)) return c;
    return rho_sample_run(h, "cmps_rho_sample_primed", S, save_states, stream);
}

size_t cmps_rho_stream_state_bytes(cmps_handle_t h, int n) {
    if (!h || n < 1 || h->mode != MODE_PSI || !h->rho_set) return 0;
    return (size_t)n * rho_stream_rec_floats(h) * sizeof(float);
}

int cmps_rho_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, int forced,
                    const float* noise_dev, int length, int n, float* out_dev, float* pred_dev, int save_states, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_mode(h, "cmps_rho_stream", in(MODE_PSI), h->rho_set,
                                 ": call cmps_set_params and cmps_rho_set_state first (not available in legacy mode)")) return rc;
    StreamCall C;
    if (int c = stream_args(h, "cmps_rho_stream", state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, noise_dev, n, length, n, out_dev, pred_dev,
                            rho_stream_rec_floats(h), plain_rows, MemberDev{}, C))
        return c;
    return rho_sample_run(h, "cmps_rho_stream", C.S, save_states, stream);
}

int cmps_rho_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, int forced,
                          int n, float* nll_dev, float* loss_dev, float* pred_dev, int save_states, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_mode(h, "cmps_rho_stream_score", in(MODE_PSI), h->rho_set,
                                 ": call cmps_set_params and cmps_rho_set_state first (not available in legacy mode)")) return rc;
    StreamCall C;
    if (int c = score_args(h, "cmps_rho_stream_score", state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, n, nll_dev, loss_dev, pred_dev,
                           rho_stream_rec_floats(h), "path", plain_rows, MemberDev{}, C))
        return c;
    return rho_sample_run(h, "cmps_rho_stream_score", C.S, save_states, stream);
}

// ---- a RhoCMPS bank's streams: k_sample_rho_mfma's STREAM / SCORE instances with the members as a second grid dimension (include/cmps.h) ----
// What cmps_rho_bank_stream and cmps_rho_bank_stream_score refuse before they look at their arguments
static int rho_bank_stream_check_mode(cmps_handle_t h, const char* who) {
    if (const int rc = need_mode(h, who, in(MODE_RHO_BANK), true, ": needs a RhoCMPS bank (call cmps_rho_bank_set_state_dev first)")) return rc;
    if (const int rc = rho_bank_check_mode(h, who, h->W.rank)) return rc;        // (a variant or an option set behind cmps_rho_bank_set_state_dev)
    return CMPS_OK;
}

size_t cmps_rho_bank_stream_state_bytes(cmps_handle_t h, int n) {
    if (!h || n < 1 || h->mode != MODE_RHO_BANK) return 0;
    return (size_t)h->bank_M * (size_t)n * stream_rec_rho_mfma(h->W.rank) * sizeof(float);
}

int cmps_rho_bank_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, int forced,
                         const float* noise_dev, int n_noise, int length, int n, float* out_dev, float* pred_dev, void* stream) {
    const char* who = "cmps_rho_bank_stream";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = rho_bank_stream_check_mode(h, who)) return rc;
    const MemberDev MB{h->bank_M, audio_dev ? bank_member_stride(h, n_audio, n, (size_t)forced + 1) : 0,
                       length > 0 ? bank_member_stride(h, n_noise, n, (size_t)length) : 0};
    StreamCall C;
    if (int c = stream_args(h, who, state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, noise_dev, n_noise, length, n, out_dev, pred_dev,
                            stream_rec_rho_mfma(h->W.rank), bank_rows, MB, C))
        return c;
    return rho_sample_run(h, who, C.S, 0, stream);
}

int cmps_rho_bank_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio,
                               int forced, int n, float* nll_dev, float* loss_dev, float* pred_dev, void* stream) {
    const char* who = "cmps_rho_bank_stream_score";
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = rho_bank_stream_check_mode(h, who)) return rc;
    StreamCall C;
    if (int c = score_args(h, who, state_in_dev, state_out_dev, k0, audio_dev, n_audio, forced, n, nll_dev, loss_dev, pred_dev,
                           stream_rec_rho_mfma(h->W.rank), "member and path", bank_rows,
                           MemberDev{h->bank_M, bank_member_stride(h, n_audio, n, (size_t)forced + 1), 0}, C))
        return c;
    return rho_sample_run(h, who, C.S, 0, stream);
}

int cmps_rho_states(cmps_handle_t h, int B, int steps, float* rho_out_dev, float* purity_out_dev, void* stream) {
    if (!h) return CMPS_ERR_BAD_ARG;
    if (const int rc = need_mode(h, "cmps_rho_states", in(MODE_PSI), h->rho_set && h->rho.valid,
                                 ": needs cmps_rho_loss_fwd(save_for_bwd=1) or cmps_rho_sample(save_states=1) first")) return rc;
    if (B != h->rho.B || steps != h->rho.steps || (!rho_out_dev && !purity_out_dev))
        return fail(h, CMPS_ERR_BAD_ARG, "cmps_rho_states: bad argument");
    Dev P = h->P;
    P.ttab += h->rho.k0;                                         // (a stream segment's step k was taken at t_{k0 + k})
    hipError_t e = launch_states_rho(P, rho_dev(h), B, steps, rho_out_dev, purity_out_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(h, e, "cmps_rho_states");
    return CMPS_OK;
}

// ---------------------------------------------------------------------------------------------------
// per-kernel durations recorded while CMPS_OPT_KERNEL_EVENTS is on
// ---------------------------------------------------------------------------------------------------
int cmps_kernel_times(cmps_handle_t h, char* names, size_t names_bytes, float* ms_sum, int* calls, int cap) {
    if (!h) return -1;
    if (!h->ktimer) { fail(h, CMPS_ERR_STATE, "cmps_kernel_times: CMPS_OPT_KERNEL_EVENTS is off"); return -1; }
    if (!names || !ms_sum || !calls || cap < 1 || names_bytes < 1) { fail(h, CMPS_ERR_BAD_ARG, "cmps_kernel_times: bad argument"); return -1; }
    KTimer* t = h->ktimer;
    std::vector<const char*> order;
    std::vector<double> sum;
    std::vector<int> cnt;
    for (auto& r : t->recs) {
        if (hipEventSynchronize(r.b) != hipSuccess) { fail(h, CMPS_ERR_HIP, "cmps_kernel_times: hipEventSynchronize"); return -1; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        size_t i = 0;
        for (; i < order.size(); ++i) if (!strcmp(order[i], r.name)) break;
        if (i == order.size()) { order.push_back(r.name); sum.push_back(0.0); cnt.push_back(0); }
        sum[i] += ms; cnt[i] += 1;
        t->pool.push_back(r.a); t->pool.push_back(r.b);
    }
    t->recs.clear();
    std::string joined;
    int n = 0;
    for (size_t i = 0; i < order.size() && n < cap; ++i, ++n) {
        if (i) joined += '\n';
        joined += order[i];
        ms_sum[n] = (float)sum[i];
        calls[n] = cnt[i];
    }
    if (joined.size() + 1 > names_bytes) { fail(h, CMPS_ERR_BAD_ARG, "cmps_kernel_times: names buffer too small"); return -1; }
    memcpy(names, joined.c_str(), joined.size() + 1);
    return n;
}

// ---------------------------------------------------------------------------------------------------
// host utility of the data-format row: CRC-32C (Castagnoli) of TFRecord framing
// ---------------------------------------------------------------------------------------------------
unsigned cmps_crc32c(const void* data, size_t n, unsigned crc_in) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    unsigned long long crc = crc_in ^ 0xFFFFFFFFu;
#if defined(__SSE4_2__)
    while (n && ((uintptr_t)p & 7)) { crc = __builtin_ia32_crc32qi((unsigned)crc, *p++); --n; }
    for (; n >= 8; n -= 8, p += 8) {
        unsigned long long v;
        memcpy(&v, p, 8);
        crc = __builtin_ia32_crc32di(crc, v);
    }
    while (n--) crc = __builtin_ia32_crc32qi((unsigned)crc, *p++);
#else
    static unsigned table[256];
    static bool init = false;
    if (!init) {
        for (unsigned i = 0; i < 256; ++i) {
            unsigned c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            table[i] = c;
        }
        init = true;
    }
    while (n--) crc = table[(crc ^ *p++) & 0xFF] ^ (crc >> 8);
#endif
    return (unsigned)crc ^ 0xFFFFFFFFu;
}

}  // extern "C"
