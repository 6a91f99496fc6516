/*
 * cmps.h -- C ABI of libcmps.so: the MI355X (gfx950) implementation of audio-mps's per-timestep cMPS
 * contraction scan (PsiCMPS log-likelihood forward and its gradient).
 *
 * The reference has no FFI: the path sits behind Python object attributes (PsiCMPS(...).loss,
 * /root/reference/model.py:211-225, 257-334) and its gradient is produced by TensorFlow's autodiff
 * (train.py:89).  Each entry point below names the reference lines it replaces.  All pointers named
 * *_dev are DEVICE pointers owned by the caller; the library allocates no device memory, launches
 * everything asynchronously on the caller's stream and never synchronises.  `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).  A handle must not be shared between host threads.
 *
 * Every function returns CMPS_OK (0) or a CMPS_ERR_* code; cmps_last_error(h) gives the message.
 * NaN / Inf in the loss is NOT an error at this boundary (it propagates, as in the reference where
 * only tests/test_model.py:113 looks at it) -- into the loss of THAT clip: the forward entries (cmps_psi_loss_fwd with either value
 * of save_for_bwd, cmps_legacy_loss_fwd, cmps_rho_loss_fwd, the scored streams) keep the clips of a batch apart, also where one
 * workgroup runs several of them; a clip with a NaN, an Inf or a sample of 2^40 leaves the losses of the others where the clean batch
 * has them (tests/test_gpu_wild_clip.py).  The gradient sums of such a batch are non-finite by definition.
 */
#ifndef CMPS_H_
#define CMPS_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cmps_handle_s* cmps_handle_t;

enum {
    CMPS_OK = 0,
    CMPS_ERR_BAD_ARG = 1,       /* null pointer, non-positive size, T < 2 ... */
    CMPS_ERR_UNSUPPORTED_D = 2, /* bond dimension outside [1, 128] */
    CMPS_ERR_WORKSPACE = 3,     /* workspace missing or smaller than cmps_workspace_bytes() */
    CMPS_ERR_HIP = 4,           /* a HIP runtime call or kernel launch failed */
    CMPS_ERR_STATE = 5,         /* call order: set_params -> fwd(save_for_bwd=1) -> bwd */
    CMPS_ERR_F16_RANGE = 6      /* cmps_psi_grad_status only: the gradient sums of the last cmps_psi_loss_bwd hold Inf / NaN although
                                 * every per-clip loss is finite -- an fp16-split operand left its scaled range (see CMPS_RANK1_F16X2) */
};

/* workspace flags */
enum {
    CMPS_WS_FWD_ONLY = 0, /* loss only */
    CMPS_WS_TRAIN = 1,    /* forward + backward (adds the per-step state stash and gradient slabs) */
    CMPS_WS_REUSE_TABLES = 4, /* OR-ed into `flags` of cmps_set_params: the caller vouches that the workspace still holds what the
                           * handle's previous cmps_set_params left in it -- the time table is then rebuilt only when T or delta_t
                           * changed.  WITHOUT this flag every call rebuilds every table (the safe default for a C caller). */
    CMPS_WS_FRESH = 2     /* (kept for v200 callers; now the default behaviour) the workspace memory was (re)allocated, zeroed or used
                           * for something else since the previous call -- rebuild every cached table (see below) */
};

/* Kernel variants (cmps_set_variant).  AUTO picks the register-resident wave-per-clip kernels for D <= 32 and the "wide"
 * kernels above that.  Both follow the reference's float32 / complex64 arithmetic (model.py:300-325) in this sense:
 *   - state, identity part of every update, normalisation, loss and every accumulation are float32;
 *   - D <= 32: the mat-vec on the serial chain is an fp32 FMA chain.  The two products nothing waits for run on the matrix
 *     cores with split operands and fp32 accumulation: the loss product H y and the rank-1 gradient sums
 *     (both follow CMPS_OPT_RANK1; default two scaled fp16 pieces, three products);
 *   - 32 < D <= 128: the mat-vecs of both serial chains, H y and the gradient GEMM all run on the matrix cores with two
 *     scaled fp16 pieces per operand (CMPS_OPT_WIDE_CHAIN, CMPS_OPT_RANK1 select the fp32-VALU / bf16-piece forms).
 * Split products carry 22-24 operand bits: within float32 rounding of an fp32 FMA chain, not bit-identical to it.
 * Only CMPS_VARIANT_BLOCK is plain fp32 FMA code throughout. */
enum {
    CMPS_VARIANT_AUTO = 0,
    CMPS_VARIANT_BLOCK = 1, /* one workgroup per clip, any D <= 128 */
    CMPS_VARIANT_WAVE = 2,  /* wavefront-per-clip kernels, state and R in registers, D <= 32: the 16-row lane layout
                             * (cmps_wave16.hip) for D <= 16, the 32-row layout above that */
    CMPS_VARIANT_PAIR = 3,  /* 32 < D <= 128: one workgroup per pair of clips, matrices as bf16 MFMA fragments, fp32 accumulate */
    CMPS_VARIANT_WAVE32 = 4, /* the 32-row wave layout for every D <= 32 (zero padding below 32; cross-check of the 16-row layout) */
    CMPS_VARIANT_WIDE = 5   /* 32 < D <= 128 in float32 (what AUTO picks there): one workgroup per pair of clips, R / Q resident in
                             * registers for the whole launch; arithmetic selected by CMPS_OPT_WIDE_CHAIN and CMPS_OPT_RANK1 */
};

/* options (cmps_set_option / cmps_get_option) */
enum {
    CMPS_OPT_RANK1 = 1 /* arithmetic of the rank-1 gradient sums: the wave-per-clip reverse scan of 17 <= D <= 32 (the 16-row layout
                        * of D <= 16 always uses exact fp32 MFMAs) and the gradient GEMM of the wide kernels (32 < D <= 128:
                        * BF16X2 = two bf16 pieces / three products, F16X2 = two fp16 pieces / three products, anything else = three
                        * bf16 pieces / six products) */,
    CMPS_OPT_WIDE_CHAIN = 3 /* how the wide kernels (32 < D <= 128, float32) run the training forward's serial chain: see the values below */,
    CMPS_OPT_RHO_BWD = 5 /* which reverse sweep follows the RhoCMPS row-array GEMM forward (D <= 32; the forward runs from rank 3 with
                        * CMPS_RHO_BWD_VIRTUAL, from rank 9 with CMPS_RHO_BWD_GEMM, the column-by-column kernels below that): see the values below */,
    CMPS_OPT_BWD_WAVES = 6 /* the reverse scan of 17 <= D <= 32 (PsiCMPS arithmetic, F16X2 sums): 2 (default) = two wavefronts per clip on one
                        * SIMD, a chain wave and a gradient wave (k_bwd_wave2w, cmps_wave_bwd2.hip); 1 = one wavefront per clip (k_bwd_wave,
                        * the round-4 kernel: the A/B setting).  Same float32 tolerances; every other CMPS_OPT_RANK1 value, a non-zero
                        * CMPS_OPT_F16_SCALE_SHIFT and the legacy mode run one wavefront whatever this says; the RhoCMPS reverse sweep on virtual clips
                        * (CMPS_OPT_RHO_BWD) follows it.
                        * The SAVED FORWARD is tied to the reverse kernel it was written for: when cmps_psi_loss_fwd(save_for_bwd = 1) runs
                        * with the settings of k_bwd_wave2w (17 <= D <= 32 or CMPS_VARIANT_WAVE32, this option 2, F16X2 / DEFAULT sums, no
                        * scale shift), its stash rows are written normalised, (yhat_k, 2 ebar_k H y_k) instead of (y_k, H y_k), and the
                        * cmps_psi_loss_bwd of that forward runs k_bwd_wave2w whatever this option, CMPS_OPT_RANK1 and
                        * CMPS_OPT_F16_SCALE_SHIFT say by then: they take effect with the next forward.  cmps_psi_states reads either kind. */,
    CMPS_OPT_SAVED_ROWS = 7 /* READ-ONLY (cmps_get_option): 1 when the main workspace holds a saved pure-state forward with normalised stash
                        * rows (see CMPS_OPT_BWD_WAVES), else 0 */,
    CMPS_OPT_F16_SCALE_SHIFT = 4 /* DIAGNOSTIC, default 0: added to the exponent of every data-dependent fp16 scale of the wave reverse
                        * scan's F16X2 arithmetic (range -40 .. 40).  A positive value pushes the pieces out of fp16 range on purpose:
                        * how tests/test_gpu_parity.py provokes CMPS_ERR_F16_RANGE.  No reference counterpart. */,
    CMPS_OPT_KERNEL_EVENTS = 2 /* 1: every kernel cmps_psi_loss_fwd / _bwd, cmps_rho_loss_fwd / _bwd, cmps_psi_sample, cmps_psi_sample_primed, cmps_psi_stream, cmps_psi_stream_score, cmps_rho_sample_primed, cmps_rho_stream, cmps_rho_stream_score, cmps_noise_fill (as k_noise_philox), cmps_batch_gather (as k_batch_gather), cmps_batch_gather_i16 (as k_batch_gather_i16), cmps_loss_stats (as k_loss_stats), cmps_bank_classify_stats (as k_classify_stats), cmps_bank_classify_weights (as k_classify_weights), cmps_bank_posterior (as k_bank_posterior), cmps_bank_calibrate (as k_calib_pass and k_calib_update, one pair per iteration), cmps_bank_loss_bwd_weighted (the scan of cmps_bank_loss_bwd, then "reduce + finalize (weighted)") and cmps_damped_sine_fill (as k_damped_sine) launch is bracketed by two HIP events on the caller's stream
                        * (read and reset with cmps_kernel_times); 0 (default): nothing is recorded.  A measurement aid -- the reference
                        * has no counterpart (no tracing / profiling hooks); bench.py uses it OUTSIDE its timed region to price
                        * each kernel of a multi-kernel family against the pipe it runs on */
};
/* Values of CMPS_OPT_RANK1.  All accumulate in fp32; they differ in how the two factors of every product
 * dR += a b^dagger enter the matrix cores:
 *   EXACT_F32  v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 fma chain (slowest: it holds the fp32 ALUs).
 *   BF16X2     each factor split into two bf16 pieces, 3 products: 16 operand bits, error <= ~2^-16 |a||b|.
 *   BF16X3     each factor split EXACTLY into three bf16 pieces (8+8+8 bits), 6 products: 24 operand bits,
 *              error <= 2^-23 |a||b| (what is dropped is below the fp32 rounding of the product).
 *   F16X2      each factor multiplied by a power of two and split into two fp16 pieces, round to nearest
 *              (11+1+11+1 bits), 3 products on v_mfma_f32_32x32x16_f16 / 16x16x32_f16: BF16X2's instruction count in
 *              BF16X3's accuracy class.  Error <= ~2^-22 |a||b| for factors within 2^-18 of the largest value their
 *              scale was chosen for, and <= 2^-39 of that largest value below.
 * Which kernels know which value, and where the fp16 scales come from:
 *   kernel                                        EXACT_F32  BF16X2  BF16X3  F16X2                          DEFAULT means
 *   wave reverse scan, 17 <= D <= 32 (PsiCMPS)    yes        yes     yes     scales per eight-step octet    F16X2
 *   wave reverse scan in legacy AudioMPS mode     yes        yes     yes     runs BF16X3                    BF16X3
 *   wave kernels, D <= 16                         always exact fp32 MFMAs (the option is ignored)
 *   wide kernels' H y GEMM (forward), D > 32      runs BF16X3  yes   yes     scales per clip                F16X2
 *   wide kernels' gradient GEMM, D > 32           runs BF16X3  yes   yes     scales per pair of clips       F16X2
 *   RhoCMPS row-array GEMM forward and sampler    runs BF16X3 (every value but F16X2 / DEFAULT)  scales per clip / fixed   F16X2
 *   RhoCMPS reverse scan, pair (bf16) kernels     the option is ignored
 * The fp16 scales follow guaranteed bounds; should one ever be violated the pieces overflow to Inf and the gradient
 * comes out non-finite: cmps_psi_grad_status reports that as CMPS_ERR_F16_RANGE. */
enum {
    CMPS_RANK1_EXACT_F32 = 0,
    CMPS_RANK1_BF16X2 = 1,
    CMPS_RANK1_BF16X3 = 2,
    CMPS_RANK1_F16X2 = 3,
    CMPS_RANK1_DEFAULT = 4   /* a new handle's setting: see the table above (the cheapest arithmetic of the 24-operand-bit
                              * class each kernel has; scripts/rank1_accuracy_wide.py,
                              * tests/test_gpu_parity.py::test_rank1_modes_order_of_accuracy) */
};

/* values of CMPS_OPT_RHO_BWD */
enum {
    CMPS_RHO_BWD_VIRTUAL = 0,  /* (a new handle's setting) every column of rho as one clip of the pure-state wave reverse scan (k_bwd_wave): given
                                * the clip's per-step scalars the column cotangents do not couple; cost linear in the rank, rank-1 sums in the
                                * CMPS_OPT_RANK1 arithmetic */
    CMPS_RHO_BWD_GEMM = 1      /* k_bwd_rho_mfma: the cotangent array as row-array GEMMs (bf16 x 3), the same cost at every rank <= 32 */
};

/* values of CMPS_OPT_WIDE_CHAIN */
enum {
    CMPS_WIDE_CHAIN_VALU = 0,   /* k_fwd_wide: the mat-vec as fp32 v_pk_fma_f32 chains (R, Q register resident) */
    CMPS_WIDE_CHAIN_MFMA_FWD = 2,  /* the forward as MFMA below, the reverse scan as VALU (k_bwd_wide): for A/B measurements */
    CMPS_WIDE_CHAIN_MFMA = 1    /* (a new handle's setting) k_fwd_chain16 / k_bwd_chain16: the correction (Q + s R) u as power-of-two scaled fp16 x 2 split operands on
                                 * v_mfma_f32_16x16x32_f16 (three products, fp32 accumulate: the accuracy class of CMPS_RANK1_F16X2);
                                 * the forward scales each clip's vector from that clip's own largest |s| (the matrices' scales are shared);
                                 * identity part and everything behind the mat-vec in float32 */
};

/* Library version (major * 10000 + minor * 100 + patch). */
int cmps_version(void);

/* Replaces: construction of the model object's constant part, CMPS.__init__ (model.py:9-52).
 * D = hparams.bond_dim. */
int cmps_create(int D, cmps_handle_t* out);
int cmps_destroy(cmps_handle_t h);
const char* cmps_last_error(cmps_handle_t h);
int cmps_set_variant(cmps_handle_t h, int variant);
/* The variant the next launch will use (after AUTO resolution): CMPS_VARIANT_BLOCK, _WAVE, _PAIR, _WAVE32 or _WIDE. */
int cmps_get_variant(cmps_handle_t h);
/* Numerical options of the gradient path; the reference has one arithmetic (TensorFlow float32 kernels behind
 * train.py:89), so every value of every option must stay within the stated float32 tolerance of it.
 * cmps_get_option returns the value, or -1 for an unknown option / null handle. */
int cmps_set_option(cmps_handle_t h, int option, int value);
int cmps_get_option(cmps_handle_t h, int option);
/* With CMPS_OPT_KERNEL_EVENTS on: waits for the recorded events, writes per kernel name (in first-launch order) the summed milliseconds
 * and the launch count since the last call, the names '\n'-joined into `names`; returns the number of distinct kernels (<= cap), -1 on
 * error (option off, bad argument, buffer too small).  Resets the record.  No reference counterpart (see CMPS_OPT_KERNEL_EVENTS). */
int cmps_kernel_times(cmps_handle_t h, char* names, size_t names_bytes, float* ms_sum, int* calls, int cap);

/* Bytes of device workspace the caller must provide for bond dimension D, B clips of T samples.
 * Returns 0 for invalid arguments. */
size_t cmps_workspace_bytes(int D, int B, int T, int flags);

/*
 * Replaces: the parameter-derived constants that the TF graph rebuilds on every session.run --
 * model.py:41-42 (complex R), :52 (freqsc), :304-305 / :321-322 (phases = exp(1j * freqsc * t) for every
 * step, with t accumulated as a sequential float32 sum, model.py:16, 266, 281), :308 (adjoint(R)),
 * :312 (-delta_t * sigma**2 / 2 factor), :221-222 (psi_0).
 * Inputs are the EFFECTIVE parameters (after the rsqrt(reg) scaling and the diagonal removal of
 * model.py:36-42, 49), float32, on the device:
 *   R_re_dev, R_im_dev [D*D] row-major R[i][j];  freqs_dev [D];  psi0_re_dev, psi0_im_dev [D] (normalised).
 * A = model.A (model.py:19), sigma (model.py:21), delta_t (model.py:15), T = samples per clip.
 * Builds, on `stream`, inside `workspace_dev`: R^T, Q = -(delta_t sigma^2 / 2) R^dagger R, the float32
 * time table t_k, and the per-step phase-rotation table.
 * Caching contract: the time table depends only on (T, delta_t).  By default every call rebuilds it (~0.7 ms at T = 16000);
 * a caller that keeps the workspace untouched between calls passes CMPS_WS_REUSE_TABLES and the table is rebuilt only when the
 * workspace address, T or delta_t differ from the handle's previous call.  The workspace is caller-owned memory: after
 * freeing, zeroing, re-obtaining (an allocator may hand back the same address) or sharing it, drop the flag for one call.
 * Everything else in the workspace is rebuilt by every call.
 */
int cmps_set_params(cmps_handle_t h, const float* R_re_dev, const float* R_im_dev,
                    const float* freqs_dev, const float* psi0_re_dev, const float* psi0_im_dev,
                    float A, double sigma, double delta_t, int T, int B_max, int flags,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/*
 * cmps_set_params with every parameter -- model.A (model.py:19) included -- read from device memory:
 *   params_dev [2 D^2 + 3 D + 1] = R_re [D*D] | R_im [D*D] | freqs [D] | psi0_re [D] | psi0_im [D] | A,
 * the buffer cmps_psi_apply_step writes.  The scan kernels then load A from params_dev + 2 D^2 + 3 D, so a training loop needs
 * no device -> host copy between steps.  Everything else as cmps_set_params.
 */
int cmps_set_params_dev(cmps_handle_t h, const float* params_dev, double sigma, double delta_t, int T, int B_max, int flags,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/*
 * Replaces: the optimiser half of a training step, which the reference runs inside session.run(train_op) --
 * tf.train.AdamOptimizer(learning_rate).minimize(total_loss) (train.py:88-89; beta1 0.9, beta2 0.999, epsilon 1e-8:
 * logging/graph.pbtxt:32102-32192), i.e. the chain rule from the effective parameters back to the trainable variables
 * (adjoint of model.py:36-42, 49, 221-222), the regularisers total = loss + h_reg sum freqs^2 + r_reg sum |R|^2 of
 * train.py:55-60 (with_reg != 0), the Adam update, and the next step's effective parameters (model.py:36-42, 49, 221-222).
 *   vars_dev, adam_m_dev, adam_v_dev [2 D^2 + 3 D + 1]: A | Rx [D*D] | Ry [D*D] | freqs [D] | psi_x [D] | psi_y [D]  (in / out)
 *   grad_sums_dev [2 D^2 + 3 D + 2]: the buffer of cmps_psi_loss_bwd, summed over all ranks; global_batch = clips it covers.
 *     NULL: no update -- only params_dev is computed from vars_dev (the first step).
 *   lr_t = learning_rate * sqrt(1 - beta2^t) / (1 - beta1^t) for the step count t the caller keeps (train.py:88 global_step).
 *   c_r, c_h: the rsqrt(r_reg), rsqrt(h_reg) factors of model.py:36-39, 49 (1 when R_in / freqs_in were given).
 *   params_dev [2 D^2 + 3 D + 1]: out, the input of cmps_set_params_dev.   losses_dev [2]: out, mean_b loss_b and the total loss
 *   of the gradients consumed.   scratch_dev: cmps_apply_step_scratch_bytes(D) bytes, 8-byte aligned.
 * One small kernel on `stream`; nothing is copied to the host.
 */
size_t cmps_apply_step_scratch_bytes(int D);
int cmps_psi_apply_step(cmps_handle_t h, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev,
                        double global_batch, double lr_t, double beta1, double beta2, double epsilon, double h_reg, double r_reg,
                        double c_r, double c_h, int with_reg, float* params_dev, float* losses_dev, void* scratch_dev,
                        void* stream);

/*
 * Replaces: PsiCMPS._build_loss_psi (model.py:257-267) = tf.foldl of _psi_and_loss_update
 * (model.py:276-282) over the T-1 increments, i.e. _update_ancilla_psi (:300-317), _inc_loss_psi
 * (:293-294), _expectation (:319-325), _normalize_psi (:327-334) per step.
 * audio_dev [B*T] row-major float32 clips (the `data_iterator` tensor);  loss_dev [B] receives the
 * per-clip loss (the fold carry); PsiCMPS.loss is its mean (model.py:267).
 * save_for_bwd != 0 stashes the per-step state in the workspace (needs CMPS_WS_TRAIN): un-normalised, or -- in the form the two-wave
 * reverse scan reads -- normalised; which one is chosen from the handle's options at THIS call and recorded with the saved forward
 * (CMPS_OPT_BWD_WAVES, CMPS_OPT_SAVED_ROWS).  cmps_psi_loss_bwd and cmps_psi_states follow the record.
 */
int cmps_psi_loss_fwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* loss_dev,
                      int save_for_bwd, void* stream);

/*
 * Replaces: the reverse while-loop that tf.train.AdamOptimizer.minimize builds (train.py:89,
 * training_estimators.py:68) for d(sum_b loss_b)/d(effective parameters).
 * Must follow cmps_psi_loss_fwd(..., save_for_bwd=1) on the same audio, B, T and stream.
 * grad_dev [2*D*D + 3*D + 2] receives SUMS over the B clips (divide by the global batch for the mean):
 *   dR_re [D*D], dR_im [D*D] (row-major, dL/dRe R[i][j], dL/dIm R[i][j]), dfreqs [D],
 *   dpsi0_re [D], dpsi0_im [D], dA, sum_b loss_b.
 */
int cmps_psi_loss_bwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* grad_dev,
                      void* stream);

/*
 * Run-time check of the split-operand arithmetic (no reference counterpart: the reference has one float32 arithmetic).
 * cmps_psi_loss_bwd leaves two flag words in the workspace: bit 0 = a gradient sum is Inf / NaN, bit 1 = the loss sum is.
 * This call waits for `stream`, reads them and returns
 *   CMPS_OK             gradient finite, or loss and gradient both non-finite (that propagates, as in the reference);
 *   CMPS_ERR_F16_RANGE  gradient non-finite although the loss is finite: with an F16X2 arithmetic in force an operand piece
 *                       overflowed fp16 (a violated scale bound).  Documented fallback: set CMPS_OPT_RANK1 = BF16X3 and
 *                       CMPS_OPT_WIDE_CHAIN = VALU and repeat cmps_psi_loss_fwd / _bwd (audio_mps_amd.scan.HipScan does so).
 * *sticky_out (may be NULL) receives the OR of the flag words of every cmps_psi_loss_bwd since the previous call of this
 * function, for loops that do not check every step; cmps_psi_apply_step given `status_dev` skips the update of such a step.
 */
int cmps_psi_grad_status(cmps_handle_t h, int* sticky_out, void* stream);

/*
 * ---- Model bank: M PsiCMPS models of one shape per kernel launch ----
 * Replaces: the Python loop over models that a sweep of the reference is -- a grid over --hparams (train.py:31) at its own settings
 * minibatch_size = 8, bond_dim = 8 (train.py:41), several seeds of the random initialisation, one model per pitch or instrument
 * (reader.py:9-66).  Every scan here is bound by its serial chain, so M members cost about the time of one.  D, B, T, sigma, delta_t,
 * Adam's betas and epsilon and with_reg are common to a bank; the variables, learning_rate, h_reg, r_reg (with c_r, c_h) and the data
 * are free per member.  Member m computes, bit for bit, what the plain entry computes for model m alone: the kernels are the plain
 * ones with a second grid dimension, each member working in its own workspace.
 *
 * Kernel families: D <= 16, 17 <= D <= 32 with the default options under CMPS_VARIANT_AUTO / WAVE, and CMPS_VARIANT_BLOCK at every D.
 * Errors of every cmps_bank_* entry that launches scans: CMPS_ERR_UNSUPPORTED_D for D > 32 without CMPS_VARIANT_BLOCK (a bank above
 * D = 32 needs CMPS_VARIANT_BLOCK); CMPS_ERR_STATE in legacy mode or with a non-default CMPS_OPT_RANK1, CMPS_OPT_BWD_WAVES or
 * CMPS_OPT_F16_SCALE_SHIFT; CMPS_ERR_BAD_ARG (the message starts with the entry's name) for null pointers, M outside [1, 1024],
 * B < 1, T < 2, M B T beyond 2^31 - 1, n_audio not in {1, M}; CMPS_ERR_WORKSPACE for a workspace smaller than
 * cmps_bank_workspace_bytes.  All of them are returned before the device is touched.  Every entry is asynchronous on `stream`, never
 * synchronises (cmps_bank_grad_status excepted, like cmps_psi_grad_status), allocates nothing and touches nothing outside the
 * stated extents.
 *
 * cmps_bank_workspace_bytes = M * cmps_workspace_bytes(D, B, T, flags): member m's workspace is the plain layout at byte m * that.
 */
size_t cmps_bank_workspace_bytes(int D, int M, int B, int T, int flags);

/*
 * Mirrors cmps_set_params_dev for M members: params_dev [M][2 D^2 + 3 D + 1], the buffer cmps_bank_apply_step writes; member m's A is
 * read from its row by the scan kernels.  Every member gets its own tables (the time table is built M times in parallel);
 * CMPS_WS_REUSE_TABLES as in cmps_set_params.  Puts the handle into bank mode; a plain cmps_set_params* puts it back.  In bank mode
 * the plain entries that read the tables of ONE model -- cmps_psi_loss_fwd / _bwd, cmps_psi_grad_status, cmps_psi_states,
 * cmps_psi_update_ancilla, cmps_psi_sample*, cmps_psi_stream*, cmps_rho_set_state, cmps_rho_update_ancilla -- return CMPS_ERR_STATE.
 * Sampling, following and scoring with every member at once are cmps_bank_stream / cmps_bank_stream_score below (a plain or a primed
 * sample of a bank is a stream from k0 = 0); the state read-outs and the ancilla updates need a member taken out as a plain model.
 */
int cmps_bank_set_params_dev(cmps_handle_t h, int M, const float* params_dev, double sigma, double delta_t, int T, int B_max, int flags,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/*
 * Mirror cmps_psi_loss_fwd / cmps_psi_loss_bwd.  audio_dev [n_audio][B][T]: n_audio = 1 is one batch shared by every member (a sweep
 * over seeds or hyper-parameters, train.py:31), n_audio = M one batch per member (a model per pitch, reader.py:9-66).
 * loss_dev [M][B], grad_dev [M][2 D^2 + 3 D + 2].  The saved-forward record of the handle is one record for the whole bank:
 * cmps_bank_loss_bwd without a matching cmps_bank_loss_fwd(save_for_bwd = 1) of the same audio, n_audio, B, T is CMPS_ERR_STATE, and
 * so is a plain cmps_psi_loss_bwd after a bank forward or a bank reverse pass after a plain forward.
 */
int cmps_bank_loss_fwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* loss_dev, int save_for_bwd, void* stream);
int cmps_bank_loss_bwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* grad_dev, void* stream);

/*
 * cmps_bank_loss_bwd with a cotangent per clip and member: member m's grad_dev row is the gradient of sum_b w[m][b] loss[m][b] with
 * w[m][b] = weight_dev[m * ldw + b] (ldw >= B; the output of cmps_bank_classify_weights, or any float32 values), and its last element
 * is that weighted sum itself.  Every family a bank may use writes one gradient slab per clip and member, linear in the cotangent of
 * that clip's loss, and so are the closing terms: the reverse scan is cmps_bank_loss_bwd's, kernel for kernel, and only the cross-clip
 * reduction and the loss sum differ.  They accumulate (double)w * (double)value -- a product of two float32 values is exact in
 * double -- in the plain reduction's fixed order (groups of clips, then the groups).  A clip whose weight is exactly 0 (either sign) is
 * not read at all, neither its slab nor its loss: a diverged clip, or a member absent for a clip, cannot reach the sums or the words of
 * cmps_bank_grad_status.  Weights of all 1.0f give cmps_bank_loss_bwd's grad_dev bit for bit.
 * Preconditions, errors and the saved-forward record are cmps_bank_loss_bwd's; in addition a null weight_dev or ldw < B is
 * CMPS_ERR_BAD_ARG (these two are checked first, on any handle), and a RhoCMPS bank is refused with CMPS_ERR_STATE and a message: its
 * reverse pass runs `rank` virtual clips per clip and closes with kernels of its own.  Reads weight_dev[m * ldw + b], m < M, b < B only.
 */
int cmps_bank_loss_bwd_weighted(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, const float* weight_dev, long long ldw,
                                float* grad_dev, void* stream);

/*
 * Mirrors cmps_psi_apply_step (train.py:55-60, 88-89), one workgroup per member.  vars_dev, adam_m_dev, adam_v_dev, params_dev
 * [M][2 D^2 + 3 D + 1]; grad_sums_dev [M][2 D^2 + 3 D + 2] or NULL (only params_dev is computed); losses_dev [M][2];
 * scratch_dev cmps_bank_apply_step_scratch_bytes(D, M) = M * cmps_apply_step_scratch_bytes(D) bytes, 8-byte aligned.
 * hyper_dev [M][5] doubles on the device, 8-byte aligned: learning_rate, h_reg, r_reg, c_r, c_h of every member.  The device forms
 * lr_t = (learning_rate * bias_num) / bias_den in double with bias_num = sqrt(1 - beta2^t), bias_den = 1 - beta1^t -- the value a
 * host computes for cmps_psi_apply_step, to the bit -- so hyper_dev is uploaded once per run.  The skipped step (a non-finite gradient
 * next to a finite loss) is per member: that member's variables and Adam slots stay as they are, its losses_dev[1] is NaN.
 */
size_t cmps_bank_apply_step_scratch_bytes(int D, int M);
int cmps_bank_apply_step(cmps_handle_t h, int M, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev,
                         double global_batch, double bias_num, double bias_den, double beta1, double beta2, double epsilon,
                         const double* hyper_dev, int with_reg, float* params_dev, float* losses_dev, void* scratch_dev, void* stream);

/*
 * Mirrors cmps_psi_grad_status per member: codes_out [M] receives CMPS_OK or CMPS_ERR_F16_RANGE, sticky_out [M] (may be NULL) the OR
 * of every member's flag words since the previous call.  Waits for `stream`.  Returns CMPS_OK when the words were read.
 */
int cmps_bank_grad_status(cmps_handle_t h, int* codes_out, int* sticky_out, void* stream);

/*
 * ---- Model bank: stream, sample and score with M PsiCMPS models per launch ----
 * Replaces: the Python loop over a trained bank's members that listening to a sweep (the samples of every member, as the reference's
 * summaries give them for one model: model.sample(3, sample_duration), train.py:82-85) or classifying with one model per pitch or
 * instrument (reader.py:9-66: follow one signal with all M, compare the per-sample surprise) is.  The samplers are bound by their
 * serial chain as the training scans are, and n = 3 paths of one model are three wavefronts.
 *
 * cmps_bank_stream / cmps_bank_stream_score are cmps_psi_stream / cmps_psi_stream_score (below: every convention of the segment, the
 * one-sample overlap of the audio, the state rule, the exact cut, the running loss) with the members as a second grid dimension of
 * the same kernels: member m runs n paths on its own tables, and the caller's arrays are indexed by the global path g = m * n + b.
 *   out_dev, noise_dev (n_noise == M * n)   [M][n][length]
 *   pred_dev, nll_dev                       [M][n][forced]
 *   loss_dev                                [M][n]
 *   state_in_dev, state_out_dev             [M][n] records: cmps_bank_stream_state_bytes(h, n) = M * n records of the handle's sampler
 *                                           family (0 for a null handle, n < 1, and outside PsiCMPS bank mode)
 *   audio_dev                               [n_audio][forced + 1], n_audio in {1, n, M * n}: one signal for every path of every member
 *                                           (the classifier), one per path shared by the members, or one per member and path
 *   noise_dev                               [n_noise][length], n_noise in {n, M * n}: every member hears the same noise -- what differs
 *                                           between two members' samples is then the model and not the draw -- or every global path
 *                                           its own (n_noise is not looked at when length == 0)
 * The promise: member m's slices of out, pred, nll, loss and the state records hold, bit for bit, what cmps_psi_stream /
 * cmps_psi_stream_score give on a plain handle set to model m (cmps_set_params_dev on row m of params_dev) with the same T, fed member
 * m's audio and noise rows.  A cut changes no bit, as for the plain stream.
 * The handle must be in PsiCMPS bank mode (after cmps_bank_set_params_dev), otherwise CMPS_ERR_STATE: plain mode, legacy mode, a
 * RhoCMPS bank, before any set_params.  The kernel families are the bank's: k_sample_wave for D <= 32 under CMPS_VARIANT_AUTO / WAVE,
 * k_sample_block under CMPS_VARIANT_BLOCK at every D <= 128 (cmps_bank_*'s own mode errors apply).
 * CMPS_ERR_BAD_ARG: n_audio not in {1, n, M * n}; n_noise not in {n, M * n} when length > 0; M * n * (forced + length) beyond 2^31 - 1;
 * and everything the plain entries refuse (state_in_dev NULL <=> k0 == 0, the table rows with a message naming the needed T, null
 * pointers, the counts).  Every message starts with the entry's name and is returned before the device is touched.
 * Asynchronous on `stream`; never synchronises, allocates nothing, touches nothing outside the stated extents.  With
 * CMPS_OPT_KERNEL_EVENTS the launch is recorded under the plain entries' names: k_sample_wave_stream, k_sample_wave_score,
 * k_sample_block_stream, k_sample_block_score.
 */
size_t cmps_bank_stream_state_bytes(cmps_handle_t h, int n);
int cmps_bank_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                     const float* audio_dev, int n_audio, int forced,
                     const float* noise_dev, int n_noise, int length,
                     int n, float* out_dev, float* pred_dev, void* stream);
int cmps_bank_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                           const float* audio_dev, int n_audio, int forced, int n,
                           float* nll_dev, float* loss_dev, float* pred_dev, void* stream);

/*
 * Replaces: PsiCMPS._update_ancilla_psi (model.py:300-317), one step in the lab frame.
 * psi_in_dev / psi_out_dev [B*D*2] interleaved (re, im); signal_dev [B]; t = time of the step.
 */
int cmps_psi_update_ancilla(cmps_handle_t h, const float* psi_in_dev, const float* signal_dev,
                            float t, int B, float* psi_out_dev, void* stream);

/*
 * Replaces: PsiCMPS.psi_evolve_with_data (model.py:231-240): the normalised lab-frame state after
 * every step, psi_out_dev [B*(T-1)*D*2] interleaved (re, im), reconstructed from the stash written by
 * cmps_psi_loss_fwd(..., save_for_bwd=1).
 * In legacy mode (after cmps_legacy_set_params) it returns CMPS_ERR_STATE: the lab-frame phases need the time table, which that mode does not have.
 */
int cmps_psi_states(cmps_handle_t h, int B, int T, float* psi_out_dev, void* stream);

/*
 * Replaces: PsiCMPS.sample's tf.scan of _psi_and_sample_update (model.py:242-251, 284-291) for pre-drawn noise
 * (the reference draws it with tf.random_normal([length, n], stddev = sigma * sqrt(temp * delta_t)), model.py:246).
 * noise_dev [n * length] row-major [path][step] (transposed w.r.t. the reference so that a path reads contiguous
 * memory); out_dev [n * length] receives A * (running sum of the increments), i.e. `self.A * transpose(samples)`.
 * Needs cmps_set_params with T >= length + 1 (the per-step time/phase tables); any workspace flags.
 */
int cmps_psi_sample(cmps_handle_t h, const float* noise_dev, int n, int length, float* out_dev, void* stream);

/*
 * PsiCMPS.sample (model.py:242-251) continued from a clip: P = prime_T - 1 teacher-forced steps of _psi_update
 * (model.py:269-274) on the increments of prime_dev, then `length` steps of _psi_and_sample_update (:284-291).
 * The reference has no such method (its sample.py is an empty stub); both halves are its own steps, run as ONE scan over the
 * steps k = 0 .. P + length - 1 on table row k, so the time grid t_k and the rotating frame run through the hand-over unbroken.
 *   forced step, k < P:   increment = prime[b'][k + 1] - prime[b'][k] in float32 (the subtraction of model.py:263), b' = b, or 0 when
 *                         one clip is shared;  the running sum stays 0;  pred[b][k] = 2 Re<psi|R|psi> * delta_t on the normalised
 *                         state at t_k, BEFORE the step sees the data: the model's expected increment, the expression the sampler
 *                         adds its noise to at model.py:286.
 *   sampled step, k >= P: exactly the step of cmps_psi_sample with noise[b][k - P];  out[b][k - P] = A * (running sum of the
 *                         sampled increments, starting from zero at k = P).
 * So out_dev is what cmps_psi_sample would return had it started from the primed state at t_P; in the clip's own units the
 * continuation is prime[b'][prime_T - 1] + out[b][:] / A.
 * prime_dev [n_prime * prime_T] row-major clips, n_prime == n, or n_prime == 1 for one clip shared by every path; prime_T >= 2.
 * noise_dev [n * length], out_dev [n * length] as in cmps_psi_sample; pred_dev [n * (prime_T - 1)] row-major [path][step], or NULL.
 * Needs cmps_set_params* with T >= prime_T + length (one row of the per-step tables per step, forced or sampled), otherwise
 * CMPS_ERR_BAD_ARG with a message naming the needed T; null pointers, n < 1, length < 1, prime_T < 2 and n_prime not in {1, n} are
 * CMPS_ERR_BAD_ARG; before cmps_set_params and in legacy mode CMPS_ERR_STATE.  The kernel is chosen exactly as in cmps_psi_sample.
 */
int cmps_psi_sample_primed(cmps_handle_t h, const float* prime_dev, int n_prime, int prime_T,
                           const float* noise_dev, int n, int length,
                           float* out_dev, float* pred_dev, void* stream);

/*
 * One segment of a resumable PsiCMPS.sample scan: `forced` steps of _psi_update (model.py:269-274) on the increments of audio_dev, then
 * `length` steps of _psi_and_sample_update (:284-291), on table rows k0 .. k0 + forced + length - 1.  Either count may be 0, not both.
 * The reference has no such method; the steps are cmps_psi_sample_primed's, and what a sampler kernel carries from one step into the
 * next leaves the kernel between two calls, so a scan can be carried on (another second behind what was generated, the next block of an
 * incoming signal), can alternate between following and generating (filling a gap), and can follow only (length == 0).
 *   forced step j < forced:  increment = audio[b'][j + 1] - audio[b'][j] in float32 (model.py:263), b' = b, or 0 when one signal is
 *                            shared;  the running sum is reset to 0;  pred[b][j] = 2 Re<psi|R|psi> * delta_t before the step.
 *   sampled step j >= forced: increment = expectation * delta_t + noise[b][j - forced];  the running sum continues (from state_in_dev's,
 *                            0 at the start of a stream or behind a forced step);  out[b][j - forced] = A * running sum.
 * audio_dev [n_audio * (forced + 1)] row-major, n_audio == n, or 1: shared.  audio_dev[b'][0] is the sample BEFORE the segment's first
 * forced step: consecutive blocks of a signal overlap by one sample, so the subtraction of model.py:263 happens here as everywhere else.
 * noise_dev [n * length], out_dev [n * length] row-major [path][step]; pred_dev [n * forced] or NULL.
 * State: cmps_psi_stream_state_bytes(h, n) bytes of caller-owned device memory, n records (a multiple of 16 bytes; 0 for a null handle
 * or n < 1).  A record is opaque and belongs to the handle's D and to the sampler kernel its variant resolves to (as cmps_psi_sample
 * chooses it); it holds the carried values themselves, which makes a cut exact: a scan run as one call or in any number of segments
 * gives the same bits in out, pred and the final record.  (The carried values fill a record from its first byte; the up to 12 bytes
 * that round it up to a multiple of 16 are never written and keep what the caller's memory held.  The same holds for cmps_rho_stream.)
 *   state_in_dev == NULL  <=>  k0 == 0: the start of a stream (psi_0, running sum 0); anything else is CMPS_ERR_BAD_ARG.
 *   state_out_dev may be NULL (the last segment) and may equal state_in_dev (a path reads its record before it writes it).
 * Parameters, T, variant and n are the caller's to keep fixed over a stream.  The exact split holds for tables built by equal
 * cmps_set_params* calls; calling it again with the same arguments between two segments is allowed and changes nothing.  A different T
 * moves the drift-corrected last row of the final 64-step chunk of the phase table, i.e. rounding only.
 * CMPS_ERR_BAD_ARG: n < 1, forced < 0, length < 0, forced + length < 1, k0 < 0; audio_dev == NULL with forced > 0; noise_dev or out_dev
 * == NULL with length > 0; n_audio not in {1, n}; k0 + forced + length > T - 1 of cmps_set_params*, with a message naming the needed
 * T >= k0 + forced + length + 1.  CMPS_ERR_STATE before cmps_set_params and in legacy mode.
 * Asynchronous on `stream`; never synchronises, allocates nothing.  With CMPS_OPT_KERNEL_EVENTS the launch is recorded as
 * k_sample_wave_stream, k_sample_wide_stream or k_sample_block_stream.
 */
size_t cmps_psi_stream_state_bytes(cmps_handle_t h, int n);
int cmps_psi_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                    const float* audio_dev, int n_audio, int forced,
                    const float* noise_dev, int length,
                    int n, float* out_dev, float* pred_dev, void* stream);

/*
 * One scored segment of a resumable scan: `forced` steps of cmps_psi_stream (forced steps only, same conventions: audio_dev
 * [n_audio, forced + 1] with the one-sample overlap, n_audio in {1, n}, state_in_dev == NULL <=> k0 == 0, state_out_dev NULL or equal to
 * state_in_dev, table rows k0 .. k0 + forced - 1) that also give the loss increment of every step (model.py:276-282, 293-294):
 *   step j:  y_j = u + Q u + s R u on the normalised state u, s = x_j / A, x_j = audio[b'][j + 1] - audio[b'][j]  (the followed step);
 *            e'  = 2 Re(y_j^dagger R y_j) in float32 on the updated, UN-normalised state, still in the frame of t_j;
 *            z   = (e' * x_j) / A;   nll[b][j] = -logf(1.0f + z)   -- the operation order of cmps_psi_loss_fwd (model.py:294);
 *            loss[b] += nll[b][j], sequentially in step order in float32 (model.py:279).
 * pred_dev[b][j] holds 2 Re<u|R|u> * delta_t on the state BEFORE the step; the increment needs its own product R y_j (another state,
 * another frame than the next step's rho_j y_j), which is what this entry adds to a followed step.  Nothing of it feeds the chain:
 * pred and the state record carry the bits cmps_psi_stream gives on the same steps, the record is the one
 * cmps_psi_stream_state_bytes describes, and a stream may alternate between this entry and cmps_psi_stream freely.
 * nll_dev [n * forced] row-major [path][step], or NULL.  loss_dev [n], required: the running loss lives with the caller, not in the
 * record.  At the start of a stream (state_in_dev == NULL) it is not read and is written from 0; otherwise it is loaded once, continued,
 * and stored once behind the last step.  Cut anywhere, nll, loss, pred and the final record keep their bits; over a whole clip from
 * k0 = 0 loss is the clip's cmps_psi_loss_fwd to rounding.  Where 1 + z <= 0 the NaN / Inf of the logarithm propagates into nll and
 * loss, as in the loss entries.
 * CMPS_ERR_BAD_ARG: cmps_psi_stream's (with length = 0), and forced < 1 or loss_dev == NULL; k0 + forced > T - 1 with a message naming
 * the needed T >= k0 + forced + 1.  CMPS_ERR_STATE before cmps_set_params* and in legacy mode.
 * Asynchronous on `stream`; never synchronises, allocates nothing.  The kernel is chosen as cmps_psi_sample chooses it; with
 * CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_sample_wave_score, k_sample_wide_score or k_sample_block_score.
 */
int cmps_psi_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                          const float* audio_dev, int n_audio, int forced, int n,
                          float* nll_dev, float* loss_dev, float* pred_dev, void* stream);

/*
 * Legacy `AudioMPS` arithmetic (the model training_estimators.py:43-45 was written for; its class body is gone from
 * model.py, its training graph survives in logging/graph.pbtxt: psi_0 = e_0, loss += (x - 2 Re<psi|R|psi>)^2 / 2 before
 * the update, psi' = psi + Q psi + dt x R psi, Q = dt (-i H_s - R^T R / 2), graph.pbtxt:10585-14847).
 * R_dev [D*D] real row-major; Q_re_dev, Q_im_dev [D*D] (Q is built by the caller from H and R).
 * cmps_legacy_loss_fwd / _bwd mirror cmps_psi_loss_fwd / _bwd; grad_dev [3*D*D + 1] receives sums over clips of
 *   dQ_re [D*D], dQ_im [D*D], dR (the direct real-R part) [D*D], sum_b loss_b.
 * D <= 32 runs on the wavefront-per-clip kernels of the pure-state path in their legacy mode (same rank-1 arithmetic option,
 * CMPS_OPT_RANK1); 32 < D <= 128 on the wide kernels in their legacy mode (fp32 VALU chains; the H y and gradient GEMMs with two fp16
 * pieces for CMPS_RANK1_F16X2 / DEFAULT, three bf16 pieces otherwise); CMPS_VARIANT_BLOCK runs the general one-workgroup-per-clip
 * kernels at every D (the cross-check implementation).
 */
int cmps_legacy_set_params(cmps_handle_t h, const float* R_dev, const float* Q_re_dev, const float* Q_im_dev,
                           double delta_t, int T, int B_max, int flags, void* workspace_dev, size_t workspace_bytes,
                           void* stream);
int cmps_legacy_loss_fwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* loss_dev, int save_for_bwd,
                         void* stream);
int cmps_legacy_loss_bwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* grad_dev, void* stream);

/*
 * RhoCMPS: the density-matrix scan (model.py:55-203).  All entries need cmps_set_params first (R, freqs, A, sigma,
 * delta_t and the per-step tables are shared with the pure-state path; its psi_0 arguments are ignored here).
 *
 * The reference's rho_0 = W^dagger W / trace (model.py:127-132) has rank `rank` = hparams.initial_rank (default D), and
 * rho -> U rho U^dagger / trace keeps it, so the state is handed over and carried as its `rank` columns:
 *   phi_re_dev, phi_im_dev [rank*D] row-major [a][d],  rho_0 = sum_a phi_a phi_a^dagger,  phi_a = conj(W[a, :]) / sqrt(tr).
 *
 * cmps_rho_workspace_bytes / cmps_rho_set_state: a second caller-owned, 256-B aligned workspace for the columns, their
 *   per-step stash (CMPS_WS_TRAIN: B_max * (T-1) * rank * D' * 8 bytes) and the reduction buffers.  Replaces `_rho_init`
 *   (model.py:119-132) + `tf.stack(batch_size * [self.rho_0])` (:136).  Any rank <= 128 (the reference's default is rank = D,
 *   model.py:62-65): up to rank * D = 5000 the general kernels keep their column arrays in LDS, above that in this workspace
 *   (B_max * 4 * rank * D * 8 more bytes; cmps_rho_sample then needs n <= B_max).
 * cmps_rho_loss_fwd: RhoCMPS._build_loss_rho (model.py:133-144) = tf.foldl of _rho_and_loss_update (:152-158):
 *   _update_ancilla_rho (:172-187), _inc_loss_rho (:166), _expectation (:189-196), _normalize_rho (:198-203).
 *   loss_dev [B] per-clip loss; the caller takes the mean (:144).
 * cmps_rho_loss_bwd: the reverse while-loop TF autodiff builds for that fold.  grad_dev [2*D*D + 3*D + 2 + 2*rank*D]
 *   receives sums over clips:  the cmps_psi_loss_bwd layout (dR_re, dR_im, dfreqs, 2*D unused zeros, dA, sum_b loss_b)
 *   followed by dphi_re [rank*D], dphi_im [rank*D] (cotangents of the columns phi_a).
 * cmps_rho_update_ancilla: RhoCMPS._update_ancilla_rho (model.py:172-187) for arbitrary rho_in_dev [B*D*D*2]
 *   (row-major, interleaved re/im), signal_dev [B], time t; rho_out_dev like rho_in_dev.  Needs no cmps_rho_set_state.
 * cmps_rho_sample: RhoCMPS.sample / rho_evolve_with_sampling / purity (model.py:86-116): tf.scan of
 *   _rho_and_sample_update (:160-167) for pre-drawn noise_dev [n*length] ([path][step]); out_dev [n*length] = A * running
 *   sum.  save_states != 0 keeps the columns of every step (needs a CMPS_WS_TRAIN rho workspace sized for B_max >= n,
 *   T >= length + 1) for cmps_rho_states.  Kernel selection follows cmps_set_variant like the loss entries: D <= 32 and
 *   rank <= 32 run the row-array GEMM kernels (one wavefront per clip / path), CMPS_VARIANT_BLOCK the general ones.
 * cmps_rho_states: lab-frame normalised rho after every step of the last cmps_rho_loss_fwd(save_for_bwd=1) or
 *   cmps_rho_sample / cmps_rho_sample_primed / cmps_rho_stream(save_states=1): rho_out_dev [B*steps*D*D*2] (rho_evolve_with_data, model.py:76-84 /
 *   rho_evolve_with_sampling, :86-92) and/or purity_out_dev [B*steps] = tr rho^2 (:94-101); either may be NULL.
 */
size_t cmps_rho_workspace_bytes(int D, int rank, int B, int T, int flags);
int cmps_rho_set_state(cmps_handle_t h, const float* phi_re_dev, const float* phi_im_dev, int rank, int T, int B_max,
                       int flags, void* rho_workspace_dev, size_t rho_workspace_bytes, void* stream);
int cmps_rho_loss_fwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* loss_dev, int save_for_bwd,
                      void* stream);
int cmps_rho_loss_bwd(cmps_handle_t h, const float* audio_dev, int B, int T, float* grad_dev, void* stream);
int cmps_rho_update_ancilla(cmps_handle_t h, const float* rho_in_dev, const float* signal_dev, float t, int B,
                            float* rho_out_dev, void* stream);
int cmps_rho_sample(cmps_handle_t h, const float* noise_dev, int n, int length, float* out_dev, int save_states,
                    void* stream);
int cmps_rho_states(cmps_handle_t h, int B, int steps, float* rho_out_dev, float* purity_out_dev, void* stream);

/*
 * RhoCMPS.sample (model.py:103-116) continued from a clip: cmps_psi_sample_primed for the density-matrix model, with the same
 * conventions.  P = prime_T - 1 teacher-forced steps of _rho_update (model.py:144-150) on the increments of prime_dev, then `length`
 * steps of _rho_and_sample_update (:160-167), as ONE scan over the steps k = 0 .. P + length - 1 on table row k from the `rank` columns
 * of cmps_rho_set_state, so the time grid t_k and the rotating frame run through the hand-over unbroken.
 *   forced step, k < P:   increment = prime[b'][k + 1] - prime[b'][k] in float32 (the subtraction of model.py:138), b' = b, or 0 when
 *                         one clip is shared;  the running sum stays 0;  pred[b][k] = Re tr((Rt + Rt^dagger) rho) * delta_t on the
 *                         normalised state at t_k, BEFORE the step sees the data: the expression the sampler adds its noise to at
 *                         model.py:162;  the update is the sampler's own with the given increment.
 *   sampled step, k >= P: exactly the step of cmps_rho_sample with noise[b][k - P];  out[b][k - P] = A * (running sum of the
 *                         sampled increments, starting from zero at k = P).
 * prime_dev [n_prime * prime_T] row-major clips, n_prime == n, or n_prime == 1 for one clip shared by every path; prime_T >= 2.
 * noise_dev [n * length], out_dev [n * length] as in cmps_rho_sample; pred_dev [n * (prime_T - 1)] row-major [path][step], or NULL.
 * save_states != 0 keeps the columns of ALL P + length steps, forced ones first (needs a CMPS_WS_TRAIN rho workspace with
 * B_max * (T - 1) >= n * (P + length)): cmps_rho_states(h, n, P + length, ...) then returns rho and purity across the hand-over.
 * Needs cmps_set_params* with T >= prime_T + length (one row of the per-step tables per step, forced or sampled), otherwise
 * CMPS_ERR_BAD_ARG with a message naming the needed T; null prime_dev / noise_dev / out_dev, n < 1, length < 1, prime_T < 2 and
 * n_prime not in {1, n} are CMPS_ERR_BAD_ARG; before cmps_set_params or cmps_rho_set_state and in legacy mode CMPS_ERR_STATE;
 * CMPS_ERR_WORKSPACE as for cmps_rho_sample (columns in the workspace and n > B_max; save_states without the rows for it).
 * The kernel is chosen exactly as in cmps_rho_sample; with CMPS_OPT_KERNEL_EVENTS its time is recorded as k_sample_rho_mfma_primed /
 * k_sample_rho_primed.
 */
int cmps_rho_sample_primed(cmps_handle_t h, const float* prime_dev, int n_prime, int prime_T,
                           const float* noise_dev, int n, int length,
                           float* out_dev, float* pred_dev, int save_states, void* stream);

/*
 * One segment of a resumable RhoCMPS.sample scan: cmps_psi_stream for the density-matrix model, with the same step conventions.  `forced`
 * steps of _rho_update (model.py:144-150) on the increments of audio_dev, then `length` steps of _rho_and_sample_update (:160-167), on table
 * rows k0 .. k0 + forced + length - 1.  Either count may be 0, not both.  The steps are cmps_rho_sample_primed's (pred[b][j] =
 * Re tr((Rt + Rt^dagger) rho) * delta_t before forced step j; a forced step resets the running sum to 0, a sampled step continues it from
 * state_in_dev's), and what the sampler kernel carries from one step into the next leaves the kernel between two calls.
 * audio_dev [n_audio * (forced + 1)] row-major, n_audio == n, or 1: shared; audio_dev[b'][0] is the sample BEFORE the segment's first forced
 * step (consecutive blocks overlap by one sample).  noise_dev [n * length], out_dev [n * length] row-major [path][step] of the SEGMENT;
 * pred_dev [n * forced] or NULL.
 * State: cmps_rho_stream_state_bytes(h, n) bytes of caller-owned device memory, n records (a multiple of 16 bytes; 0 for a null handle,
 * n < 1 or before cmps_rho_set_state).  A record is opaque and belongs to the handle's D, to the rank of cmps_rho_set_state and to the
 * sampler kernel the variant resolves to (as cmps_rho_sample chooses it): the float32 rows of the row-array kernel (256 rank + 16 bytes),
 * or the columns of the block kernel (8 rank D + 4 bytes, rounded up to 16), and the running sum.  It holds the carried values themselves,
 * which makes a cut exact: a scan run as one call or in any number of segments gives the same bits in out, pred, the saved columns and
 * the final record.
 *   state_in_dev == NULL  <=>  k0 == 0: the start of a stream (the columns of cmps_rho_set_state, running sum 0); anything else is
 *   CMPS_ERR_BAD_ARG.  state_out_dev may be NULL (the last segment) and may equal state_in_dev (a path reads its record before it
 *   writes it).
 * save_states != 0 keeps the columns of THIS segment's forced + length steps in stash rows 0 ..: needs a CMPS_WS_TRAIN rho workspace with
 * B_max * (T_rho - 1) >= n * (forced + length), B_max and T_rho those of cmps_rho_set_state -- whose T is independent of cmps_set_params'
 * (it must not exceed it) and is only a stash capacity: a long run needs rows for one segment, not for the run.
 * cmps_rho_states(h, n, forced + length, ...) then returns the segment's lab-frame rho and purity, with the phases of t_{k0 + k}.
 * Parameters, T, the columns, variant and n are the caller's to keep fixed over a stream; calling cmps_set_params* and
 * cmps_rho_set_state again with the same arguments between two segments is allowed and changes nothing.
 * CMPS_ERR_BAD_ARG: n < 1, forced < 0, length < 0, forced + length < 1, k0 < 0; audio_dev == NULL with forced > 0; noise_dev or out_dev
 * == NULL with length > 0; n_audio not in {1, n}; k0 + forced + length > T - 1 of cmps_set_params*, with a message naming the needed
 * T >= k0 + forced + length + 1.  CMPS_ERR_STATE before cmps_set_params* or cmps_rho_set_state and in legacy mode.  CMPS_ERR_WORKSPACE
 * as for cmps_rho_sample_primed (columns in the workspace and n > B_max; save_states without the rows for it).
 * Asynchronous on `stream`; never synchronises, allocates nothing.  With CMPS_OPT_KERNEL_EVENTS the launch is recorded as
 * k_sample_rho_mfma_stream or k_sample_rho_stream.
 */
size_t cmps_rho_stream_state_bytes(cmps_handle_t h, int n);
int cmps_rho_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                    const float* audio_dev, int n_audio, int forced,
                    const float* noise_dev, int length,
                    int n, float* out_dev, float* pred_dev, int save_states, void* stream);

/*
 * One scored segment of a resumable RhoCMPS scan: cmps_psi_stream_score for the density-matrix model.  `forced` >= 1 forced steps of
 * cmps_rho_stream (length = 0, same conventions: audio_dev [n_audio, forced + 1] with the one-sample overlap, n_audio in {1, n},
 * state_in_dev == NULL <=> k0 == 0, state_out_dev NULL or equal to state_in_dev, table rows k0 .. k0 + forced - 1, save_states as there)
 * that also give the loss increment of every step (_rho_and_loss_update, model.py:152-158; _inc_loss_rho, :169-170), formed behind the
 * update and before the normalisation:
 *   step j:  y_a = u_a + Q u_a + s R u_a on the columns of the normalised rho, s = x_j / A, x_j = audio[b'][j + 1] - audio[b'][j];
 *            e'  = Re tr((Rt + Rt^dagger) rho') = 2 sum_a Re(y_a^dagger R y_a) in float32 on the UN-normalised columns, in the frame of t_j;
 *            z   = (e' * x_j) / A;   nll[b][j] = -logf(1.0f + z)   -- the operation order of cmps_rho_loss_fwd (model.py:166);
 *            loss[b] += nll[b][j], sequentially in step order in float32 (model.py:155).
 * The reference gives only the batch mean of the whole clip (_build_loss_rho, model.py:132-142); this entry gives every sample's share.
 * Nothing of it feeds the chain: pred, the state record and the saved columns carry the bits cmps_rho_stream gives on the same steps,
 * the record is the one cmps_rho_stream_state_bytes describes, and a stream may alternate between this entry and cmps_rho_stream freely.
 * nll_dev [n * forced] row-major [path][step], or NULL.  loss_dev [n], required: the running loss lives with the caller, not in the
 * record.  At the start of a stream (state_in_dev == NULL) it is not read and is written from 0; otherwise it is loaded once, continued,
 * and stored once behind the last step.  pred_dev [n * forced] or NULL, as in cmps_rho_stream.  Cut anywhere, nll, loss, pred, the final
 * record and the saved columns keep their bits; over a whole clip from k0 = 0 loss is the clip's cmps_rho_loss_fwd to rounding.  Where
 * 1 + z <= 0 the NaN / Inf of the logarithm propagates into nll and loss, as in the loss entries.
 * CMPS_ERR_BAD_ARG: cmps_rho_stream's (with length = 0), and forced < 1 or loss_dev == NULL; k0 + forced > T - 1 with a message naming
 * the needed T >= k0 + forced + 1.  CMPS_ERR_STATE before cmps_set_params* or cmps_rho_set_state and in legacy mode.  CMPS_ERR_WORKSPACE
 * as for cmps_rho_stream.
 * Asynchronous on `stream`; never synchronises, allocates nothing.  The kernel is chosen as cmps_rho_sample chooses it; with
 * CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_sample_rho_mfma_score or k_sample_rho_score.
 */
int cmps_rho_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                          const float* audio_dev, int n_audio, int forced, int n,
                          float* nll_dev, float* loss_dev, float* pred_dev, int save_states, void* stream);

/*
 * Replaces: the optimiser half of a RhoCMPS training step -- tf.train.AdamOptimizer(learning_rate).minimize(total_loss)
 * (train.py:88-89) with the regularisers of train.py:55-60, i.e. the chain rule from the effective parameters and the columns of
 * rho_0 back to the trainable variables (adjoint of model.py:36-42, 49, 119-132), the Adam update, and the next step's effective
 * parameters and columns (model.py:36-42, 49, 119-132).  cmps_psi_apply_step for the density-matrix model: everything not named
 * here (lr_t, c_r, c_h, with_reg, losses_dev, the skipped step) is as described there.
 *   vars_dev, adam_m_dev, adam_v_dev [2 D^2 + D + 1 + 2 rank D]: A | Rx [D*D] | Ry [D*D] | freqs [D] | Wx [rank*D] | Wy [rank*D]
 *     (in / out; W row-major [a][d] as the reference's variables, model.py:121-127)
 *   grad_sums_dev [2 D^2 + 3 D + 2 + 2 rank D]: the buffer of cmps_rho_loss_bwd, summed over all ranks (its two unused psi_0 blocks
 *     are not read).  NULL: no update -- only params_dev and phi_dev are computed from vars_dev (the first step).
 *     A non-finite entry in its gradient part (the column cotangents included) next to a finite loss sum skips the update:
 *     variables and Adam slots stay as they are, losses_dev[1] = NaN, params_dev / phi_dev are written from the unchanged variables.
 *   params_dev [2 D^2 + 3 D + 1]: out, the input of cmps_set_params_dev; its psi_0 slot is written as e_0 (unused on this path).
 *   phi_dev [2 rank D]: out, phi_re [rank*D] | phi_im [rank*D], phi_a = conj(W[a, :]) / sqrt(tr W^dagger W): the two pointers
 *     cmps_rho_set_state takes.  There is no floor on the trace (the reference has none, model.py:130).
 *   scratch_dev: cmps_rho_apply_step_scratch_bytes(D, rank) bytes (0 for D or rank outside [1, 128]), 8-byte aligned.
 * One small kernel on `stream`; nothing is copied to the host.
 */
size_t cmps_rho_apply_step_scratch_bytes(int D, int rank);
int cmps_rho_apply_step(cmps_handle_t h, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev,
                        int rank, double global_batch, double lr_t, double beta1, double beta2, double epsilon, double h_reg,
                        double r_reg, double c_r, double c_h, int with_reg, float* params_dev, float* phi_dev, float* losses_dev,
                        void* scratch_dev, void* stream);

/*
 * ---- Model bank: M RhoCMPS models of one shape per kernel launch ----
 * Replaces: the Python loop over models of a sweep with --mps_model rho_mps -- the reference offers psi_mps and rho_mps side by side
 * (train.py:18-20, 50-53) at minibatch_size = 8, bond_dim = 8 (train.py:41), where one RhoCMPS model (model.py:55-203) occupies 8 of
 * the 1024 SIMDs in its forward and is bound by its serial chain whatever the rank.  As for the PsiCMPS bank (cmps_bank_* above): D,
 * rank, B, T, sigma, delta_t, Adam's betas and epsilon and with_reg are common to a bank; the variables, learning_rate, h_reg, r_reg
 * (with c_r, c_h) and the data are free per member, and member m computes, bit for bit, what the plain cmps_rho_* entries compute for
 * model m alone: the kernels are the plain ones with a second grid dimension.
 *
 * Scope: D <= 32 and 3 <= rank <= 32 under CMPS_VARIANT_AUTO or CMPS_VARIANT_WAVE with the default CMPS_OPT_RHO_BWD (VIRTUAL),
 * CMPS_OPT_RANK1, CMPS_OPT_BWD_WAVES and CMPS_OPT_F16_SCALE_SHIFT -- the kernel set a plain handle picks there: k_fwd_rho_mfma (forward
 * with save_for_bwd = 0 at rank <= 8: k_fwd_rho_wave), k_bwd_wave2w on B rank virtual clips, the slab reduction, k_finalize and
 * k_rho_phi_from_slabs.  Out of scope and refused: rank <= 2, D > 32 and rank > 32 (the block and wide families), CMPS_VARIANT_BLOCK /
 * WAVE32, k_bwd_rho_mfma (CMPS_OPT_RHO_BWD = GEMM) and every other non-default option.  There are no multi-rank banks and no status
 * words (RhoCMPS has none).  Sampling, following and scoring with every member at once are cmps_rho_bank_stream /
 * cmps_rho_bank_stream_score below; the state read-outs (cmps_rho_states, save_states) need a member taken out as a plain model.
 * Errors, all returned before the device is touched, every message starting with the entry's name: CMPS_ERR_UNSUPPORTED_D for D or rank
 * outside the scope; CMPS_ERR_STATE for another variant or a non-default option (checked at the forward and the reverse call too);
 * CMPS_ERR_BAD_ARG for null pointers, M outside [1, 1024], n_audio not in {1, M}, B < 1, T < 2, M B rank T beyond 2^31 - 1;
 * CMPS_ERR_WORKSPACE for a null, unaligned (256 bytes) or too small workspace.  Every entry is asynchronous on `stream`, allocates
 * nothing and touches nothing outside the stated extents.
 *
 * One workspace, one stride: a RhoCMPS bank does not take a main and a rho workspace but ONE, in which member m's region is the plain
 * main layout (tables only: CMPS_WS_FWD_ONLY) followed by the plain rho layout, at byte m * (their sum).
 * cmps_rho_bank_workspace_bytes = M * (cmps_workspace_bytes(D, B, T, CMPS_WS_FWD_ONLY) + cmps_rho_workspace_bytes(D, rank, B, T, flags));
 * 0 for M outside [1, 1024], D or rank outside the scope, B < 1 or T < 2.
 */
size_t cmps_rho_bank_workspace_bytes(int D, int rank, int M, int B, int T, int flags);

/*
 * cmps_bank_set_params_dev plus cmps_rho_set_state for every member: params_dev [M][2 D^2 + 3 D + 1] and phi_dev [M][2 rank D] (phi_re
 * [rank][D], then phi_im), the buffers cmps_rho_bank_apply_step writes.  flags: CMPS_WS_TRAIN for the rho part, CMPS_WS_REUSE_TABLES as
 * in cmps_bank_set_params_dev.  Puts the handle into the rho-bank mode: every plain one-model entry and the PsiCMPS bank's
 * cmps_bank_loss_fwd / _bwd / _grad_status return CMPS_ERR_STATE, and cmps_rho_bank_loss_* return CMPS_ERR_STATE in every other mode.
 * A plain cmps_set_params* puts the handle back.
 */
int cmps_rho_bank_set_state_dev(cmps_handle_t h, int M, const float* params_dev, const float* phi_dev, int rank, double sigma, double delta_t,
                                int T, int B_max, int flags, void* workspace_dev, size_t workspace_bytes, void* stream);

/*
 * Mirror cmps_rho_loss_fwd / cmps_rho_loss_bwd.  audio_dev [n_audio][B][T] with n_audio = 1 (one batch shared by every member) or M;
 * loss_dev [M][B]; grad_dev [M][2 D^2 + 3 D + 2 + 2 rank D] (the layout of cmps_rho_loss_bwd per member).  One saved-forward record
 * for the whole bank: cmps_rho_bank_loss_bwd without a matching cmps_rho_bank_loss_fwd(save_for_bwd = 1) of the same audio, n_audio,
 * B, T is CMPS_ERR_STATE.
 */
int cmps_rho_bank_loss_fwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* loss_dev, int save_for_bwd, void* stream);
int cmps_rho_bank_loss_bwd(cmps_handle_t h, const float* audio_dev, int n_audio, int B, int T, float* grad_dev, void* stream);

/*
 * Mirrors cmps_rho_apply_step, one workgroup per member (train.py:55-60, 88-89).  vars_dev, adam_m_dev, adam_v_dev
 * [M][1 + 2 D^2 + D + 2 rank D]; params_dev [M][2 D^2 + 3 D + 1]; phi_dev [M][2 rank D]; grad_sums_dev [M][2 D^2 + 3 D + 2 + 2 rank D] or
 * NULL (only params_dev and phi_dev are computed); losses_dev [M][2]; scratch_dev cmps_rho_bank_apply_step_scratch_bytes(D, rank, M) =
 * M * cmps_rho_apply_step_scratch_bytes(D, rank) bytes (0 outside the scope), 8-byte aligned.  hyper_dev [M][5] doubles as in
 * cmps_bank_apply_step; lr_t = (learning_rate * bias_num) / bias_den is formed in double on the device.  The skipped step (a non-finite
 * gradient next to a finite loss) is per member.
 */
size_t cmps_rho_bank_apply_step_scratch_bytes(int D, int rank, int M);
int cmps_rho_bank_apply_step(cmps_handle_t h, int M, float* vars_dev, float* adam_m_dev, float* adam_v_dev, const float* grad_sums_dev, int rank,
                             double global_batch, double bias_num, double bias_den, double beta1, double beta2, double epsilon,
                             const double* hyper_dev, int with_reg, float* params_dev, float* phi_dev, float* losses_dev, void* scratch_dev,
                             void* stream);

/*
 * ---- Model bank: stream, sample and score with M RhoCMPS models per launch ----
 * Replaces: the Python loop of M plain cmps_rho_stream* handles over a trained RhoCMPS bank's members (the samples of every member,
 * model.sample(3, sample_duration), train.py:82-85; one model per class following one signal, reader.py:9-66).  k_sample_rho_mfma puts
 * one path on one wavefront and is bound by its serial chain: n = 3 paths of one model are three wavefronts.
 *
 * cmps_rho_bank_stream / cmps_rho_bank_stream_score are cmps_rho_stream / cmps_rho_stream_score (above: every convention of the segment,
 * the one-sample overlap of the audio, the state rule, the exact cut, the running loss) without save_states, with the members as a
 * second grid dimension of the same kernel; the argument lists and the array shapes are those of cmps_bank_stream / _score:
 *   out_dev, noise_dev (n_noise == M * n)   [M][n][length]
 *   pred_dev, nll_dev                       [M][n][forced]
 *   loss_dev                                [M][n]
 *   state_in_dev, state_out_dev             [M][n] records: cmps_rho_bank_stream_state_bytes(h, n) = M * cmps_rho_stream_state_bytes of
 *                                           a plain handle of the same D and rank (records of 64 rank + 4 floats; 0 for a null handle,
 *                                           n < 1, and outside RhoCMPS bank mode)
 *   audio_dev                               [n_audio][forced + 1], n_audio in {1, n, M * n}
 *   noise_dev                               [n_noise][length], n_noise in {n, M * n} (not looked at when length == 0)
 * The promise: member m's slices of out, pred, nll, loss and the state records hold, bit for bit, what cmps_rho_stream /
 * cmps_rho_stream_score give on a plain handle set to model m with the same T -- cmps_set_params_dev on row m of params_dev, then
 * cmps_rho_set_state on member m's columns (phi_dev + m * 2 rank D: phi_re, then phi_im) -- fed member m's audio and noise rows.  A cut
 * changes no bit, as for the plain stream.
 * Scope: the RhoCMPS bank's own (D <= 32, 3 <= rank <= 32, CMPS_VARIANT_AUTO / WAVE, default options), where a plain handle picks
 * k_sample_rho_mfma too.  There is no save_states: a bank has one T, the table length, and no separate stash capacity; a member taken
 * out as a plain model keeps cmps_rho_states.  A saved cmps_rho_bank_loss_fwd stays valid across these calls (they write no stash).
 * CMPS_ERR_STATE outside RhoCMPS bank mode (before any set_params, plain mode, legacy mode, a PsiCMPS bank) and for a variant or a
 * non-default option set behind cmps_rho_bank_set_state_dev; the plain cmps_rho_stream* entries return CMPS_ERR_STATE in bank mode, and
 * cmps_bank_stream* (the PsiCMPS bank's) refuse a RhoCMPS bank.  CMPS_ERR_BAD_ARG: n_audio not in {1, n, M * n}; n_noise not in
 * {n, M * n} when length > 0; M * n * (forced + length) beyond 2^31 - 1; and everything the plain entries refuse (state_in_dev NULL <=>
 * k0 == 0, the table rows with a message naming the needed T, null pointers, the counts).  Every message starts with the entry's name
 * and is returned before the device is touched.
 * Asynchronous on `stream`; never synchronises, allocates nothing, touches nothing outside the stated extents.  With
 * CMPS_OPT_KERNEL_EVENTS the launch is recorded under the plain entries' names: k_sample_rho_mfma_stream, k_sample_rho_mfma_score.
 */
size_t cmps_rho_bank_stream_state_bytes(cmps_handle_t h, int n);
int cmps_rho_bank_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                         const float* audio_dev, int n_audio, int forced,
                         const float* noise_dev, int n_noise, int length,
                         int n, float* out_dev, float* pred_dev, void* stream);
int cmps_rho_bank_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0,
                               const float* audio_dev, int n_audio, int forced, int n,
                               float* nll_dev, float* loss_dev, float* pred_dev, void* stream);

/*
 * The samplers' Gaussian noise, drawn on the device.  Replaces: tf.random_normal([length, n], stddev = sigma * sqrt(temp * delta_t)) inside
 * `sample` (model.py:246 / :88, 96, 106), for the noise_dev argument of cmps_psi_sample, _sample_primed, cmps_psi_stream, cmps_rho_sample,
 * _sample_primed and cmps_rho_stream -- same layout, row-major [path][step]:
 *   noise_dev[b * length + j] = stddev * z(seed, first_path + b, first_step + j)      (one float32 multiply), b < n, j < length.
 * The generator is counter-based: z is a pure function of (seed, path, step), so cutting a run differently, resuming it in another process
 * or sharding its paths gives the same noise without any generator state.  THE DEFINITION (normative; tests/_noise_ref.py restates it in
 * numpy) for a 64-bit seed, a 32-bit path and a 64-bit step index s:
 *   q = s >> 2,  r = s & 3
 *   (x0, x1, x2, x3) = Philox4x32-10(counter = (q & 0xffffffff, q >> 32, path, 0), key = (seed & 0xffffffff, seed >> 32))
 *     multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2), key increments 0x9E3779B9 and 0xBB67AE85, ten rounds, in the
 *     Random123 form: per round  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),  then the key is bumped.
 *     Known answers (counter words, key words -> output):
 *       00000000 x 4                        | 00000000 x 2        -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *       ffffffff x 4                        | ffffffff x 2        -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *       243f6a88 85a308d3 13198a2e 03707344 | a4093822 299f31d0   -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   for the pair j in {0, 1}:
 *     a = x[2j] >> 8,      u = (a + 1) * 2^-24     in (0, 1]   (exact in float32)
 *     c = x[2j+1] >> 8,    v = c * 2^-23           in [0, 2)   (exact in float32)
 *     rad = sqrtf(-2 * logf(u));   z[2j] = rad * cospif(v),   z[2j+1] = rad * sinpif(v)        (float32; the accurate functions, not the
 *     fast intrinsics: near u -> 1 the result is the small difference a fast logarithm gets wrong)
 *   z(seed, path, s) = z[r].   |z| <= sqrt(48 ln 2) ~ 5.768, and u > 0: no Inf or NaN can arise.
 * The integer part is bit-exact; the float part is within a few float32 roundings of the definition evaluated in double.
 * first_step is THE TABLE ROW OF THE FIRST SAMPLED STEP: 0 for cmps_*_sample, prime_T - 1 behind a prime, k0 + forced in a stream segment
 * -- so a primed sample and a follow-then-generate stream with the same seed draw the same noise.  first_path keeps the paths of a
 * caller who shards them over processes distinct.
 * Needs no cmps_set_params: it works on a fresh handle of any D and in legacy mode.  Asynchronous on `stream`; never synchronises,
 * allocates nothing, reads no device memory and touches no element outside noise_dev[0 .. n * length).
 * CMPS_ERR_BAD_ARG, each with a message: a null handle or noise_dev; n < 1 or length < 1; stddev negative or not finite;
 * first_path + n > 2^32; first_step + length overflowing 64 bits.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_noise_philox.
 */
int cmps_noise_fill(cmps_handle_t h, unsigned long long seed, unsigned long long first_step,
                    unsigned first_path, int n, int length, float stddev,
                    float* noise_dev, void* stream);

/*
 * A training batch cut out of a dataset that is already in device memory.  Replaces: audio_dataset.batch(...) ... get_next()
 * (data.py:37-43), whose order the caller plans on clip indices (audio_mps_amd/device_data.py).
 *   data_dev  [n_clips * clip_len] float32, row-major [clip][sample];  index_dev [B] int;  offset_dev [B] int, or NULL for all zero;
 *   audio_dev[b * T + j] = data_dev[index[b] * clip_len + offset[b] + j],   b < B, j < T      (all address arithmetic in 64 bits).
 * THE ROW GUARD: a row whose index[b] lies outside [0, n_clips) or whose offset[b] lies outside [0, clip_len - T] is written as T quiet
 * NaNs (0x7fc00000) and nothing is read for it -- a bad plan is memory-safe and loud (the loss turns NaN); the other rows are unaffected.
 * Only rows named by a valid index are read, and of those only the T samples copied.
 * Every pointer needs 4-byte alignment only.  Needs no cmps_set_params: it works on a fresh handle of any D and in legacy mode.
 * Asynchronous on `stream`; never synchronises, allocates nothing and touches no element outside audio_dev[0 .. B * T).
 * CMPS_ERR_BAD_ARG, each with a message, the first failing check speaking: a null handle, data_dev, index_dev or audio_dev; B < 1 or T < 1;
 * n_clips < 1 or n_clips > 2^31 - 1; clip_len < T.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_batch_gather.
 */
int cmps_batch_gather(cmps_handle_t h, const float* data_dev, long long n_clips, long long clip_len,
                      const int* index_dev, const int* offset_dev, int B, int T,
                      float* audio_dev, void* stream);

/*
 * cmps_batch_gather out of a dataset held as int16 (16-bit PCM, x = i / 32768: half the memory of float32), widened on the way:
 *   data_dev  [n_clips * clip_len] int16, row-major [clip][sample];  index_dev, offset_dev, audio_dev as in cmps_batch_gather;
 *   audio_dev[b * T + j] = (float)data_dev[index[b] * clip_len + offset[b] + j] * scale,   b < B, j < T
 * -- an exact integer-to-float conversion followed by ONE float32 multiply, so with scale = 2^-15 a batch holds the bits of the float32
 * dataset i * 2^-15.  THE ROW GUARD, the address arithmetic, the argument checks, their order and their messages are cmps_batch_gather's: a
 * row out of range is written as T quiet NaNs (0x7fc00000) and nothing is read for it; only rows named by a valid index are read, and of those
 * only the T samples copied -- EXCEPT that a read may reach the aligned dword that contains the row's first or last copied sample, that is at
 * most 2 bytes before the first and 2 bytes behind the last, and never outside data_dev[0 .. n_clips * clip_len): the first and last
 * element of the buffer are not overshot by a byte.
 * data_dev needs 2-byte alignment only, index_dev, offset_dev and audio_dev 4-byte alignment.  Needs no cmps_set_params: it works on a fresh
 * handle of any D and in legacy mode.  Asynchronous on `stream`; never synchronises, allocates nothing and touches no element outside
 * audio_dev[0 .. B * T).
 * CMPS_ERR_BAD_ARG, each with a message, the first failing check speaking: a null handle, data_dev, index_dev or audio_dev; B < 1 or T < 1;
 * n_clips < 1 or n_clips > 2^31 - 1; clip_len < T; and last, scale not finite or <= 0.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_batch_gather_i16.
 */
int cmps_batch_gather_i16(cmps_handle_t h, const short* data_dev, long long n_clips, long long clip_len,
                          const int* index_dev, const int* offset_dev, int B, int T, float scale,
                          float* audio_dev, void* stream);

/*
 * The per-clip losses of an evaluation pass reduced on the device: loss_dev[0 .. B), the losses of the clips first_id .. first_id + B - 1
 * (the id of loss_dev[b] is first_id + b), are folded into ONE 64-byte record in caller-owned device memory, so that a pass over a whole
 * dataset downloads 64 bytes once.  Replaces: eval_metric_ops={"loss": tf.metrics.mean(loss)} (training_estimators.py:70-74), and says what a
 * bare mean hides.  THE RECORD (normative; little-endian, 8-byte aligned; cmps_loss_stats_rec below):
 *   offset  type       field
 *        0  double     sum              of the finite losses
 *        8  double     sumsq            of the finite losses, each squared in double (exact for a float32)
 *       16  long long  n_finite
 *       24  long long  n_nonfinite      NaN, +Inf, -Inf
 *       32  long long  argmin           id of the smallest finite loss, the lowest id on ties; -1 while there is none
 *       40  long long  argmax           likewise for the largest
 *       48  long long  first_nonfinite  the lowest id of a non-finite loss; -1 while there is none
 *       56  float      min              the loss at argmin (+Inf while n_finite == 0)
 *       60  float      max              the loss at argmax (-Inf while n_finite == 0)
 * reset != 0 ignores what the record held (no memset is needed before the first call); reset == 0 continues it.  A non-finite value enters
 * nothing but n_nonfinite and first_nonfinite.  No atomics: one workgroup, a fixed assignment of elements to threads and a fixed reduction
 * tree, and the update is ordered by the stream -- the same sequence of calls gives the same bits on every run.  sum and sumsq are
 * accumulated in double in that fixed order: within n_finite * 2^-53 * sum |x| of the exact sums.
 * Needs no cmps_set_params: it works on a fresh handle of any D and in legacy mode.  Asynchronous on `stream`; never synchronises, allocates
 * nothing, reads loss_dev[0 .. B) and touches only the 64 bytes of the record.
 * CMPS_ERR_BAD_ARG, each with a message, the first failing check speaking: a null handle; a null loss_dev; a null stats_dev or one that is
 * not 8-byte aligned; B < 1; first_id < 0 or first_id + B > 2^63 - 1.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_loss_stats.
 */
typedef struct cmps_loss_stats_rec {
    double sum, sumsq;
    long long n_finite, n_nonfinite, argmin, argmax, first_nonfinite;
    float min, max;
} cmps_loss_stats_rec;
int cmps_loss_stats(cmps_handle_t h, const float* loss_dev, int B, long long first_id,
                    int reset, void* stats_dev, void* stream);

/*
 * A bank of one model per class judged as a classifier, on the device: loss_dev[m * ld + b] (ld >= B) is the [M][B] output of
 * cmps_bank_loss_fwd / cmps_rho_bank_loss_fwd over ONE shared batch, the loss of clip first_id + b under member m; label_dev[b] is the
 * member that clip belongs to (a value outside [0, M): unlabelled; label_dev == NULL: every clip unlabelled); best_dev is [B] int or NULL.
 * Replaces: nothing -- the reference trains a model per pitch (reader.py:9-66) and never judges them against each other.
 * PER CLIP (normative; tests/_classify_ref.py restates it in numpy).  A NaN or +-Inf loss makes that member ABSENT for that clip.
 *   best    the present member with the smallest loss (float32 compare; the lowest m on ties), written to best_dev[b].  No present member:
 *           the clip is UNDECIDED, best = -1, and it enters n_undecided and first_undecided and nothing else.
 *   margin  (second-smallest present loss) - (smallest), each widened to double first; over decided clips with at least two present members.
 *   xent    -log p(label | clip), p = softmax(-loss) over the present members (a uniform prior), over labelled clips whose own member is
 *           present:  xent = (loss[label] - lmin) + log(sum_m exp(-(loss[m] - lmin))),  lmin the smallest present loss, everything in double,
 *           the sum in member order.  xent >= 0.
 * THE RECORD (normative; little-endian, 8-byte aligned): the 72-byte header cmps_bank_classify_head below, then the counts
 *   offset  type       field
 *        0  double     sum_xent         over the n_xent clips
 *        8  double     sum_margin       over the n_margin clips
 *       16  long long  n_decided        clips with a best member, labelled or not
 *       24  long long  n_undecided
 *       32  long long  n_unlabelled     decided clips without a label in [0, M)
 *       40  long long  n_correct        labelled decided clips with best == label
 *       48  long long  n_xent
 *       56  long long  n_margin
 *       64  long long  first_undecided  the lowest id of an undecided clip; -1 while there is none
 *       72  long long  confusion[M][M]  row = label, column = best: the labelled decided clips
 *   72 + 8 M M  long long  unlabelled_best[M]   the decided unlabelled clips by best
 * cmps_bank_classify_stats_bytes(M) = 72 + 8 M M + 8 M is the record's size; 0 for M outside [1, 1024].
 * reset != 0 ignores what the record held (no memset is needed before the first call); reset == 0 continues it.  One workgroup, a fixed
 * assignment of clips to threads and a fixed reduction tree for the header, and the update is ordered by the stream; the confusion counts
 * are integer atomic adds, whose sum does not depend on the order -- the same sequence of calls gives the same bits on every run.
 * ROUNDING.  With L = max |present loss|, u = 2^-53, and exp and log of the device within 4 ulp in double (HIP documents 1 ulp for both;
 * OpenCL's bound is 3): a clip's xent is within u (1.4 M + 78 + 4 L) of exact arithmetic on the float32 losses -- the sum of at most M
 * terms in (0, 1], the log of a number in [1, M], and two differences of numbers of size L -- and a margin within u |margin|.  Summed in
 * double in any order:
 *   |sum_xent   - exact| <= 2^-52 n_xent   (M + 40 + 2 L + sum of the exact xent)
 *   |sum_margin - exact| <= 2^-52 n_margin (sum of the exact margins)
 * Needs no cmps_set_params: it works on a fresh handle of any D and in legacy mode.  Asynchronous on `stream`; never synchronises, allocates
 * nothing, reads loss_dev[m * ld + b] for m < M, b < B and label_dev[0 .. B) only, and writes only the record and best_dev[0 .. B).
 * CMPS_ERR_BAD_ARG, each with a message, the first failing check speaking: a null handle; a null loss_dev; a null stats_dev or one that is
 * not 8-byte aligned; M outside [1, 1024]; B < 1; ld < B; first_id < 0 or first_id + B > 2^63 - 1.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_classify_stats.
 */
typedef struct cmps_bank_classify_head {
    double sum_xent, sum_margin;
    long long n_decided, n_undecided, n_unlabelled, n_correct, n_xent, n_margin, first_undecided;
} cmps_bank_classify_head;
size_t cmps_bank_classify_stats_bytes(int M);
int cmps_bank_classify_stats(cmps_handle_t h, const float* loss_dev, int M, int B, long long ld,
                             const int* label_dev, long long first_id, int reset,
                             void* stats_dev, int* best_dev, void* stream);

/*
 * The same [M][B] losses and labels turned into the cotangents of a cross-entropy training step, on the device: the members of a class bank
 * trained AGAINST each other.  loss_dev[m * ld + b] (ld >= B) as above, the output of cmps_bank_loss_fwd(save_for_bwd = 1) over ONE shared
 * batch; label_dev[b] the member clip b belongs to; weight_dev[m * ldw + b] (ldw >= B) receives the weights cmps_bank_loss_bwd_weighted takes.
 * Replaces: nothing -- the reference trains a model per pitch (reader.py:9-66), each on its own clips alone.
 * THE OBJECTIVE (normative; tests/_disc_ref.py restates it in numpy).  inv_temp = kappa > 0, gen_weight = alpha >= 0, disc_weight = beta >= 0,
 * doubles.  Per clip b, with l_m = loss_dev[m * ld + b], y = label_dev[b], and a NaN or +-Inf loss making that member ABSENT for that clip:
 *   SKIPPED  y outside [0, M): every weight of the clip is +0 and it counts in n_unlabelled.  Else member y absent: every weight of the clip
 *            is +0 and it counts in n_own_absent.  A skipped clip enters nothing else.
 *   USED     every other clip.  With lmin the smallest present loss, everything in double, the sums in member order:
 *              S      = sum over the present m of exp(-kappa (l_m - lmin))                         1 <= S <= M
 *              p_m    = exp(-kappa (l_m - lmin)) / S
 *              xent   = kappa (l_y - lmin) + log S                                                 >= 0
 *              w[m][b] = float32(alpha [m == y] + beta kappa ([m == y] - p_m))   for a present m;   +0 for an absent m
 *            w[m][b] is d J_b / d l_m of J_b = alpha l_y + beta xent_b: the gradient of sum_b J_b with respect to member m's parameters is
 *            the gradient of sum_b w[m][b] loss[m][b], which cmps_bank_loss_bwd_weighted computes.  With kappa = 1 the xent is exactly the
 *            one of cmps_bank_classify_stats.
 * THE RECORD (normative; little-endian, 8-byte aligned; cmps_bank_classify_weights_rec below), 40 bytes:
 *   offset  type       field
 *        0  double     sum_xent         over the used clips
 *        8  double     sum_own_loss     sum of l_y over the used clips
 *       16  long long  n_used
 *       24  long long  n_unlabelled
 *       32  long long  n_own_absent
 * reset != 0 ignores what the record held (no memset is needed before the first call); reset == 0 continues it.  One workgroup, a fixed
 * assignment of clips to threads, a fixed reduction tree for the record, no floating-point atomics, and the update is ordered by the
 * stream -- the same sequence of calls gives the same bits on every run.
 * ROUNDING.  u = 2^-53, L = max |present loss|, exp and log of the device within 4 ulp = 8 u in double (as for cmps_bank_classify_stats).
 * The argument a = kappa (l_m - lmin) >= 0 carries two roundings, |da| <= 2 u a, so the computed e_m = exp(-a) is within
 * u e_m (8 + 2 a) <= u (8 e_m + 0.74) of the exact one (a exp(-a) <= 1 / e).  S, a sum of at most M such terms with S >= 1, is within
 * u S (1.74 M + 7) of exact; p_m = e_m / S <= 1 within u (0.74 + p_m (1.74 M + 16)) <= u (1.74 M + 17).  [m == y] - p_m, the product
 * beta kappa, the product of the two and the sum with alpha add four roundings of numbers no larger than alpha + beta kappa.  The result is
 * rounded to float32 once (a subnormal result to within 2^-150):
 *   |w[m][b] - exact| <= 2^-24 |exact| + 2^-52 (alpha + beta kappa) (M + 16) + 2^-149
 * and two evaluations that each meet this bound -- the device's and a float64 restatement -- differ by at most twice it.
 * A clip's xent: the argument's two roundings (2 u kappa |l_y - lmin| <= 4 u kappa L), log S within u (1.74 M + 7) + 8 u log M
 * <= u (1.74 M + 63), one sum: within u (2 M + 64 + 4 kappa L + xent).  Summed in double in any order:
 *   |sum_xent     - exact| <= 2^-52 n_used (M + 32 + 2 kappa L + sum of the exact xent)
 *   |sum_own_loss - exact| <= 2^-53 n_used (sum of |l_y|)
 * Needs no cmps_set_params: it works on a fresh handle of any D and in legacy mode.  Asynchronous on `stream`; never synchronises, allocates
 * nothing, reads loss_dev[m * ld + b] for m < M, b < B and label_dev[0 .. B) only, and writes exactly weight_dev[m * ldw + b] for m < M,
 * b < B and the 40 bytes of the record.
 * CMPS_ERR_BAD_ARG, each with a message, the first failing check speaking: a null handle; a null loss_dev; a null label_dev; a null
 * weight_dev; a null record_dev or one that is not 8-byte aligned; M outside [1, 1024]; B < 1; ld < B; ldw < B; inv_temp not finite or
 * <= 0; gen_weight not finite or < 0; disc_weight not finite or < 0.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_classify_weights.
 */
typedef struct cmps_bank_classify_weights_rec {
    double sum_xent, sum_own_loss;
    long long n_used, n_unlabelled, n_own_absent;
} cmps_bank_classify_weights_rec;
int cmps_bank_classify_weights(cmps_handle_t h, const float* loss_dev, int M, int B, long long ld, const int* label_dev, double inv_temp,
                               double gen_weight, double disc_weight, int reset, float* weight_dev, long long ldw, void* record_dev,
                               void* stream);

/*
 * A bank followed along a signal judged as a classifier AFTER EVERY SAMPLE, on the device: nll_dev [M][n][steps], contiguous, is what
 * cmps_bank_stream_score / cmps_rho_bank_stream_score wrote for one segment -- the loss increment of step k of path g under member m at
 * nll_dev[(m * n + g) * steps + k] -- and this entry folds it into the running totals and, per path and step, the posterior over the
 * members, the most probable member, its probability, and the first step at which that probability reached a threshold.
 * Replaces: nothing -- the reference scores one model along one clip (model.py:279, 293-294) and never weighs models against each other.
 *   total_in_dev  [M][n] the running totals before the segment, or NULL: every total starts at 0.f (a stream at k0 == 0)
 *   log_prior_dev [M] doubles, 8-byte aligned, or NULL: a uniform prior (log prior 0 for every member).  An entry is finite or -inf; it need
 *                 not be normalised (a common shift changes nothing).  NaN and +inf entries give unspecified values, within the extents.
 *   inv_temp      kappa > 0
 *   total_out_dev [M][n], post_dev [M][n][steps], best_dev [n][steps] int, conf_dev [n][steps]: each may be NULL and is then not written;
 *                 total_out_dev may equal total_in_dev
 *   decision_dev  [n] records cmps_bank_decision (16 bytes each, 8-byte aligned), or NULL; threshold, first_step and reset are read only
 *                 with a record
 * THE DEFINITION (normative; tests/_posterior_ref.py restates it in numpy).  Per member m and path g:
 *   c_m(-1) = total_in[m][g] (or 0.f);  c_m(k) = c_m(k - 1) + nll[m][g][k]: ONE float32 addition per step, in step order -- the fold
 *   every score kernel performs on its running loss.  total_out[m][g] = c_m(steps - 1) is therefore, bit for bit, the loss_dev the score
 *   call of the same segment wrote, and cutting a run into calls (total_out of one as total_in of the next) changes no bit of anything.
 *   Member m is ABSENT at step k of path g when c_m(k) is NaN or +-Inf; the total being a running sum, it stays absent from there on.
 * Per (g, k), over the present members, in double:
 *   a_m  = kappa (double)c_m(k) - log_prior[m]
 *   amin = the smallest a_m
 *   S    = sum over the present m of exp(-(a_m - amin))                                          1 <= S <= M
 *   p_m  = exp(-(a_m - amin)) / S
 *   post[m][g][k] = float32(p_m) for a present m, +0 for an absent one
 *   best[g][k]    = the present m with the smallest a_m (a double compare; the lowest m on ties);  conf[g][k] = float32(1 / S) = p_best
 *   No member present: best = -1, conf = +0, every post = +0.
 *   A member with log prior -inf has a_m = +inf: it never wins and its p is 0; it is present only in the sense that its total is finite.
 *   A step at which every present member has log prior -inf is a step with no member present.
 * THE DECISION.  decision_dev[g] = {step, member, reserved} holds the FIRST step at which the bank was sure.  reset != 0 ignores what the
 * record held and starts from {-1, -1, 0} (no memset is needed before the first call); reset == 0 continues it.  A record with step >= 0
 * is left as it is.  Otherwise the first k of this call with 1 / S >= threshold -- compared in double, before the rounding to float32 --
 * sets step = first_step + k and member = best[g][k]; later dips below the threshold change nothing.
 * ROUNDING.  u = 2^-53, A' = max over the present m with a finite log prior of (kappa |c_m| + |log_prior_m|), exp of the device within 4 ulp = 8 u in double (as
 * for cmps_bank_classify_stats).  a_m carries two roundings of numbers no larger than A' (one where the compiler fuses them), amin the
 * same, and their difference d = a_m - amin >= 0 one more: |dd| <= u (4 A' + d).  e_m = exp(-d) <= 1 is then within
 * u (e_m (8 + 4 A') + 0.37) of the exact one (d exp(-d) <= 1 / e), whatever shift stands in for amin -- the soft-max does not depend on
 * it.  S, a sum of at most M such terms in any order with S >= 1, is within u S (1.37 M + 8 + 4 A') of exact; p_m = e_m / S <= 1 and
 * 1 / S within u (1.37 M + 18 + 8 A').  The result is rounded to float32 once (a subnormal result to within 2^-150):
 *   |post[m][g][k] - exact| <= 2^-24 |exact| + 2^-52 (M + 16 + 4 A') + 2^-149          and the same for conf[g][k]
 * where "exact" is exact arithmetic on the float32 totals c_m(k), which every evaluation shares bit for bit.  Two evaluations that each
 * meet this bound -- the device's and a float64 restatement -- differ by at most twice it.  best and the decision are exact compares of
 * rounded doubles: two evaluations agree on them wherever the runner-up's a is not within that error of the best's and 1 / S not within
 * it of the threshold.
 * One workgroup per path, a fixed assignment of members and steps to threads, fixed merge orders, no atomics, and nll_dev is read once:
 * the same call gives the same bits on every run.
 * Needs no cmps_set_params: it works on a fresh handle of any D, in legacy mode and for either kind of bank.  Asynchronous on `stream`;
 * never synchronises, allocates nothing, uses no global scratch, reads nll_dev[0 .. M n steps), total_in_dev[0 .. M n),
 * log_prior_dev[0 .. M) and (reset == 0) decision_dev[0 .. n) only, and writes only the stated extents of the outputs that are not NULL.
 * CMPS_ERR_BAD_ARG, each with a message that starts with the entry's name, the first failing check speaking, before the device is
 * touched: a null handle; a null nll_dev; M outside [1, 1024]; n < 1; steps < 1; M n steps > 2^31 - 1; inv_temp not finite or <= 0;
 * log_prior_dev not 8-byte aligned; decision_dev not 8-byte aligned; with a decision_dev: threshold not finite or outside (0, 1];
 * first_step < 0 or first_step + steps > 2^63 - 1.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_bank_posterior.
 */
typedef struct cmps_bank_decision {
    long long step;      /* first_step + k of the first sure step; -1 while undecided */
    int member;          /* best at that step; -1 while undecided */
    int reserved;        /* 0 */
} cmps_bank_decision;
int cmps_bank_posterior(cmps_handle_t h, const float* nll_dev, int M, int n, int steps,
                        const float* total_in_dev, const double* log_prior_dev, double inv_temp,
                        float* total_out_dev, float* post_dev, int* best_dev, float* conf_dev,
                        double threshold, long long first_step, int reset, void* decision_dev, void* stream);

/*
 * The temperature and the prior of a class bank FITTED on held-out losses, on the device: loss_dev[m * ld + b] (ld >= N) holds the [M][N]
 * losses of N held-out clips under the M members -- the outputs of cmps_bank_loss_fwd / cmps_rho_bank_loss_fwd over the batches of a
 * held-out set, kept side by side -- and label_dev[b] the member clip b belongs to.  The bank answers with
 * p_m ~ prior_m exp(-loss_m / temperature); this entry finds the temperature and (or) the prior under which the held-out labels are the
 * most likely.  With max_iter == 0 or fit == 0 it evaluates the held-out cross-entropy under the GIVEN temperature and prior.
 * Replaces: nothing -- the reference trains a model per pitch (reader.py:9-66) and never judges them against each other.
 * THE MODEL AND THE OBJECTIVE (normative; tests/_calib_ref.py restates them in numpy).  l[m][b] = loss_dev[m * ld + b], y_b = label_dev[b].
 * theta = (kappa, c_0 .. c_{M-1}) in double: kappa = 1 / temperature > 0, c_m = log prior_m up to a common shift.  A NaN or +-Inf loss
 * makes that member ABSENT for that clip.
 *   SKIPPED  y_b outside [0, M): counted in n_unlabelled.  Else member y_b absent: counted in n_own_absent.  A skipped clip enters nothing
 *            else (the rules and counters of cmps_bank_classify_weights).
 *   USED     every other clip; n of them, n_m with label m.  With lmin_b the smallest present loss, everything in double, the sums in
 *            member order:
 *              a_m    = kappa (l_m - lmin_b) - c_m,  amin = the smallest a_m  (the shift of the exponentials, as in cmps_bank_posterior)
 *              S      = sum over the present m of exp(-(a_m - amin))                               1 <= S <= M
 *              p_m    = exp(-(a_m - amin)) / S
 *              xent_b = (a_y - amin) + log S
 *              E_b    = sum_m p_m (l_m - lmin_b),   V_b = sum_m p_m (l_m - lmin_b)^2 - E_b^2
 *   Over the used clips:
 *              J(theta) = (1 / n) sum_b xent_b                                   the objective, convex in theta
 *              g = dJ / dkappa   = (1 / n) sum_b ((l_y - lmin_b) - E_b)         monotone in kappa
 *              h = d2J / dkappa2 = (1 / n) sum_b V_b  >= 0
 *              q_m = sum_b p_m(b),  so  dJ / dc_m = (q_m - n_m) / n
 * THE FIT.  fit is a set of bits.  With CMPS_CALIB_TEMPERATURE kappa moves inside [kappa_min, kappa_max] towards the root of g: a Newton
 * step on g of at most a factor 8 in kappa, kept inside a sign bracket and sent to the bracket's middle in log kappa when it leaves it.
 * With CMPS_CALIB_PRIOR every member with n_m > 0 takes the iterative-scaling step c_m += log(n_m / q_m) (generalised iterative scaling
 * for one-hot features: its auxiliary bound separates per coordinate, so J never rises); a member with n_m == 0 is UNFITTED and its c_m
 * keeps its input bits.  With both, kappa steps and prior sweeps alternate (whichever of the two has met its test stands back), and the
 * bracket is opened again whenever c has moved.  c is never shifted on the device: the host normalises it for display.  The iterates are
 * not normative; the properties below are.
 *   theta_dev   [1 + M] doubles, 8-byte aligned: in the start, out the fit.  A start kappa outside the box cannot be refused without a
 *               download: where the temperature is fitted and max_iter > 0 the first update puts it on the nearer bound (a NaN on
 *               kappa_min).  That counts as a pass, and the theta with kappa on the box is then "the input theta" of the record and
 *               of the properties: xent_start is J there.  A c_m is finite or -inf (a prior of zero); a used clip whose OWN member has
 *               c = -inf has probability zero, J is +inf (NaN where no present member of a clip has a finite c) and theta, the record
 *               and the flags are unspecified, within the extents -- the host layer refuses such a prior.
 *   record_dev  80 bytes, 8-byte aligned (cmps_bank_calibrate_rec below); written once, when the fit finishes
 *   scratch_dev cmps_bank_calibrate_scratch_bytes(M, N) bytes, 8-byte aligned; may hold anything before the call; 0 for M outside
 *               [1, 1024], N < 1 or M N beyond 2^62
 * THE RECORD (normative; little-endian, 8-byte aligned):
 *   offset  type       field
 *        0  double     xent_start     J at the input theta (kappa put on the box first where it lay outside: see theta_dev)
 *        8  double     xent_end       J at the returned theta
 *       16  double     g_logk         kappa g at the returned theta
 *       24  double     resid_prior    max over the fitted m of |q_m - n_m| / n at the returned theta; 0 when the prior is not fitted
 *       32  double     curvature      h at the returned theta
 *       40  long long  n_used
 *       48  long long  n_unlabelled
 *       56  long long  n_own_absent
 *       64  int        passes         evaluations of J made
 *       68  int        flags          1 CONVERGED, 2 AT_KAPPA_MIN, 4 AT_KAPPA_MAX, 8 NO_DATA, 16 MAX_ITER
 *       72  int        n_unfitted     members with n_m == 0
 *       76  int        reserved       0
 * PROPERTIES.
 *   1  CONVERGED means that at ONE pass, at the returned theta: |kappa g| <= tol, or kappa sits on a bound of the box with g pushing
 *      outwards (the bound's flag is then set as well); and, with the prior fitted, resid_prior <= tol.  Otherwise MAX_ITER is set and the
 *      theta with the lowest J of all passes is returned, with the record's figures from that pass.
 *   2  xent_end <= xent_start (a converged theta whose J came out above xent_start by rounding is given up for the best one, under
 *      MAX_ITER).  With fit == 0 or max_iter == 0: theta keeps its bits, xent_end == xent_start, passes == 1.
 *   3  Without CMPS_CALIB_PRIOR every c_m keeps its bits, without CMPS_CALIB_TEMPERATURE kappa keeps its bits, an unfitted member always
 *      keeps its bits, kappa stays inside [kappa_min, kappa_max], and where g == 0 (all present losses of every clip equal) kappa keeps its
 *      start value.
 *   4  n_used == 0: NO_DATA, theta untouched, both xents 0, passes == 1.
 * A FINITE OPTIMUM needs clips that are wrong and more clips than fitted parameters.  An unfitted member with a finite c_m keeps a share
 * of every clip's probability that no finite c of the others takes away: with the prior fitted J then has no minimum, the fitted c_m
 * grow without bound (the residual falls like 1 / passes) and the fit ends with MAX_ITER at the best theta.  c_m = -inf, a prior of zero,
 * is carried through as a member that never wins (a_m = +inf, p_m = 0) and keeps its bits like any unfitted member's.
 * HOW IT RUNS.  One iteration is two launches: k_calib_pass, many workgroups over the clips, each leaving its sums of J, g, h and q[M] in
 * double in a row of scratch_dev; k_calib_update, one workgroup that adds the rows in row order, decides, moves theta and keeps the solver's
 * state, the best theta and a `done` word in scratch_dev.  The entry enqueues max_iter + 1 such pairs without looking; once `done` is set
 * the later launches leave at their first, uniform branch.  No cooperative launch, no workgroup waits for another, no floating-point
 * atomics (n_m is an integer count); the assignment of clips to threads and every order of summation are fixed: the same call gives the
 * same bits on every run.
 * ROUNDING.  u = 2^-53, exp and log of the device within 4 ulp = 8 u in double (as for cmps_bank_classify_stats).  At a theta, with
 * D = the largest (l_m - lmin_b) over the present members of the used clips and A = kappa D + max_m |c_m|:  d = l_m - lmin_b carries one
 * rounding, a_m two more, each of a number no larger than A, and so does amin: t = a_m - amin >= 0 has |dt| <= u (6 A + t), and
 * e_m = exp(-t) <= 1 is within u (e_m (8 + 6 A) + 0.37) of exact (t exp(-t) <= 1 / e).  S, a sum of at most M such terms with S >= 1, is
 * within u S (1.37 M + 8 + 6 A); p_m within u (1.37 M + 18 + 12 A); log S within u (1.37 M + 8 + 6 A) + 8 u log M, so a clip's xent
 * within u (1.37 M + 64 + 12 A + 2 xent).  sum_m e_m d_m <= S D is within u S D (1.37 M + 10 + 6 A), E_b within u D (3 M + 24 + 12 A), and
 * (l_y - lmin_b) - E_b, of size at most D, within u D (3 M + 27 + 12 A).  A mean of n terms summed in double in any order adds
 * n u (mean of the absolute terms):
 *   eps_J = 2^-52 (M + 32 + 6 A + (n / 2 + 2) J)                  bounds |J_device - J_exact|
 *   eps_g = 2^-52 D (1.5 M + 14 + 6 A + n / 2)                    bounds |g_device - g_exact|
 *   eps_q = 2^-52 n (0.7 M + 9 + 6 A + n / 2)                     bounds |q_m device - q_m exact|;  resid_prior within eps_q / n
 * where "exact" is exact arithmetic on the float32 losses and the doubles of theta.
 * Needs no cmps_set_params: it works on a fresh handle of any D, in legacy mode and for either kind of bank.  Asynchronous on `stream`;
 * never synchronises, allocates nothing, reads loss_dev[m * ld + b] for m < M, b < N and label_dev[0 .. N) only, and writes only
 * theta_dev[0 .. 1 + M), the record and the scratch.
 * CMPS_ERR_BAD_ARG, each with a message that starts with the entry's name, the first failing check speaking, before the device is
 * touched: a null handle; a null loss_dev; a null label_dev; a null theta_dev or one that is not 8-byte aligned; the same for record_dev;
 * the same for scratch_dev; M outside [1, 1024]; N < 1 or M ld beyond 2^62; ld < N; fit outside [0, 3]; max_iter outside [0, 10000]; tol
 * not finite or <= 0; kappa_min not finite or <= 0; kappa_max not finite or < kappa_min; scratch_bytes below
 * cmps_bank_calibrate_scratch_bytes(M, N).
 * With CMPS_OPT_KERNEL_EVENTS the launches are recorded as k_calib_pass and k_calib_update.
 */
enum { CMPS_CALIB_TEMPERATURE = 1, CMPS_CALIB_PRIOR = 2 };            /* `fit` is a bit set; 0 = evaluate only */
enum { CMPS_CALIB_CONVERGED = 1, CMPS_CALIB_AT_KAPPA_MIN = 2, CMPS_CALIB_AT_KAPPA_MAX = 4, CMPS_CALIB_NO_DATA = 8, CMPS_CALIB_MAX_ITER = 16 };
typedef struct cmps_bank_calibrate_rec {
    double xent_start, xent_end, g_logk, resid_prior, curvature;
    long long n_used, n_unlabelled, n_own_absent;
    int passes, flags, n_unfitted, reserved;
} cmps_bank_calibrate_rec;
size_t cmps_bank_calibrate_scratch_bytes(int M, long long N);
int cmps_bank_calibrate(cmps_handle_t h, const float* loss_dev, int M, long long N, long long ld, const int* label_dev,
                        int fit, int max_iter, double tol, double kappa_min, double kappa_max,
                        double* theta_dev, void* record_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/*
 * The synthetic training batch, generated where it is used.  Replaces: the damped_sine branch of get_audio (data.py:8-22): a 261.6 Hz sine
 * that starts after a Gamma(2)-distributed delay and decays with a time constant of 0.1 s.  Row b of audio_dev [B * T] is clip
 * c = first_clip + b, a pure function of (seed, c, T, delta_t): a caller who fills clips [start, start + count) of a global batch gets exactly
 * those rows of the whole batch without generating the rest, and a resumed run continues the sequence without generator state.
 * THE DEFINITION (normative; tests/_data_ref.py restates it in numpy), fl32(x) = x rounded to float32, every operation in float32:
 *   (x0, x1, ., .) = Philox4x32-10(counter = (c & 0xffffffff, c >> 32, 0, 1), key = (seed & 0xffffffff, seed >> 32))     as in cmps_noise_fill;
 *     counter word 3 = 1 keeps these draws apart from the noise's, which use 0
 *   u_i = ((x_i >> 8) + 1) * 2^-24     in (0, 1]   (exact in float32)
 *   delay = fl32(T / 200.0) * (-(logf(u0) + logf(u1)))       a Gamma(2, scale = delay_time / 2) draw with delay_time = T / 100
 *                                                            (data.py:13, 15), as the sum of two exponentials;  0 <= delay < 0.1664 T
 *   for sample j:  t = ((float)j - delay) * fl32(delta_t)
 *                  audio[b * T + j] = ((0.5f * (sign(t) + 1.0f)) * sinf(fl32(2 pi 261.6) * t)) * expf(-t / fl32(0.1))
 *     a product, in this order, as the reference writes it (data.py:19-22), with sign(0) = 0; the accurate logf / sinf / expf, not the fast
 *     intrinsics (the sine's argument reaches thousands of radians).
 * The Philox integers are bit-exact; the float part is within a few float32 roundings of the definition evaluated in double.  As in the
 * reference, the samples before the onset are the product 0 * expf(-t / 0.1) with t < 0: exactly zero while 0.1664 T delta_t stays below
 * 8.8 s (expf finite), which every clip shorter than 53 s does.
 * Needs no cmps_set_params: it works on a fresh handle of any D and in legacy mode.  Asynchronous on `stream`; never synchronises, allocates
 * nothing, reads no device memory and touches no element outside audio_dev[0 .. B * T).
 * CMPS_ERR_BAD_ARG, each with a message, the first failing check speaking: a null handle or audio_dev; B < 1, T < 1 or T > 2^24 (beyond that
 * (float)j is not exact); delta_t not finite or <= 0; first_clip + B overflowing 64 bits.
 * With CMPS_OPT_KERNEL_EVENTS the launch is recorded as k_damped_sine.
 */
int cmps_damped_sine_fill(cmps_handle_t h, unsigned long long seed, unsigned long long first_clip,
                          int B, int T, double delta_t, float* audio_dev, void* stream);

/*
 * Host utility (no GPU involved): CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of `n` bytes, continuing from
 * `crc_in` (0 to start).  TFRecord framing stores it masked (((crc >> 15) | (crc << 17)) + 0xa282ead8) behind the length
 * and behind the payload of every record; the reference reads those files with tf.data.TFRecordDataset (data.py:29,
 * training_estimators.py:79), which verifies them.  audio_mps_amd/tfrecord.py calls this when verify=True.
 */
unsigned cmps_crc32c(const void* data, size_t n, unsigned crc_in);

#ifdef __cplusplus
}
#endif
#endif /* CMPS_H_ */
