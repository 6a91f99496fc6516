"""The float32 kernels of 32 < D <= 128 (cmps_wide.hip, CMPS_VARIANT_WIDE: what AUTO selects above D = 32) against the C
oracle, through the C ABI.  The reference is float32 / complex64 at every bond dimension (/root/reference/model.py:300-325),
so the bars are the ones of the D <= 32 kernels (tests/test_gpu_parity.py):
  * per-clip log-likelihood: |hip - oracle_f32| <= 1e-5 * max(|oracle_f32|, 1)
  * gradients: max |hip - oracle_f32| <= 1e-4 * max |oracle_f32| per effective tensor (R, freqs, psi_0, A)."""
import numpy as np
import pytest

from _util import c_oracle_run, elastic_check, make_audio, rel_inf, strict_grad_sums
from test_gpu_parity import BLOCK, GRAD_RTOL, LOSS_RTOL, _check_against_oracle, _model

pytestmark = pytest.mark.gpu

WIDE, AUTO = 5, 0


def _wide_model(D, T, B, sigma=1e-4, seed=0, rscale=None, variant=WIDE):
    # the reference's random init makes 1 + e x / A go negative at large D (SURVEY hard part viii): scale R like the benchmark does
    if rscale is None:
        rscale = 0.1 if sigma == 1.0 else (1.0 if D <= 64 else 0.35)
    return _model(D, T, B, variant, sigma=sigma, seed=seed, rscale=rscale)


@pytest.mark.parametrize("D,T,B,sigma", [
    (64, 300, 4, 1e-4), (96, 260, 3, 1e-4), (128, 200, 4, 1e-4),          # the three padded sizes, even and odd batches
    (33, 150, 2, 1e-4), (40, 131, 5, 1e-4), (72, 140, 3, 1e-4), (100, 100, 1, 1e-4), (127, 90, 2, 1e-4),   # zero-padded rows
    (64, 257, 3, 1.0), (128, 130, 2, 1.0),                                # sigma = 1: Q = -(dt sigma^2 / 2) R^dagger R is visible
])
def test_oracle_parity(D, T, B, sigma):
    m, audio = _wide_model(D, T, B, sigma=sigma, seed=D + T)
    assert m._get_backend().variant == WIDE
    _check_against_oracle(m, audio)


@pytest.mark.parametrize("D,T,rs", [(40, 60, 0.6), (64, 130, 0.6), (128, 90, 0.5), (96, 257, 0.6)])
def test_qbar_sums_visible_at_large_sigma(D, T, rs):
    """The wide family's counterpart of tests/test_gpu_parity.py::test_qbar_sums_visible_at_large_sigma (the
    sigma = 1 cases above scale R by 0.1, which hides Qbar).  sigma = 0.36, A = 66, quiet audio and a large R make
    Q = -(delta_t sigma^2 / 2) R^dagger R (/root/reference/model.py:312) carry 14 ... 50 % of the R gradient (oracle, sigma = 0.36 against
    1e-4), so a wrong Qbar = sum ybar u^dagger cannot hide.  Every chain form (VALU, MFMA, MFMA forward only) and every GEMM arithmetic
    against f64t32 (float64 on the float32 time grid the kernels follow), the bar being the float32 oracle's own distance from it (x 3)
    plus the arithmetic's operand bits."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan, unpack_grad
    from oracle import c_oracle as C
    B = 3
    hp = HParams(minibatch_size=B, bond_dim=D, sigma=0.36, A=66.0)
    audio = (make_audio(B, T, hp.delta_t, 3) * np.float32(0.09)).astype(np.float32)
    gt = g64 = ref32 = None
    for chain in (0, 1, 2):
        for mode in (1, 2, 3):
            be = HipScan(D, rank1=mode)
            be.set_wide_chain(chain)
            m = PsiCMPS(hp, data_iterator=audio, seed=7, backend=be)
            assert be.variant == WIDE
            m.variables["Rx"] *= np.float32(rs)
            m.variables["Ry"] *= np.float32(rs)
            per = m.loss_per_clip()
            g = unpack_grad(strict_grad_sums(m)[0].cpu().numpy(), D)
            if gt is None:
                gt = C.unpack_grad(c_oracle_run(m, audio, "f64t32")["grad"], D)
                g64 = C.unpack_grad(c_oracle_run(m, audio, "f64")["grad"], D)
                ref32 = c_oracle_run(m, audio, "f32")
                g32 = C.unpack_grad(ref32["grad"], D)
                assert np.all(np.isfinite(ref32["loss_per_clip"]))
            assert np.max(np.abs(per - ref32["loss_per_clip"]) / np.maximum(np.abs(ref32["loss_per_clip"]), 1.0)) <= LOSS_RTOL
            for k in ("Rbar", "fbar", "psi0bar", "Abar"):
                floor = 3e-5 if mode == 1 else 1e-5                      # BF16X2 carries 16 operand bits
                elastic_check(f"chain {chain} mode {mode} {k}", rel_inf(g[k], gt[k]), 3 * rel_inf(g32[k], gt[k]) + floor,
                              rel_inf(g[k], g64[k]), 3 * rel_inf(g32[k], g64[k]) + floor)


def test_auto_selects_wide_above_32():
    from audio_mps_amd.scan import HipScan
    assert HipScan(33).variant == WIDE and HipScan(128).variant == WIDE and HipScan(32).variant == 2
    assert HipScan(64, variant=BLOCK).variant == BLOCK and HipScan(64, variant=3).variant == 3


@pytest.mark.parametrize("T", [2, 3, 4, 5, 6, 64, 65, 66, 67, 129, 130, 193, 258])
def test_chunk_and_unit_boundaries(T):
    """T - 1 steps around the 64-step scalar chunks, the 4-step ring of the reverse scan and the 4-step units of the gradient
    GEMM (1 .. 5, 63 .. 66, 128, 129, 192, 257 steps)."""
    m, audio = _wide_model(64, T, 3, seed=T)
    _check_against_oracle(m, audio)


def test_long_clip():
    """D = 128 at the full clip length of BASELINE configs[4] (T = 16000), four clips against the C oracle."""
    m, audio = _wide_model(128, 16000, 4, seed=5)
    _check_against_oracle(m, audio, nthreads=16)


def test_config5_float32_full_size_properties():
    """BASELINE configs[4] in float32 at full size (D=128, T=16000, 512 clips; 25 GB of workspace): finite results, the loss
    sum the reverse path reports equals the sum of the forward's per-clip losses, and the clip order does not matter (clips are
    processed in pairs: permuting the batch must permute the per-clip losses exactly and leave the gradient sums unchanged up
    to float32 summation order)."""
    from audio_mps_amd.scan import unpack_grad
    m, audio = _wide_model(128, 16000, 512, seed=4)
    per = m.loss_per_clip()
    flat, _ = strict_grad_sums(m)
    g = unpack_grad(flat.cpu().numpy(), 128)
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat.cpu().numpy()))
    assert abs(g["loss_sum"] - float(np.sum(per, dtype=np.float64))) <= 1e-5 * max(abs(g["loss_sum"]), 1.0)
    perm = np.random.default_rng(0).permutation(512)
    per2 = m.loss_per_clip(audio[perm])
    np.testing.assert_array_equal(per2, per[perm])
    flat2, _ = strict_grad_sums(m, audio[perm])
    g2 = unpack_grad(flat2.cpu().numpy(), 128)
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        assert rel_inf(g2[k], g[k]) <= 1e-5, k


@pytest.mark.parametrize("D", [64, 96, 128])
def test_wide_matches_block(D):
    """The wide kernels against the block-per-clip kernels (plain fp32 FMA code throughout): same arithmetic up to float32
    summation order; states from the wide stash layout."""
    mw, audio = _wide_model(D, 500, 5, seed=D)
    mb, _ = _wide_model(D, 500, 5, seed=D, variant=BLOCK)
    pw, pb = mw.loss_per_clip(), mb.loss_per_clip()
    assert np.max(np.abs(pw - pb) / np.maximum(np.abs(pb), 1.0)) <= LOSS_RTOL
    fw, fb = strict_grad_sums(mw)[0].cpu().numpy(), strict_grad_sums(mb)[0].cpu().numpy()
    assert rel_inf(fw[:2 * D * D], fb[:2 * D * D]) <= GRAD_RTOL
    assert rel_inf(fw[2 * D * D:2 * D * D + D], fb[2 * D * D:2 * D * D + D]) <= GRAD_RTOL
    sw, sb = mw.psi_evolve_with_data(), mb.psi_evolve_with_data()
    assert sw.shape == (5, 499, D) and np.max(np.abs(sw - sb)) < 1e-5
    np.testing.assert_allclose(np.sum(np.abs(sw) ** 2, axis=-1), 1.0, rtol=1e-5)      # tests/test_model.py:115-122


def test_rank1_option_two_pieces():
    """CMPS_OPT_RANK1 = BF16X2 selects two bf16 pieces / three products in the gradient GEMM (16 operand bits): still inside the
    gradient bar, and different bits from the default three-piece product."""
    from audio_mps_amd.scan import HipScan
    m3, audio = _wide_model(64, 400, 4, seed=9)
    m3._get_backend().set_rank1(2)
    m2, _ = _wide_model(64, 400, 4, seed=9)
    m2._get_backend().set_rank1(1)
    _check_against_oracle(m2, audio)
    f3, f2 = strict_grad_sums(m3)[0].cpu().numpy(), strict_grad_sums(m2)[0].cpu().numpy()
    assert not np.array_equal(f3[:2 * 64 * 64], f2[:2 * 64 * 64])
    assert rel_inf(f2[:2 * 64 * 64], f3[:2 * 64 * 64]) <= GRAD_RTOL


@pytest.mark.parametrize("D,T,B,sigma", [
    (64, 300, 4, 1e-4), (96, 260, 3, 1e-4), (128, 200, 4, 1e-4), (100, 100, 1, 1e-4), (40, 131, 5, 1e-4),
    (64, 257, 3, 1.0), (128, 130, 2, 1.0), (64, 2, 3, 1e-4), (64, 5, 2, 1e-4), (64, 66, 3, 1e-4), (64, 130, 1, 1e-4),
])
def test_rank1_option_f16x2(D, T, B, sigma):
    """CMPS_OPT_RANK1 = F16X2: two fp16 pieces per operand (scaled by a power of two per pair of clips), three products on
    v_mfma_f32_32x32x16_f16 -- inside the unchanged float32 bars at the three padded sizes, odd batches, sigma = 1 and around the
    unit / chunk boundaries."""
    m, audio = _wide_model(D, T, B, sigma=sigma, seed=D + T)
    be = m._get_backend()
    assert be.rank1 == 4 and be.effective_rank1 == 3             # a new handle: DEFAULT = F16X2 on the wide kernels
    _, flat_default = _check_against_oracle(m, audio)
    be.set_rank1(3)
    assert be.rank1 == 3 and be.effective_rank1 == 3
    np.testing.assert_array_equal(strict_grad_sums(m)[0].cpu().numpy(), flat_default)
    be.set_rank1(2)                                               # three bf16 pieces stay selectable
    _check_against_oracle(m, audio)
    assert not np.array_equal(strict_grad_sums(m)[0].cpu().numpy()[:2 * D * D], flat_default[:2 * D * D])


def test_rank1_f16x2_accuracy_class():
    """The gate VERDICT r3 item 3 put on the fp16 split: on the gradient GEMM's sums its distance to the float64 restatement of the
    float32 time grid (f64t32, so that no mode's distance is padded by the f64 twin's different time grid) is at most 4 x BF16X3's, and it sits at least 8 x closer to BF16X3 than BF16X2 does (all three share every other instruction, so the
    differences isolate the product arithmetic).  Short clips: with few accumulations per sum the product arithmetic is what shows
    (at T >= 2000 float32 accumulation noise of ~1e-5, common to all modes, covers it: scripts/rank1_accuracy_wide.py).  Small and
    large amplitudes exercise the power-of-two operand scales."""
    from _util import c_oracle_run
    from oracle import c_oracle as C
    from audio_mps_amd.scan import unpack_grad
    for D, T, B, amp in ((128, 33, 2, 1.0), (128, 9, 3, 1e-3), (64, 33, 2, 4.0), (96, 129, 4, 1.0), (128, 33, 2, 1e-6)):
        m, audio = _wide_model(D, T, B, seed=T + B)
        audio = (audio * np.float32(amp)).astype(np.float32)
        ref = C.unpack_grad(c_oracle_run(m, audio, "f64t32", nthreads=8)["grad"], D)["Rbar"]
        ref64 = C.unpack_grad(c_oracle_run(m, audio, "f64", nthreads=8)["grad"], D)["Rbar"]
        out = {}
        for mode in (1, 2, 3):
            m._get_backend().set_rank1(mode)
            out[mode] = unpack_grad(strict_grad_sums(m, audio)[0].cpu().numpy(), D)["Rbar"].astype(np.complex128)
        assert all(np.all(np.isfinite(v)) for v in out.values()) and np.all(np.isfinite(ref))
        e = {mode: rel_inf(out[mode], ref) for mode in out}
        e64 = {mode: rel_inf(out[mode], ref64) for mode in out}
        d2, d3 = rel_inf(out[1], out[2]), rel_inf(out[3], out[2])
        print(f"D {D} T {T} amp {amp}: vs f64t32  bf16x2 {e[1]:.2e}  bf16x3 {e[2]:.2e}  f16x2 {e[3]:.2e};  to bf16x3: bf16x2 {d2:.2e}  f16x2 {d3:.2e}")
        elastic_check(f"D {D} T {T} amp {amp} f16x2 vs 4 x bf16x3", e[3], 4 * e[2], e64[3], 4 * e64[2])
        assert 8 * d3 <= d2, (D, T, amp, d2, d3)


@pytest.mark.parametrize("D,length,n,variant", [(33, 150, 2, WIDE), (64, 300, 5, WIDE), (96, 200, 3, AUTO), (128, 260, 4, WIDE), (128, 65, 1, WIDE),
                                                (128, 130, 3, 3)])
def test_sampling_matches_oracle(D, length, n, variant):
    """PsiCMPS.sample (model.py:242-251) above D = 32: the wide chain's sampling mode (k_sample_wide; also what the bf16 pair variant
    samples with) against the numpy oracle and the block sampler, even and odd path counts, lengths around the 64-step noise chunks."""
    from oracle import cmps_oracle as O
    from _util import oracle_hparams, oracle_variables
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    m = PsiCMPS(hp, seed=D, backend=HipScan(D, variant=variant))
    mb = PsiCMPS(hp, seed=D, backend=HipScan(D, variant=BLOCK))
    for mm in (m, mb):
        mm.variables["Rx"] *= np.float32(0.03)
        mm.variables["Ry"] *= np.float32(0.03)
    noise = O.sample_noise(oracle_hparams(hp), n, length, temp=0.5, seed=D)
    ref = O.psi_sample(oracle_hparams(hp), oracle_variables(m), noise)
    out = m.sample(n, length, noise=noise)
    assert out.shape == (n, length) and np.all(np.isfinite(out))
    scale = max(1.0, np.max(np.abs(ref)))
    assert np.max(np.abs(out - ref)) <= 2e-5 * scale
    assert np.max(np.abs(out - mb.sample(n, length, noise=noise))) <= 2e-5 * scale


def _mfma_chain_model(D, T, B, sigma=1e-4, seed=0, rscale=None):
    m, audio = _wide_model(D, T, B, sigma=sigma, seed=seed, rscale=rscale)
    assert m._get_backend().wide_chain == 1                      # a new handle's setting: forward and reverse chains on the matrix cores
    m._get_backend().set_wide_chain(1)
    return m, audio


@pytest.mark.parametrize("D,T,B,sigma", [(64, 300, 4, 1e-4), (96, 260, 3, 1e-4), (128, 200, 4, 1e-4), (40, 131, 5, 1e-4), (64, 257, 3, 1.0),
                                         (128, 130, 2, 1.0), (64, 2, 3, 1e-4), (64, 66, 3, 1e-4), (100, 100, 1, 1e-4)])
def test_mfma_forward_valu_reverse(D, T, B, sigma):
    """CMPS_OPT_WIDE_CHAIN = MFMA_FWD: k_fwd_chain16 with the VALU reverse scan k_bwd_wide (the A/B setting)."""
    m, audio = _wide_model(D, T, B, sigma=sigma, seed=D + T)
    m._get_backend().set_wide_chain(2)
    _check_against_oracle(m, audio)


@pytest.mark.parametrize("D,T,B,sigma", [(64, 300, 4, 1e-4), (96, 260, 3, 1e-4), (128, 200, 4, 1e-4), (40, 131, 5, 1e-4), (64, 257, 3, 1.0),
                                         (128, 130, 2, 1.0), (64, 2, 3, 1e-4), (64, 66, 3, 1e-4), (100, 100, 1, 1e-4)])
def test_valu_chain_oracle_parity(D, T, B, sigma):
    """CMPS_OPT_WIDE_CHAIN = VALU: the training forward's chain as fp32 v_pk_fma_f32 code (k_fwd_wide<SAVE>; rounds 3's form, still
    selectable) against the oracle."""
    m, audio = _wide_model(D, T, B, sigma=sigma, seed=D + T)
    m._get_backend().set_wide_chain(0)
    assert m._get_backend().wide_chain == 0
    _check_against_oracle(m, audio)
    with pytest.raises(Exception):
        m._get_backend().set_wide_chain(3)


@pytest.mark.parametrize("D,T,B,sigma", [
    (64, 300, 4, 1e-4), (96, 260, 3, 1e-4), (128, 200, 4, 1e-4),
    (33, 150, 2, 1e-4), (40, 131, 5, 1e-4), (72, 140, 3, 1e-4), (100, 100, 1, 1e-4), (127, 90, 2, 1e-4),
    (64, 257, 3, 1.0), (128, 130, 2, 1.0), (96, 150, 2, 1.0),
    (64, 2, 3, 1e-4), (64, 3, 2, 1e-4), (64, 4, 1, 1e-4), (64, 33, 2, 1e-4), (64, 34, 2, 1e-4), (64, 65, 3, 1e-4), (64, 66, 3, 1e-4), (64, 130, 2, 1e-4),
])
def test_mfma_chain_oracle_parity(D, T, B, sigma):
    """CMPS_OPT_WIDE_CHAIN = MFMA (k_fwd_chain16: the training forward's chain with fp16 x 2 split operands on the matrix cores) inside
    the unchanged float32 bars: the three padded sizes, zero-padded rows, odd batches, sigma = 1, clip lengths around the two-step
    loop, the 32-step rho chunks and the 64-step scalar chunks."""
    m, audio = _mfma_chain_model(D, T, B, sigma=sigma, seed=D + T)
    _check_against_oracle(m, audio)


def test_mfma_chain_long_clip_and_states():
    """D = 128 at T = 16000 against the C oracle, and the stashed states (psi_evolve_with_data reads the y rows the chain kernel left)
    against the VALU chain's."""
    m, audio = _mfma_chain_model(128, 16000, 4, seed=5)
    _check_against_oracle(m, audio, nthreads=16)
    m2, audio2 = _mfma_chain_model(96, 400, 3, seed=8)
    mv, _ = _wide_model(96, 400, 3, seed=8)
    mv._get_backend().set_wide_chain(0)
    strict_grad_sums(m2); strict_grad_sums(mv)
    s2, sv = m2.psi_evolve_with_data(), mv.psi_evolve_with_data()
    assert s2.shape == sv.shape and np.max(np.abs(s2 - sv)) < 1e-5
    pm, pv = m2.loss_per_clip(), mv.loss_per_clip()           # (the forward-only path is the VALU kernel in both)
    np.testing.assert_array_equal(pm, pv)


@pytest.mark.parametrize("T", [5, 8, 9, 10, 16, 17, 31, 32, 33, 34, 63, 64, 65, 66, 67, 129, 257])
def test_mfma_chain_block_boundaries(T):
    """T - 1 steps around the reverse scan's eight-step blocks, the 32-step rho chunks and the 64-step scalar chunks, D = 96 (three waves)."""
    m, audio = _mfma_chain_model(96, T, 3, seed=T)
    _check_against_oracle(m, audio)


def test_mfma_chain_vector_scale_jumps():
    """The reverse scan's per-step vector scale: audio with silent stretches, clicks and a 1e4 x amplitude step (ybar changes by orders
    of magnitude from one step to the next; a wrong bound would overflow the fp16 pieces: inf / NaN), both clips different."""
    from audio_mps_amd.scan import unpack_grad
    from oracle import c_oracle as C
    rng = np.random.default_rng(7)
    m, audio = _mfma_chain_model(128, 400, 4, seed=11)
    audio = audio.copy()
    audio[0, :150] = 0.0                                          # silence, then the signal
    audio[1, 200:] *= np.float32(1e-4)                            # a loud start, then nearly nothing
    audio[2] = 0.0
    audio[2, 100] = 0.3; audio[2, 101] = -0.2; audio[2, 300] = 0.25      # clicks
    audio[3] = (1e-3 * rng.standard_normal(400)).astype(np.float32)
    audio[3, 250:] *= np.float32(100.0)
    ref = c_oracle_run(m, audio, "f32")
    assert np.all(np.isfinite(ref["loss_per_clip"]))
    flat = strict_grad_sums(m, audio)[0].cpu().numpy()
    assert np.all(np.isfinite(flat))
    g, gr = unpack_grad(flat, 128), C.unpack_grad(ref["grad"], 128)
    assert abs(g["loss_sum"] - gr["loss_sum"]) <= LOSS_RTOL * max(abs(gr["loss_sum"]), 4.0)
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        assert rel_inf(g[k], gr[k]) <= GRAD_RTOL, k


def test_mfma_chain_operand_scales():
    """The power-of-two operand scales: tiny and large R (entries 1e-6 .. 30 x the usual), loud audio (large |s| |R|), against the oracle."""
    for rscale, amp, seed in ((1e-6, 1.0, 1), (3.0, 0.05, 2), (0.35, 8.0, 3), (1e-3, 300.0, 4)):
        m, audio = _mfma_chain_model(128, 150, 2, seed=seed, rscale=rscale)
        audio = (audio * np.float32(amp)).astype(np.float32)
        ref = c_oracle_run(m, audio, "f32")
        if not np.all(np.isfinite(ref["loss_per_clip"])):
            continue
        from audio_mps_amd.scan import unpack_grad
        from oracle import c_oracle as C
        flat = strict_grad_sums(m, audio)[0].cpu().numpy()
        g, gr = unpack_grad(flat, 128), C.unpack_grad(ref["grad"], 128)
        assert abs(g["loss_sum"] - gr["loss_sum"]) <= LOSS_RTOL * max(abs(gr["loss_sum"]), 2.0), (rscale, amp)
        for k in ("Rbar", "fbar", "psi0bar", "Abar"):
            assert rel_inf(g[k], gr[k]) <= GRAD_RTOL, (rscale, amp, k)


def test_bit_reproducible():
    m, audio = _wide_model(96, 300, 5, seed=4)
    a = strict_grad_sums(m)[0].cpu().numpy().copy()
    pa = m.loss_per_clip().copy()
    for _ in range(3):
        m2, _ = _wide_model(96, 300, 5, seed=4)
        np.testing.assert_array_equal(strict_grad_sums(m2)[0].cpu().numpy(), a)
        np.testing.assert_array_equal(m2.loss_per_clip(), pa)


def test_normalisation_floor_branch():
    """|y|^2 <= 1e-12 takes the floor branch of model.py:332 in the forward and in the adjoint (ok = 0: no projection)."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    D, T, B = 64, 40, 2
    hp = HParams(minibatch_size=B, bond_dim=D)
    audio = make_audio(B, T, hp.delta_t, 3)
    m = PsiCMPS(hp, data_iterator=audio, seed=1, backend=HipScan(D, variant=WIDE))
    m.variables["psi_x"] *= np.float32(0)          # psi_0 = 0 / sqrt(max(0, 1e-12)) = 0: every step is below the floor
    m.variables["psi_y"] *= np.float32(0)
    per = m.loss_per_clip()
    assert np.all(per == 0.0)
    flat = strict_grad_sums(m)[0].cpu().numpy()
    assert np.all(np.isfinite(flat))
