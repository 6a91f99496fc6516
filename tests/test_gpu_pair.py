"""The MFMA pair kernels (32 < D <= 128, instantiated for the padded dimensions 64, 96, 128; CMPS_VARIANT_PAIR: bf16 mat-vec operands, float32 accumulation; BASELINE configs[4] is D = 128).

Two comparisons, two tolerances (stated here, derived from oracle-vs-oracle distances measured on the CPU):
  * against oracle.psi_bf16_scan, which restates the SAME reduced-precision arithmetic (same rounding points):
      per-clip loss 3e-4 * max(|loss|, 1), gradients 2e-3 of each tensor's max.  It is not tighter because a float32
      difference of 1e-7 occasionally flips a bf16 rounding (2^-9 relative), after which the two trajectories drift.
  * against the float32 restatement (the reference's arithmetic): per-clip loss 2e-3, gradients 3e-2 -- the cost of
      bf16 operands, the same distance the bf16 emulation itself has from float32 (tests/test_oracle.py).
"""
import numpy as np
import pytest

from oracle import cmps_oracle as O
from oracle import c_oracle as C
from _util import (c_oracle_run, make_audio, oracle_hparams, oracle_variables, rel_inf, strict_grad_sums,
                   strict_loss_and_grads)

pytestmark = pytest.mark.gpu
PAIR = 3


def _pair_model(T, B, seed=3, D=128, **hpkw):
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D, **hpkw)
    audio = make_audio(B, T, hp.delta_t, seed + 4)
    return PsiCMPS(hp, data_iterator=audio, seed=seed, backend=HipScan(D, variant=PAIR)), audio


@pytest.mark.parametrize("D,T,B", [(128, 2, 2), (128, 40, 2), (128, 65, 1), (128, 200, 4), (128, 300, 5),
                                   (64, 3, 1), (64, 130, 3), (64, 300, 6), (96, 150, 4),
                                   (40, 60, 3), (100, 70, 3),         # 40 and 100 run zero-padded to 64 and 128
                                   (128, 9, 2), (128, 17, 3), (64, 10, 2), (96, 8, 1)])   # one / two whole eight-step batches, 9 and 7 steps
def test_pair_matches_bf16_oracle_and_float32(D, T, B):
    from audio_mps_amd.scan import unpack_grad
    m, audio = _pair_model(T, B, D=D)
    assert m._get_backend().variant == PAIR
    per = m.loss_per_clip()
    flat, _ = strict_grad_sums(m)
    g = unpack_grad(flat.cpu().numpy(), D)
    em = O.psi_bf16_scan(oracle_hparams(m.hparams), oracle_variables(m), audio, want_grad=True)
    ref = c_oracle_run(m, audio, "f32", want_grad=True)
    gr = C.unpack_grad(ref["grad"], D)
    den = np.maximum(np.abs(ref["loss_per_clip"]), 1.0)
    assert np.max(np.abs(per - em["loss_per_clip"]) / den) <= 3e-4
    assert np.max(np.abs(per - ref["loss_per_clip"]) / den) <= 2e-3
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        assert rel_inf(g[k], em[k]) <= 2e-3, k
        assert rel_inf(g[k], gr[k]) <= 3e-2, k
    assert abs(g["loss_sum"] - float(np.sum(per, dtype=np.float64))) <= 1e-4 * max(1.0, abs(g["loss_sum"]))


@pytest.mark.parametrize("D,T,rs,sigma", [(40, 60, 0.6, 0.36), (64, 130, 0.6, 0.36), (128, 90, 0.5, 0.36), (96, 257, 0.6, 0.5), (128, 33, 0.7, 0.3)])
def test_pair_qbar_sums_visible_at_large_sigma(D, T, rs, sigma):
    """no case of this file had sigma > 1e-4, where Q = -(delta_t sigma^2 / 2) R^dagger R (/root/reference/model.py:312)
    is below float32 resolution and errors in Qbar = sum ybar u^dagger never reach a gradient.  sigma = 0.3 ... 0.5, A = 66, quiet audio and
    a large R make Q carry 14 ... 50 % of the R gradient; the pair kernels (k_bwd_pair + k_grad_gemm<1>) against the bf16-emulating
    oracle at this file's bars, and against the float32 restatement at its bf16 bars."""
    from audio_mps_amd.scan import unpack_grad
    B = 3
    m, _ = _pair_model(T, B, D=D, seed=7, sigma=sigma, A=66.0)
    audio = (make_audio(B, T, m.hparams.delta_t, 3) * np.float32(0.09)).astype(np.float32)
    m.variables["Rx"] *= np.float32(rs)
    m.variables["Ry"] *= np.float32(rs)
    per = m.loss_per_clip(audio)
    g = unpack_grad(strict_grad_sums(m, audio)[0].cpu().numpy(), D)
    em = O.psi_bf16_scan(oracle_hparams(m.hparams), oracle_variables(m), audio, want_grad=True)
    ref = c_oracle_run(m, audio, "f32", want_grad=True)
    gr = C.unpack_grad(ref["grad"], D)
    # Q is visible: the same model at sigma = 1e-4 has a different R gradient by >= 10 %
    small = C.unpack_grad(C.psi_scan(audio, *_eff(m), float(m.A), m.hparams.delta_t, 1e-4, "f32", want_grad=True)["grad"], D)
    assert rel_inf(small["Rbar"], gr["Rbar"]) >= 0.1
    den = np.maximum(np.abs(ref["loss_per_clip"]), 1.0)
    assert np.max(np.abs(per - em["loss_per_clip"]) / den) <= 3e-4
    assert np.max(np.abs(per - ref["loss_per_clip"]) / den) <= 2e-3
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        assert rel_inf(g[k], em[k]) <= 2e-3, (k, rel_inf(g[k], em[k]))
        assert rel_inf(g[k], gr[k]) <= 3e-2, (k, rel_inf(g[k], gr[k]))


def _eff(m):
    ohp, ov = oracle_hparams(m.hparams), oracle_variables(m)
    R, f, _, _ = O.effective_params(ohp, ov, "f32")
    return R, f, O.psi_0(ov, "f32")


def test_pair_agrees_with_block_variant_at_reduced_c5():
    """BASELINE configs[4] at reduced length and batch: the MFMA path against the float32 block kernels on the GPU."""
    from audio_mps_amd import PsiCMPS
    from audio_mps_amd.scan import HipScan
    m, audio = _pair_model(1000, 8, seed=5)
    blk = PsiCMPS(m.hparams, data_iterator=audio, seed=5, backend=HipScan(128, variant=1))
    for k in m.variables:
        blk.variables[k] = m.variables[k].copy()
    a, b = m.loss_per_clip(), blk.loss_per_clip()
    assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) <= 2e-3
    la, ga = strict_loss_and_grads(m)
    lb, gb = strict_loss_and_grads(blk)
    assert abs(float(la) - float(lb)) <= 2e-3 * max(1.0, abs(float(lb)))
    for k in ga:
        assert rel_inf(ga[k], gb[k]) <= 5e-2, k


def test_pair_training_reduces_the_loss():
    from audio_mps_amd.train import Trainer
    m, _ = _pair_model(300, 6, seed=2, learning_rate=1e-2)
    tr = Trainer(m, m.hparams)
    losses = [tr.step()["total_loss"] for _ in range(12)]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_pair_variant_rules():
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import HipScan
    with pytest.raises(_capi.CmpsError) as ei:
        HipScan(16, variant=PAIR)                      # the MFMA pair kernels are for 32 < D <= 128
    assert ei.value.code == _capi.CMPS_ERR_UNSUPPORTED_D
    assert HipScan(128).variant == 5 and HipScan(64).variant == 5   # AUTO stays float32 (the wide kernels): the bf16-operand path is opt-in


@pytest.mark.parametrize("D,B", [(128, 3), (72, 2)])
def test_pair_states_remain_normalized_and_match_block_variant(D, B):
    """psi_evolve_with_data (tests/test_model.py:115-122) from the pair kernels' stash layout."""
    from audio_mps_amd import PsiCMPS
    from audio_mps_amd.scan import HipScan
    m, audio = _pair_model(90, B, D=D)
    psi = m.psi_evolve_with_data()
    assert psi.shape == (B, 89, D)
    np.testing.assert_allclose(np.sum(np.abs(psi) ** 2, axis=2), np.ones((B, 89)), rtol=1e-5)
    blk = PsiCMPS(m.hparams, data_iterator=audio, seed=3, backend=HipScan(D, variant=1))
    for k in m.variables:
        blk.variables[k] = m.variables[k].copy()
    assert rel_inf(psi, blk.psi_evolve_with_data()) <= 5e-3


def test_config5_full_length_reduced_batch():
    """BASELINE configs[4] (D=128, T=16000) at 4 clips against the float32 restatement.  Over 16 000 steps the bf16 operand
    rounding accumulates to ~2e-3 of the per-clip loss (the bf16 emulation itself is 1.8e-3 away from float32 here), so the
    bar is 5e-3 for the loss and 6e-2 of each gradient tensor's max."""
    from audio_mps_amd.scan import unpack_grad
    m, audio = _pair_model(16000, 4, seed=2)
    per = m.loss_per_clip()
    flat, _ = strict_grad_sums(m)
    g = unpack_grad(flat.cpu().numpy(), 128)
    ref = c_oracle_run(m, audio, "f32", want_grad=True, nthreads=4)
    gr = C.unpack_grad(ref["grad"], 128)
    den = np.maximum(np.abs(ref["loss_per_clip"]), 1.0)
    assert np.max(np.abs(per - ref["loss_per_clip"]) / den) <= 5e-3
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        assert rel_inf(g[k], gr[k]) <= 6e-2, k


def test_config5_full_size_properties():
    """BASELINE configs[4] at full size (D=128, T=16000, 512 clips; 16.8 GB of stash): finite results, the loss sum the
    reverse path reports equals the sum of the forward's per-clip losses, and the clip order does not matter (clips are
    processed in pairs: permuting the batch must permute the per-clip losses and leave the gradient sums unchanged)."""
    import torch
    from audio_mps_amd.scan import unpack_grad
    m, audio = _pair_model(16000, 512, seed=4)
    per = m.loss_per_clip()
    flat, _ = strict_grad_sums(m)
    g = unpack_grad(flat.cpu().numpy(), 128)
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat.cpu().numpy()))
    assert abs(g["loss_sum"] - float(np.sum(per, dtype=np.float64))) <= 1e-4 * abs(g["loss_sum"])
    perm = np.random.default_rng(0).permutation(512)
    per2 = m.loss_per_clip(audio[perm])
    np.testing.assert_allclose(per2, per[perm], rtol=1e-6, atol=1e-6)
    flat2, _ = strict_grad_sums(m, audio[perm])
    g2 = unpack_grad(flat2.cpu().numpy(), 128)
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        assert rel_inf(g2[k], g[k]) <= 1e-4, k
