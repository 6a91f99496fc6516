"""The forward chain wave's serial tail on rotated partials (cmps_wave2.hip::rot_tail_bcast).

The mat-vec of a chain step leaves a complex partial sum per lane and K-half.  The tail used to combine the halves (one lane exchange)
and then fetch the partner component for the rotation (a second one, on the same dependency chain); now the identity term joins the
lane's own slot of the partial (a masked packed FMA), the rotation is applied to the partial pair, and one exchange each lands z_k (the
ring row) and rho_k z_k (the next broadcast) in split layout.  Same algebra, rounding points moved: every bar below is an existing one
(tests/test_gpu_parity.py, tests/test_gpu_norm_stash.py, tests/_states_ref.py), built the way those tests build them.  The gradient
cases run the two-wave reverse scan on the forward's rows and compare it with the oracle and the one-wave scan, so they also stand for
the same tail in the reverse chain wave, whose fbar and psi0bar formulas would follow it."""
import numpy as np
import pytest

from oracle import c_oracle as C
from oracle import cmps_oracle as O
from _util import c_oracle_run, elastic_check, make_audio, rel_inf, strict_grad_sums
import _states_ref as SR

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-4                  # tests/test_gpu_parity.py
LOSS_RTOL = 1e-5
WAVE = 2
KEYS = ("Rbar", "fbar", "psi0bar", "Abar")
CH2 = 32                          # steps per chunk of the forward chain wave (cmps_wave2.hip)


def _set(be, option, value):
    from audio_mps_amd import _capi
    _capi.check(be._h, be._lib.cmps_set_option(be._h, option, value))


def _saved_rows(be):
    from audio_mps_amd import _capi
    return be._lib.cmps_get_option(be._h, _capi.CMPS_OPT_SAVED_ROWS)


def _grads(m, audio, waves):
    """(unpacked gradient sums, kernel names, CMPS_OPT_SAVED_ROWS after the pass) with CMPS_OPT_BWD_WAVES = waves"""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import unpack_grad
    be = m._get_backend()
    _set(be, _capi.CMPS_OPT_BWD_WAVES, waves)
    be.kernel_events(True)
    try:
        flat = strict_grad_sums(m, audio)[0].cpu().numpy()
        names = set(be.kernel_times())
    finally:
        be.kernel_events(False)
    assert np.all(np.isfinite(flat))
    return unpack_grad(flat, m.bond_d), names, _saved_rows(be)


def _oracle(m, audio):
    """(float32 oracle's per-clip loss, its gradient, the f64t32 and f64 gradients)"""
    D = m.bond_d
    ref = c_oracle_run(m, audio, "f32")
    return (ref["loss_per_clip"], C.unpack_grad(ref["grad"], D),
            *(C.unpack_grad(c_oracle_run(m, audio, d)["grad"], D) for d in ("f64t32", "f64")))


def _check_grads(label, g, other, gr, gt, g64):
    for k in KEYS:
        bar, bar64 = max(GRAD_RTOL, 3 * rel_inf(gr[k], gt[k])), max(GRAD_RTOL, 3 * rel_inf(gr[k], g64[k]))
        e = rel_inf(g[k], other[k])
        elastic_check(f"{k} {label}", e, bar, e, bar64)


def _check_loss(m, audio, ref_per):
    be = m._get_backend()
    be.kernel_events(True)
    try:
        per = m.loss_per_clip(audio)
        names = set(be.kernel_times())
    finally:
        be.kernel_events(False)
    assert "k_fwd_wave2" in names, names
    assert np.all(np.isfinite(ref_per)) and np.all(np.isfinite(per))
    err = np.abs(per - ref_per) / np.maximum(np.abs(ref_per), 1.0)
    print(f"loss per clip: max rel err {np.max(err):.3e} (bar {LOSS_RTOL:.0e})")
    assert np.max(err) <= LOSS_RTOL, err


def _both_scans_against_oracle(m, audio):
    lr, gr, gt, g64 = _oracle(m, audio)
    _check_loss(m, audio, lr)
    g2, names2, rows2 = _grads(m, audio, 2)
    assert "k_fwd_wave2" in names2 and "k_bwd_wave2w" in names2, names2
    assert rows2 == 1                            # normalised rows: the NORM instances of both kernels
    g1, names1, _ = _grads(m, audio, 1)
    assert "k_bwd_wave" in names1 and "k_bwd_wave2w" not in names1, names1
    _check_grads("vs oracle", g2, gr, gr, gt, g64)
    _check_grads("vs one wave", g2, g1, gr, gt, g64)


# N = T - 1: step 0 alone; a lone top octet; octet boundaries (8, 9); the 32-step chunk boundary from both sides (31, 32, 33: the forward's
# rescale enters at a chunk boundary, the partial last chunk runs the counted loop); 64 / 65: a 64-step scalar chunk boundary; 130
@pytest.mark.parametrize("N", [1, 2, 8, 9, 31, 32, 33, 64, 65, 130])
@pytest.mark.parametrize("B", [1, 5])          # ragged against four clips per workgroup
@pytest.mark.parametrize("D", [17, 32])        # D = 17: padded rows and columns stay exact zeros through the masked add and the rotated combine
def test_gradient_and_loss_match_oracle_and_one_wave(D, B, N):
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D, sigma=1e-4)
    audio = make_audio(B, N + 1, hp.delta_t, D + N)
    if B >= 3:
        audio[2] = audio[2, 0]                   # a constant clip between ordinary ones (tests/test_gpu_norm_stash.py)
    m = PsiCMPS(hp, data_iterator=audio, seed=D + N, backend=HipScan(D, variant=WAVE))
    _both_scans_against_oracle(m, audio)


def test_freqs_and_psi0_cotangents_visible():
    """sigma = 0.36, R x 0.69, A = 66, audio x 0.09 (the sigma-visible cases of tests/test_gpu_parity.py): fbar and psi0bar, the two
    outputs whose formula follows the tail, are not dominated by the other terms.  D = 32, B = 3, N = 65."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    D, B, T = 32, 3, 66
    hp = HParams(minibatch_size=B, bond_dim=D, sigma=0.36, A=66.0)
    audio = (make_audio(B, T, hp.delta_t, D + T) * np.float32(0.09)).astype(np.float32)
    m = PsiCMPS(hp, data_iterator=audio, seed=D + T, backend=HipScan(D, variant=WAVE))
    m.variables["Rx"] *= np.float32(0.69)
    m.variables["Ry"] *= np.float32(0.69)
    _both_scans_against_oracle(m, audio)


@pytest.mark.parametrize("T", [34, 130])
def test_chain_state_read_out(T):
    """cmps_psi_states through the normalised rows (as tests/test_gpu_norm_stash.py::test_states_read_normalised_rows) against
    tests/_states_ref.py's f64t32 reference at its own bar: the ring row z_k and the carried state rho_k z_k still agree."""
    case = SR.PsiCase("wave32", 32, SR.WAVE32, (("rank1", SR.RANK1_DEFAULT),), T, 5, *SR.VISIBLE)
    ref, _ = SR.case_reference(case)
    m = SR.psi_model(*SR.case_inputs(case), case.variant, case.options)
    be = m._get_backend()
    psi, names = SR._with_events(be, m.psi_evolve_with_data)
    assert "k_fwd_wave2" in names, names
    assert _saved_rows(be) == 1
    assert psi.shape == ref.shape and np.all(np.isfinite(psi))
    err = SR.max_abs(psi, ref)
    print(f"{case.id}: max |hip - f64t32| {err:.3e}  bar {case.bar:.0e}")
    assert err <= case.bar


def test_rescale_in_flight():
    """tests/test_gpu_fwd_unnormalised.py::test_norm_drift_through_rescales' large-increment input (audio x 3) at N = 97, clip 1 three
    times louder still: its |z_k|^2 starts chunk 0 at 1 and has left [1, 4) before the chunk's rescale is taken (checked on the oracle's own
    float64 steps), so the chain rescales by a power of two entering chunk 1.  Loss per clip at LOSS_RTOL."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    T, B = 98, 3
    hp = HParams(minibatch_size=B, bond_dim=32, sigma=1e-4)
    audio = (make_audio(B, T, hp.delta_t, T + B) * np.float32(3.0)).astype(np.float32)
    audio[1] *= np.float32(3.0)
    m = PsiCMPS(hp, data_iterator=audio, seed=T + B, backend=HipScan(32, variant=WAVE))
    # |z_k|^2 over chunk 0 = the running product of the per-step norms n_k = |y_k|^2 (|psi_0| = 1; the chain does not normalise)
    from _util import oracle_hparams, oracle_variables
    ohp, ov = oracle_hparams(m.hparams), oracle_variables(m).astype(np.float64)
    R, freqs, _, _ = O.effective_params(ohp, ov, "f64")
    psi = O.psi_0(ov, "f64")[None, :].astype(np.complex128)
    x = (audio[1:2, 1:].astype(np.float64) - audio[1:2, :-1].astype(np.float64))
    t, z2 = np.float64(0), 1.0
    for k in range(CH2 - 2):                     # up to the step whose |z|^2 sets the rescale (CH2 - 3)
        psi = O.update_ancilla_psi(psi, x[:, k], t, R, freqs, np.float64(ov.A), ohp, "f64")
        z2 *= float(np.sum(np.abs(psi) ** 2))
        psi = O.normalize_psi(psi, axis=1, dtype="f64")
        t = t + np.float64(ohp.delta_t)
    print(f"|z|^2 of clip 1 at step {CH2 - 3}: {z2:.3e}")
    assert z2 >= 16.0                            # outside [1, 4) with a factor of four to spare: the exponent of the rescale is not 0
    ref = c_oracle_run(m, audio, "f32", want_grad=False)
    _check_loss(m, audio, ref["loss_per_clip"])
