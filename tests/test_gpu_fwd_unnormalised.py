"""k_fwd_wave2 carries the un-normalised state z_k on its chain wave and its loss wave turns the rows back into y_k = c_k z_k
(DESIGN 4.2).  Against the oracle at the bars of test_gpu_parity.py: the 1e-12 floor of the normalisation, long clips whose norm
drifts through the per-chunk power-of-two rescales, T - 1 around the 32-step chunks, the legacy arithmetic, the loss-only
forward (loss_per_clip) and the stash rows / scalars through the reverse scan's gradients (grad_sums).  Every case also checks that
no fp16-range fallback ran and that the forward ran in k_fwd_wave2."""
import numpy as np
import pytest

from oracle import cmps_oracle as O
from oracle import c_oracle as C
from _util import c_oracle_run, elastic_check, make_audio, rel_inf, strict_grad_sums

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-4


def _model(T, B, seed, sigma=1e-4, rscale=None, audio_scale=None, **hpkw):
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=32, sigma=sigma, **hpkw)
    audio = make_audio(B, T, hp.delta_t, seed)
    if audio_scale is not None:
        audio = (audio * np.float32(audio_scale)).astype(np.float32)
    m = PsiCMPS(hp, data_iterator=audio, seed=seed, backend=HipScan(32, variant=2))
    if rscale is not None:
        m.variables["Rx"] *= np.float32(rscale)
        m.variables["Ry"] *= np.float32(rscale)
    return m, audio


def _check(m, audio, elastic_bar=False):
    """HIP against the float32 oracle.  elastic_bar: the gradient bar widens to 3 x the float32 oracle's own rounding distance
    (from f64t32, float64 on the float32 time grid the kernels follow) where that is above GRAD_RTOL."""
    from audio_mps_amd.scan import unpack_grad
    be = m._get_backend()
    be.kernel_events(True)
    per = m.loss_per_clip()
    flat, B = strict_grad_sums(m)
    names = set(be.kernel_times())
    be.kernel_events(False)
    assert "k_fwd_wave2" in names, names
    assert be.f16_fallbacks == 0
    flat = flat.cpu().numpy()
    ref = c_oracle_run(m, audio, "f32")
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat))
    err = np.max(np.abs(per - ref["loss_per_clip"]) / np.maximum(np.abs(ref["loss_per_clip"]), 1.0))
    assert err <= LOSS_RTOL, f"loss rel err {err}"
    g, gr = unpack_grad(flat, 32), C.unpack_grad(ref["grad"], 32)
    if elastic_bar:
        gt = C.unpack_grad(c_oracle_run(m, audio, "f64t32")["grad"], 32)
        g64 = C.unpack_grad(c_oracle_run(m, audio, "f64")["grad"], 32)
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        e = rel_inf(g[k], gr[k])
        if elastic_bar:
            elastic_check(k, e, max(GRAD_RTOL, 3 * rel_inf(gr[k], gt[k])), e, max(GRAD_RTOL, 3 * rel_inf(gr[k], g64[k])))
        else:
            assert e <= GRAD_RTOL, (k, e, GRAD_RTOL)
    return per


@pytest.mark.parametrize("T", [2, 31, 32, 33, 34, 64, 65, 66, 96, 97, 98, 130])
def test_chunk_boundaries_32(T):
    """T - 1 = 1, 30 ... 32, 33, 63 ... 65, 95 ... 97, 129 steps: full chunks only, a lone partial last chunk, rescales between
    chunks, a clip of one step."""
    m, audio = _model(T, 5, seed=T)
    _check(m, audio)


@pytest.mark.parametrize("T,B,sigma,rscale,audio_scale,A", [
    (3000, 4, 1.0, 0.1, None, None), (1500, 5, 0.36, 0.69, 0.09, 66.0), (4000, 3, 1e-4, None, 3.0, None)])
def test_norm_drift_through_rescales(T, B, sigma, rscale, audio_scale, A):
    """Visible dissipator / large R / large increments: |z_k| drifts over many chunks and the chain rescales it by powers of two."""
    kw = {"A": A} if A is not None else {}
    m, audio = _model(T, B, seed=T + B, sigma=sigma, rscale=rscale, audio_scale=audio_scale, **kw)
    _check(m, audio, elastic_bar=True)


def test_normalisation_floor_clips():
    """|psi_0|^2 far below 1e-12: the reference's max(n, 1e-12) clips at the first step, u_1 has norm^2 n_0 / 1e-12 < 1, then the
    state recovers.  Checked against the oracle, loss-only and through the gradients."""
    m, audio = _model(100, 3, seed=11)
    m.variables["psi_x"] *= np.float32(1e-13)
    m.variables["psi_y"] *= np.float32(1e-13)
    p0 = O.psi_0(_oracle_vars(m), "f64")
    assert np.sum(np.abs(p0) ** 2) < 1e-12
    _check(m, audio)


def test_zero_state():
    """psi_0 = 0: every step clips and the state stays zero (loss 0, as the oracle has it)."""
    m, audio = _model(70, 2, seed=12)
    m.variables["psi_x"][:] = 0
    m.variables["psi_y"][:] = 0
    per = m.loss_per_clip()
    ref = c_oracle_run(m, audio, "f32", want_grad=False)
    assert np.all(np.isfinite(per))
    assert np.max(np.abs(per - ref["loss_per_clip"]) / np.maximum(np.abs(ref["loss_per_clip"]), 1.0)) <= LOSS_RTOL


def test_config3_full_T_small_batch():
    """BASELINE configs[2] at T = 16000 on 8 clips: the stash rows and scalars through the reverse scan."""
    m, audio = _model(16000, 8, seed=5)
    _check(m, audio)


@pytest.mark.parametrize("T,B", [(2, 2), (33, 3), (34, 2), (65, 4), (300, 5)])
def test_legacy_mode(T, B):
    """The legacy AudioMPS arithmetic on the same two-wave forward (k_fwd_wave2<.., LEGACY>)."""
    from audio_mps_amd import LegacyAudioMPS
    dt = 0.005
    audio = make_audio(B, T, dt, 300 + T, noise=0.05)
    m = LegacyAudioMPS(32, dt, B, data_iterator=audio, seed=T)
    ref = O.legacy_loss_and_grads(m.variables["H"], m.variables["R"], dt, audio, "f32")
    per = m.loss_per_clip()
    _, grads = m.loss_and_grads()
    assert np.max(np.abs(per - ref["per_clip"]) / np.maximum(np.abs(ref["per_clip"]), 1)) <= LOSS_RTOL
    assert max(rel_inf(grads["R"], ref["gR"]), rel_inf(grads["H"], ref["gH"])) <= GRAD_RTOL


def _oracle_vars(m):
    from _util import oracle_variables
    return oracle_variables(m)
