"""The loop from scan to raw gradient, closed on the device: ONE step of a fresh Trainer(device_step=True) -- parameter tables, forward
scan, reverse scan, cmps_psi_apply_step / cmps_rho_apply_step -- leaves m = 0.1f g in the first-moment slots, so m / 0.1f is the
device's gradient of the total loss w.r.t. every raw variable.  It is compared with the float64 oracle's end-to-end gradient on the
float32 time grid ("f64t32", with_reg=True), which tests/test_host.py asserts on the CPU only, with the oracle standing in for the
kernels.  The bars are the sweep's (tests/_sweep.py) and none is new: per tensor max(GRAD_BAR, 2 x the float32 restatement's own
distance from f64t32), as sweep_rho prices it; _dA_bar for A; the total loss at LOSS_BAR.

Measured on an MI355X (every bar stood at its floor, 1e-4 / 1e-5): total loss at most 6.4e-8; gradients, as fractions of the tensor's
max, at most 1.3e-6 (psi_x at D = 8), 8.9e-7 for RhoCMPS (Wy at D = 40), A at most 3.6e-7.  The R gradients sit at 1e-7: with the
default r_reg their largest entries are the regulariser's."""
import numpy as np
import pytest

import _step_ref as R
from _sweep import GRAD_BAR, LOSS_BAR, _dA_bar
from _util import make_audio, oracle_hparams, oracle_variables, rel_inf
from oracle import cmps_oracle as O

pytestmark = pytest.mark.gpu

T, B = 96, 3


def _first_step(model, hp):
    """One device-resident step from zero slots -> ({variable: float32 gradient read back from m}, total loss)."""
    from audio_mps_amd import _capi
    from audio_mps_amd.train import Trainer
    t = Trainer(model, hp, device_step=True)
    out = t.step()
    be = model._get_backend()
    assert be.f16_fallbacks == 0
    if not hasattr(model, "rank_rho_0"):               # (cmps_psi_grad_status reads the status words of cmps_psi_loss_bwd; the rho scans have none)
        assert be.grad_status()[0] == _capi.CMPS_OK
    t.sync_to_host()
    assert t.opt.t == 1 and np.isfinite(out["total_loss"])
    return {k: t.opt.m[k] / np.float32(0.1) for k in t.opt.m}, out["total_loss"]


def _check(label, got, total, ref, ref32, names):
    fails = []
    e = abs(total - float(ref["loss"])) / max(abs(float(ref["loss"])), 1.0)
    print(f"{label} total loss: {e:.2e} (bar {LOSS_BAR:.1e})")
    if not e <= LOSS_BAR:
        fails.append(("total", e, LOSS_BAR))
    for k in names:
        e = rel_inf(got[k], ref[k])
        bar = _dA_bar(ref32[k], ref[k], GRAD_BAR) if k == "A" else max(GRAD_BAR, 2.0 * rel_inf(ref32[k], ref[k]))
        print(f"{label} d/d{k}: {e:.2e} of the tensor's max (bar {bar:.2e})")
        if not e <= bar:
            fails.append((k, e, bar))
    assert not fails, (label, fails)


@pytest.mark.parametrize("D", [8, 24, 40])             # the 16-row wave kernels | the two-wave (32-row) kernels | the wide kernels
def test_psi_device_step_gradient_matches_float64_oracle(D):
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D, learning_rate=0.01)
    data = make_audio(B, T, hp.delta_t, 11)
    m = PsiCMPS(hp, data_iterator=data, seed=2, backend=HipScan(D))
    if D > 32:
        m.variables["Rx"] *= np.float32(0.5)
        m.variables["Ry"] *= np.float32(0.5)
    ohp, ov = oracle_hparams(hp), oracle_variables(m)
    ref, ref32 = (O.psi_loss_and_grads(ohp, ov.astype(np.float64) if d != "f32" else ov, data, d, with_reg=True) for d in ("f64t32", "f32"))
    as_dict = lambda g: {**{k: getattr(g, k) for k in O.Variables.NAMES}, "loss": g.loss}
    got, total = _first_step(m, hp)
    _check(f"psi D={D}", got, total, as_dict(ref), as_dict(ref32), O.Variables.NAMES)


@pytest.mark.parametrize("D,rank", [(6, 3), (40, 5)])  # the column kernels | the general kernels above D = 32
def test_rho_device_step_gradient_matches_float64_oracle(D, rank):
    """O.rho_loss_and_grads returns the model loss alone: the regularisers' value and gradient come from tests/_step_ref.py (the
    float64 autograd restatement with zero cotangents)."""
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=rank, learning_rate=0.01)
    data = make_audio(B, T, hp.delta_t, 12)
    m = RhoCMPS(hp, data_iterator=data, seed=2, backend=HipScan(D))
    if D > 32:
        m.variables["Rx"] *= np.float32(0.5)
        m.variables["Ry"] *= np.float32(0.5)
    ov = O.Variables(np.asarray(m.variables["A"], np.float32), m.variables["Rx"], m.variables["Ry"], m.variables["freqs"],
                     np.zeros(D, np.float32), np.zeros(D, np.float32), scaled_R=True, scaled_freqs=True)
    ohp = O.HParams(**hp.values())
    ref = O.rho_loss_and_grads(ohp, ov.astype(np.float64), m.variables["Wx"].astype(np.float64), m.variables["Wy"].astype(np.float64),
                               data, "f64t32")
    ref32 = O.rho_loss_and_grads(ohp, ov, m.variables["Wx"], m.variables["Wy"], data, "f32")
    reg, reg_grads = R.total_and_grads(m.variables, np.zeros(m.flat_size()), 1, m.h_reg, m.r_reg, float(m._c_r), float(m._c_h), rank, True)
    with_reg = lambda g: {**{k: np.asarray(g[k], dtype=np.float64) + reg_grads[k] for k in m.VARIABLE_NAMES}, "loss": float(g["loss"]) + reg}
    got, total = _first_step(m, hp)
    _check(f"rho D={D} rank={rank}", got, total, with_reg(ref), with_reg(ref32), m.VARIABLE_NAMES)
