"""cmps_rho_apply_step on the GPU: the optimiser half of a RhoCMPS training step (chain rule of model.py:36-42, 49, 119-132 +
regularisers train.py:55-60 + Adam train.py:89 + the next effective parameters and columns) against the host implementation of the
same half (RhoCMPS.chain_rule, AdamOptimizer, RhoCMPS.R / freqs / columns), first on synthetic gradient buffers (the kernel alone),
then as Trainer(device_step=True) against Trainer() on the same HIP scans, and through train.main."""
import gc
import os

import numpy as np
import pytest

from _util import make_audio

pytestmark = pytest.mark.gpu

import _step_util as U
from _step_util import B1, B2, EPS, LR, given_kw as _kw, grad_buffer as _grad_buffer     # (shared with tests/test_gpu_psi_step.py)


def _model(D, rank, given, data=None, B=6, seed=0):
    from audio_mps_amd.scan import HipScan
    m = U.rho_model(D, rank, given, seed=seed, backend=HipScan(D), data=data, B=B)
    return m, m.hparams


def _device_step(m, gs, batch, t=1):
    """One cmps_rho_apply_step on the model's variables with zero Adam slots; every output buffer starts as NaN (U.device_step).
    -> ({variable: array}, {m}, {v}, params dict, phi [rank, D] complex, losses [2]); the model itself is not touched."""
    out = U.device_step(m, gs, batch, t=t)
    return out["vars"], out["m"], out["v"], out["params"], out["phi"], out["losses"]


def _check_outputs(m_ref, params, phi):
    """params_out / phi_out against the accessors of a model holding the same variables (the bars of
    test_model_accessors_follow_the_device_resident_state)."""
    from audio_mps_amd import layout
    D = m_ref.bond_d
    assert all(np.all(np.isfinite(np.asarray(params[k]))) for k in params) and np.all(np.isfinite(phi))
    np.testing.assert_allclose(layout.join(params, "R"), m_ref.R, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(params["freqs"], m_ref.freqs, rtol=2e-5, atol=1e-4)
    np.testing.assert_allclose(phi, m_ref.columns(), rtol=2e-5, atol=2e-6)
    assert float(params["A"]) == pytest.approx(float(m_ref.A), rel=2e-5)
    e0 = np.zeros(D, np.float32)
    e0[0] = 1
    assert np.array_equal(params["psi0_re"], e0) and np.array_equal(params["psi0_im"], np.zeros(D, np.float32))


def _bits(d):
    return {k: np.asarray(a, dtype=np.float32).tobytes() for k, a in d.items()}


# ---- 1. one step on a synthetic gradient buffer: the kernel alone ------------------------------------------------------------
@pytest.mark.parametrize("D,rank,given", [(1, 1, False), (5, 3, False), (12, 12, True), (33, 40, False), (128, 128, False)])
def test_one_step_matches_host_chain_rule_and_adam(D, rank, given):
    """Every variable, m and v within rtol 1e-6 / atol 1e-6 max|host tensor| of RhoCMPS.chain_rule(with_reg=True) +
    AdamOptimizer.apply_gradients: both sides round one double result to float32 (6e-8); the bar leaves room for the cancellation in
    phibar - c phi and for summation order, a wrong formula is off by order one."""
    from audio_mps_amd.train import AdamOptimizer
    batch = 4
    m, _ = _model(D, rank, given, seed=3)
    gs = _grad_buffer(m, batch, seed=10 * D + rank)
    dv, dm, dvv, params, phi, losses = _device_step(m, gs, batch)
    total, grads = m.chain_rule(gs, batch, with_reg=True)
    opt = AdamOptimizer(LR)
    opt.apply_gradients(m.variables, grads)                      # (m now holds the host-updated variables)
    for k in m.VARIABLE_NAMES:
        for what, got, want in (("var", dv[k], m.variables[k]), ("m", dm[k], opt.m[k]), ("v", dvv[k], opt.v[k])):
            want = np.asarray(want)
            print(k, what, "max abs diff", float(np.max(np.abs(got - want))), "max abs", float(np.max(np.abs(want))))
            assert what != "var" or np.any(want != 0)
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * float(np.max(np.abs(want))), err_msg=f"{what} {k}")
    _check_outputs(m, params, phi)
    model_loss = float(np.float64(gs[2 * D * D + 3 * D + 1]) / batch)
    print("losses", losses, model_loss, float(total))
    assert float(losses[0]) == pytest.approx(model_loss, rel=1e-6)
    assert float(losses[1]) == pytest.approx(float(total), rel=1e-6)


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("D,rank,given", U.RHO_SHAPES)
def test_one_step_matches_float64_reference(D, rank, given, mode):
    """The same step against the float64 autograd reference (tests/_step_ref.py: raw -> effective -> <cotangents, effective> / B +
    regularisers, differentiated by backward(); Adam in float64), from zero slots at t = 1 and from random slots at t = 7, at the bars
    of tests/_step_util.py: the float32 gradient read back as m / 0.1f within 2.5e-7, m and v within 5e-7 of the tensor's max,
    variables within 2^-23 max |var|, both losses within 2e-7.  The ulp distances from the host step are printed, not asserted: this
    kernel's bar against the host is the 1e-6 of the test above.
    Measured on an MI355X, worst over the ten cases: gradient 9.1e-8, m 3.4e-7 (the scalar A, where 0.9 m and 0.1 g cancel), v 1.5e-7,
    variables 6.6e-8 of the tensor's max, total 4.9e-8; 0 ulp from the host step in every tensor."""
    from audio_mps_amd.scan import HipScan
    m, gs, kw = U.rho_case(D, rank, given, mode, backend=HipScan(D))
    dev, host, ref = (f(m, gs, U.BATCH, **kw) for f in (U.device_step, U.host_step, U.reference_step))
    for k in sorted(host["vars"]):
        print(f"rho D={D} rank={rank} {mode} vs host, {k}: " + ", ".join(
            f"{w} {int(np.max(U.R.ulp_distance(dev[key][k], host[key][k])))} ulp" for w, key in (("var", "vars"), ("m", "m"), ("v", "v"))))
    U.check_against_reference(f"rho D={D} rank={rank} given={given} {mode}", dev, ref, from_zero_slots=mode == "zero")
    _check_outputs(U.with_variables(m, dev["vars"]), dev["params"], dev["phi"])


# ---- 2. grad_sums = None: the first step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rank,given", [(5, 3, False), (33, 40, True)])
def test_without_gradients_only_outputs_are_written(D, rank, given):
    import torch
    from audio_mps_amd import layout
    m, _ = _model(D, rank, given, seed=4)
    be, fields = m._get_backend(), layout.var_fields(D, rank)
    rng = np.random.default_rng(5)
    host = [layout.pack(fields, m.variables)] + [rng.standard_normal(layout.size(fields)).astype(np.float32) for _ in range(2)]
    vars_, am, av = (torch.from_numpy(x.copy()).to(be.device) for x in host)
    params = torch.full((2 * D * D + 3 * D + 1,), float("nan"), dtype=torch.float32, device=be.device)
    phi = torch.full((2 * rank * D,), float("nan"), dtype=torch.float32, device=be.device)
    losses = torch.full((2,), -1.0, dtype=torch.float32, device=be.device)
    be.rho_apply_step(vars_, am, av, None, rank, 1, 0.0, B1, B2, EPS, m.h_reg, m.r_reg, float(m._c_r), float(m._c_h), True,
                      params, phi, losses)
    for got, want in zip((vars_, am, av), host):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    ph = layout.unpack(layout.phi_fields(D, rank), phi.cpu().numpy())
    _check_outputs(m, layout.unpack(layout.param_fields(D, with_A=True), params.cpu().numpy()), layout.join(ph, "phi"))
    assert losses.cpu().tolist() == [-1.0, -1.0]                  # (no gradients consumed: no losses)


# ---- 3. the skip rule -------------------------------------------------------------------------------------------------------
def test_skip_rule_covers_the_column_cotangents():
    """One Inf in the phi tail next to a finite loss sum: the step is skipped (variables and slots bit-unchanged, losses[1] = NaN,
    losses[0] the mean loss, outputs from the unchanged variables).  With a non-finite loss sum as well the step is applied: it
    propagates as in the reference.  (Numbers fed to a one-workgroup kernel: nothing here can fault.)"""
    from audio_mps_amd.train import AdamOptimizer
    D, rank, batch = 5, 3, 4
    m, _ = _model(D, rank, False, seed=6)
    before = {k: np.array(v) for k, v in m.variables.items()}
    gs = _grad_buffer(m, batch, seed=8)
    gs[-2] = np.inf                                              # the last but one entry of phibar_im
    dv, dm, dvv, params, phi, losses = _device_step(m, gs, batch)
    assert _bits(dv) == _bits(before)
    assert all(not np.any(a) for a in dm.values()) and all(not np.any(a) for a in dvv.values())
    assert np.isnan(losses[1]) and float(losses[0]) == pytest.approx(37.5, rel=1e-6)
    _check_outputs(m, params, phi)
    # an Inf anywhere else in the gradient part does the same (the Abar word sits behind the unused blocks)
    gs2 = _grad_buffer(m, batch, seed=8)
    gs2[2 * D * D + 3 * D] = -np.inf
    dv, dm, _, _, _, losses = _device_step(m, gs2, batch)
    assert _bits(dv) == _bits(before) and all(not np.any(a) for a in dm.values()) and np.isnan(losses[1])
    # loss sum non-finite too: applied
    gs[2 * D * D + 3 * D + 1] = np.inf
    dv, dm, dvv, _, _, losses = _device_step(m, gs, batch)
    with np.errstate(all="ignore"):
        _, grads = m.chain_rule(gs, batch, with_reg=True)
        opt = AdamOptimizer(LR)
        opt.apply_gradients(m.variables, grads)
    assert np.isinf(losses[0]) and not np.isfinite(losses[1])
    for k in ("A", "Rx", "Ry", "freqs"):                         # the finite part of the gradient was consumed as the host consumes it
        assert not np.array_equal(dv[k], before[k])
        np.testing.assert_allclose(dv[k], m.variables[k], rtol=1e-6, atol=1e-6 * float(np.max(np.abs(m.variables[k]))), err_msg=k)
        np.testing.assert_allclose(dm[k], opt.m[k], rtol=1e-6, atol=1e-6 * float(np.max(np.abs(opt.m[k]))), err_msg=k)
    for k in ("Wx", "Wy"):                                       # c = sum(phi . phibar) is not finite: every column entry follows
        assert not np.any(np.isfinite(m.variables[k])) and not np.any(np.isfinite(dv[k])), k


# ---- 4. trajectory -----------------------------------------------------------------------------------------------------------
TRAJECTORY_SHAPES = [(6, 2, False), (16, 5, False), (32, 12, False), (12, 12, True), (40, 4, False)]
# max over 20 steps of |loss_a - loss_b| / max(|loss_b|, 1) between two Trainer() runs (host optimiser, same seed, same data) on two
# HipScan handles, measured with host_spread() below; 0.0: the host path reproduced itself bit for bit
HOST_SPREAD = {(6, 2, False): 0.0, (16, 5, False): 0.0, (32, 12, False): 0.0, (12, 12, True): 0.0, (40, 4, False): 0.0,
               "main": 0.0}


def _trainers(D, rank, given, device_steps, B=6, T=260):
    from audio_mps_amd.train import Trainer
    data = make_audio(B, T, 1.0 / 16000, 5)
    out = []
    for dev in device_steps:
        m, hp = _model(D, rank, given, data=data, B=B, seed=0)
        out.append(Trainer(m, hp, device_step=dev))
    return out


def host_spread(D, rank, given, steps=20):
    """The reproducibility check behind HOST_SPREAD: two host-optimiser trainers against each other."""
    a, b = _trainers(D, rank, given, (False, False))
    worst = 0.0
    for _ in range(steps):
        x, y = a.step(), b.step()
        for k in ("model_loss", "total_loss"):
            worst = max(worst, abs(x[k] - y[k]) / max(abs(y[k]), 1.0))
    return worst


def _loss_bar(key):
    s = HOST_SPREAD[key]
    return dict(rtol=1e-6, atol=1e-6) if s == 0.0 else dict(rtol=4 * s, atol=4 * s)


@pytest.mark.parametrize("D,rank,given", TRAJECTORY_SHAPES)
def test_rho_device_step_matches_host_trainer(D, rank, given, tmp_path):
    """Trainer(device_step=True) against Trainer() for RhoCMPS, both on the HIP rho scans (they differ in the optimiser half only):
    the same losses to 1e-6 over 20 steps, the same variables and Adam slots afterwards -- the bars of the PsiCMPS test.
    Host-to-host spread of the losses (HOST_SPREAD, two Trainer() runs): 0.0 at every shape, i.e. the host path reproduces itself
    bit for bit and no loss bar is widened."""
    from audio_mps_amd import RhoCMPS
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    t_dev, t_host = _trainers(D, rank, given, (True, False))
    m_dev, m_host = t_dev.model, t_host.model
    hist = []
    for _ in range(20):
        a, b = t_dev.step(), t_host.step()
        hist.append([a["model_loss"], a["total_loss"], b["model_loss"], b["total_loss"]])
    hist = np.array(hist)
    print("max rel loss diff", float(np.max(np.abs(hist[:, :2] - hist[:, 2:]) / np.maximum(np.abs(hist[:, 2:]), 1.0))))
    assert np.all(np.isfinite(hist))
    np.testing.assert_allclose(hist[:, 0], hist[:, 2], **_loss_bar((D, rank, given)))
    np.testing.assert_allclose(hist[:, 1], hist[:, 3], **_loss_bar((D, rank, given)))
    assert hist[-1, 1] < hist[0, 1]
    t_dev.sync_to_host()
    for k in RhoCMPS.VARIABLE_NAMES:
        np.testing.assert_allclose(m_dev.variables[k], m_host.variables[k], rtol=2e-5, atol=2e-6, err_msg=k)
        np.testing.assert_allclose(t_dev.opt.m[k], t_host.opt.m[k], rtol=1e-3, atol=1e-9 + 1e-5 * np.max(np.abs(t_host.opt.m[k])), err_msg=k)
    # sync=False keeps everything on the device: the losses come back as a device tensor, the step count advances
    out = t_dev.step(sync=False)
    assert "losses_dev" in out and out["losses_dev"].is_cuda and "total_loss" not in out and out["global_step"] == 21
    assert t_dev._dirty
    t_host.step()
    # the accessors follow the device state
    t_dev.sync_to_host()
    assert m_dev.variables["Wx"].shape == (rank, D)
    np.testing.assert_allclose(m_dev.columns(), m_host.columns(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(m_dev.rho_0, m_host.rho_0, rtol=2e-5, atol=2e-6)
    # checkpoint of the device-resident state -> a host-path trainer takes the same next step
    path = os.path.join(tmp_path, "model.ckpt.npz")
    t_dev.save(path)
    m2 = RhoCMPS(m_dev.hparams, data_iterator=m_dev.data_iterator, seed=1, backend=HipScan(D), **_kw(D, given))
    t2 = Trainer(m2, m_dev.hparams)
    assert t2.restore(path) and t2.global_step == 21 and t2.opt.t == 21
    assert t2.step()["total_loss"] == pytest.approx(t_dev.step()["total_loss"], rel=1e-6)


def test_lazy_sync_and_dropped_state_for_rho():
    """model.variables brings the device state back once per read after a step; assigning to it drops the device state, and the next
    device step starts from the host values (what test_model_accessors_follow_the_device_resident_state checks for PsiCMPS)."""
    t_dev, t_host = _trainers(8, 3, False, (True, False), B=4, T=120)
    m_dev, m_host = t_dev.model, t_host.model
    W0 = m_dev.W.copy()
    for _ in range(3):
        t_dev.step(sync=False)
        t_host.step()
    assert t_dev._dirty
    W3 = m_dev.W                                                    # first read: one sync
    assert not t_dev._dirty and np.max(np.abs(W3 - W0)) > 1e-4
    np.testing.assert_allclose(W3, m_host.W, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(m_dev.R, m_host.R, rtol=2e-5, atol=2e-6)
    assert float(m_dev.loss) == pytest.approx(float(m_host.loss), rel=1e-5, abs=1e-6)
    t_dev.step(sync=False)
    t_host.step()
    for mm in (m_dev, m_host):
        mm.variables["Wx"] = (mm.variables["Wx"] * np.float32(0.5)).astype(np.float32)
    assert t_dev._dev is None and not t_dev._dirty
    for _ in range(2):
        t_dev.step(sync=False)
        t_host.step()
    np.testing.assert_allclose(m_dev.columns(), m_host.columns(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(m_dev.freqs, m_host.freqs, rtol=2e-5, atol=1e-4)


def _train_and_return_the_model(steps):
    """What a helper of a training script does: build model and Trainer, step without syncing, hand back the model alone."""
    (t,) = _trainers(8, 3, False, (True,), B=4, T=120)
    for _ in range(steps):
        t.step(sync=False)
    assert t._dirty
    return t.model


def test_collected_trainer_does_not_lose_rho_steps():
    """A Trainer that goes out of scope while its device state is newer than the host copies must not take the steps with it: the
    model keeps it alive until the state has come back (CMPS.variables)."""
    m_dev = _train_and_return_the_model(3)
    gc.collect()
    (t_host,) = _trainers(8, 3, False, (False,), B=4, T=120)
    W0 = t_host.model.W.copy()
    for _ in range(3):
        t_host.step()
    m_host = t_host.model
    assert np.max(np.abs(m_host.W - W0)) > 1e-4
    for k in m_host.VARIABLE_NAMES:
        np.testing.assert_allclose(m_dev.variables[k], m_host.variables[k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(m_dev.R, m_host.R, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(m_dev.columns(), m_host.columns(), rtol=2e-5, atol=2e-6)
    assert m_dev._dirty_owner is None                              # synced by the read: the Trainer is released again
    gc.collect()
    assert m_dev._owner() is None


# ---- 5. empty shard ----------------------------------------------------------------------------------------------------------
def test_empty_shard_with_the_rho_device_step():
    """A rank whose shard is empty skips the scans and adds zeros of model.flat_size() to the all-reduce: the update comes from the
    regularisers alone."""
    (t,) = _trainers(8, 3, False, (True,), B=4, T=100)
    m = t.model
    data = m.data_iterator
    t.step()
    t.sync_to_host()
    before = {k: np.array(v) for k, v in m.variables.items()}
    out = t.step(data[:0], global_batch=4)
    t.sync_to_host()
    assert out["model_loss"] == 0.0 and np.isfinite(out["total_loss"])
    assert any(not np.array_equal(before[k], m.variables[k]) for k in before)


# ---- 6. train.main ----------------------------------------------------------------------------------------------------------
def test_train_main_runs_the_rho_device_step(tmp_path):
    """`python -m audio_mps_amd.train --mps_model rho_mps` takes the device-resident step by default on the HIP backend and follows
    the --host_optimizer run of the same command (host-to-host spread of that run: HOST_SPREAD["main"])."""
    from audio_mps_amd import RhoCMPS, train
    argv = ["--mps_model", "rho_mps", "--dataset", "damped_sine", "--sample_duration", "300", "--max_steps", "3",
            "--hparams", "bond_dim=8,initial_rank=3,minibatch_size=4,learning_rate=0.01", "--seed", "2"]
    t_dev = train.main(argv + ["--logdir", os.path.join(tmp_path, "dev")])
    t_host = train.main(argv + ["--logdir", os.path.join(tmp_path, "host"), "--host_optimizer"])
    assert t_dev.device_step and not t_host.device_step and isinstance(t_dev.model, RhoCMPS) and t_dev.model.rank_rho_0 == 3
    assert len(t_dev.history) == len(t_host.history) == 3
    for k in ("model_loss", "total_loss"):
        a, b = (np.array([h[k] for h in t.history]) for t in (t_dev, t_host))
        assert np.all(np.isfinite(a))
        np.testing.assert_allclose(a, b, **({"rtol": 1e-6} if HOST_SPREAD["main"] == 0.0 else {"rtol": 4 * HOST_SPREAD["main"]}))
    assert len({round(h["model_loss"], 6) for h in t_host.history}) > 1            # the batches differ from step to step
    np.testing.assert_allclose(t_dev.model.columns(), t_host.model.columns(), rtol=2e-5, atol=2e-6)
