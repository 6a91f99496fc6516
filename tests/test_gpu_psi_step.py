"""cmps_psi_apply_step (k_apply_step) alone on the GPU: one optimiser step of PsiCMPS on synthetic gradient buffers -- chain rule of
model.py:36-42, 49, 221-222 + regularisers train.py:55-60 + Adam train.py:89 + the next effective parameters -- against the host
implementation (PsiCMPS.chain_rule + AdamOptimizer, in ulp: the kernel promises the host's rounding points) and against the float64
autograd reference (tests/_step_ref.py, at bars built from the number formats).  tests/test_step_host.py runs the same inputs through
the host on the CPU.  The kernel is one workgroup of 1024 threads whose loops stride by 1024 over D^2: the shapes are U.PSI_SHAPES.

The host comparison found two departures from the rounding points the kernel's header promises, both fixed in cmps_opt.hip, no bar
moved: (1) HIP's __fmul_rn / __fadd_rn are the plain operators and hipcc contracted Adam's m = b1 m + (1 - b1) g and v into
v_fmac_f32 -- up to 997 ulp of m where the two terms cancel, up to 32 ulp of a variable; (2) __fsqrt_rn is the native v_sqrt_f32
(1 ulp), so sqrt(v) and with it the step were a few ulp off -- up to 8192 ulp of a variable that the step nearly cancels.

Worst distances measured on an MI355X over every case below, after the fix.  Device vs host: m, v and the variables 0 ulp,
params_out psi_0 2 ulp.  Device vs float64 reference, as fractions of the tensor's max: gradient 1.0e-7 (bar 2.5e-7), m 1.6e-7 and
v 2.1e-7 (bar 5e-7), variables 8.9e-8 (bar 1.2e-7), total 4.9e-8 and mean loss 0 (bar 2e-7)."""
import numpy as np
import pytest

import _step_ref as R
import _step_util as U

pytestmark = pytest.mark.gpu

_BACKENDS = {}


def _backend(D):
    """One HipScan handle per bond dimension for the whole module."""
    from audio_mps_amd.scan import HipScan
    if D not in _BACKENDS:
        _BACKENDS[D] = HipScan(D)
    return _BACKENDS[D]


def _bits(d):
    return {k: np.asarray(a, dtype=np.float32).tobytes() for k, a in d.items()}


def _one_step(label, m, gs, kw):
    """Device, host and reference step of one case; every check of section 3a.  -> (device, host, reference) results."""
    dev, host, ref = (f(m, gs, U.BATCH, **kw) for f in (U.device_step, U.host_step, U.reference_step))
    assert all(np.all(np.isfinite(a)) for key in ("vars", "m", "v") for a in dev[key].values()) and np.all(np.isfinite(dev["losses"]))
    U.check_against_host(label, dev, host)
    U.check_against_reference(label, dev, ref, from_zero_slots=kw["t"] == 1)
    U.check_params(label, U.with_variables(m, dev["vars"]), dev["params"])
    assert dev["losses"][0] == host["losses"][0]                      # one double product rounded once on both sides
    assert int(np.max(R.ulp_distance(dev["losses"][1], host["losses"][1]))) <= 1   # (the order of two double sums)
    return dev, host, ref


# ---- 3a. one step against both references ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("D", U.PSI_SHAPES)
def test_one_step_matches_host_and_float64_reference(D, mode):
    """From zero slots at t = 1 and from random slots at t = 7: every variable, m, v, both losses and params_out.
    Against the host: m within 1 ulp, v within 2, variables within 2 (a float32 gradient one ulp apart is the only admitted
    difference), params_out R / freqs / A bit-identical to the accessors of a model holding the updated variables, psi_0 within 4 ulp.
    Against float64: the gradient (m / 0.1f after the zero-slot step) within 2.5e-7, m and v within 5e-7 of the tensor's max,
    variables within 2^-23 max |var|, both losses within 2e-7."""
    m, gs, kw = U.psi_case(D, mode=mode, backend=_backend(D))
    dev, _, _ = _one_step(f"psi D={D} {mode}", m, gs, kw)
    if D == 1 and mode == "zero":                                     # R == 0 after the diagonal removal: its gradients are exactly 0
        assert not np.any(dev["m"]["Rx"]) and not np.any(dev["m"]["Ry"]) and not np.any(dev["v"]["Rx"])
        assert _bits({k: dev["vars"][k] for k in ("Rx", "Ry")}) == _bits({k: m.variables[k] for k in ("Rx", "Ry")})
    for k in m.variables:
        assert np.any(dev["vars"][k] != m.variables[k]) or (D == 1 and mode == "zero" and k in ("Rx", "Ry")), k


# ---- 3b. branches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("D,given,with_reg,psi", U.PSI_BRANCHES)
def test_branches_match_host_and_float64_reference(D, given, with_reg, psi, mode):
    """Mixed scaling (R_in only: c_r = 1, c_h != 1; freqs_in only; both), with_reg = 0, and the psi_0 floor (psi_x = psi_y = 0 exactly:
    pc = 0, inv = 1e6; sum |p|^2 = 1e-13: inside the floor on the float32 and on the double comparison) at the bars of 3a."""
    m, gs, kw = U.psi_case(D, given, with_reg, psi, mode, backend=_backend(D))
    dev, _, ref = _one_step(f"psi D={D} given={given} with_reg={with_reg} psi={psi} {mode}", m, gs, kw)
    if not with_reg:
        assert dev["losses"][1] == dev["losses"][0]
        if mode == "zero":
            # no 2 r_reg R term (off the diagonal the gradient is c_r Rbar / B alone); the diagonal's column sum is still taken off
            zbar = gs[U.field_slice(m, "R_re")].astype(np.float64).reshape(D, D) / U.BATCH
            want = float(m._c_r) * (zbar - np.diag(zbar.sum(axis=0)))
            got = dev["m"]["Rx"] / np.float32(0.1)
            assert U._frac(got, want) <= U.GRAD_REF_BAR and U._frac(np.diagonal(got), np.diagonal(want)) <= U.GRAD_REF_BAR
    if psi is not None and mode == "zero":
        for k, f in (("psi_x", "psi0_re"), ("psi_y", "psi0_im")):     # the gradient is psi0bar / B * 1e6 and nothing else
            want = gs[U.field_slice(m, f)].astype(np.float64) / U.BATCH * 1e6
            assert U._frac(dev["m"][k] / np.float32(0.1), want) <= U.GRAD_REF_BAR, k
    if psi is not None:
        # params_out inside the floor (the step above has moved psi out of it): without gradients psi_0 = p * fl(1 / sqrt(1e-12f)),
        # which is 0 for p = 0
        out = U.device_step(m, None, 1, **kw)
        U.check_params("floor, no gradients", m, out["params"])
        if psi == "zero":
            assert not np.any(out["params"]["psi0_re"]) and not np.any(out["params"]["psi0_im"])
        else:
            assert np.any(out["params"]["psi0_re"]) and float(np.sum(np.abs(m.psi_0) ** 2)) < 0.2   # 1e-13 * 1e12: not normalised


@pytest.mark.parametrize("D,given", [(5, False), (33, True)])
def test_without_gradients_only_outputs_are_written(D, given):
    """grad_sums = None (the first step): variables and slots bit-unchanged from random contents, losses untouched, params_out as in 3a."""
    m = U.psi_model(D, given, seed=4, backend=_backend(D))
    m0, v0 = U.random_slots(m, 5)
    m0 = {k: (10 * a).astype(np.float32) for k, a in m0.items()}
    out = U.device_step(m, None, 1, t=1, m0=m0, v0=v0, losses_init=-1.0)
    assert _bits(out["vars"]) == _bits(m.variables) and _bits(out["m"]) == _bits(m0) and _bits(out["v"]) == _bits(v0)
    assert out["losses"].tolist() == [-1.0, -1.0]                     # (no gradients consumed: no losses)
    U.check_params(f"psi D={D} no gradients", m, out["params"])


_FIELDS = ("R_re", "R_im", "freqs", "psi0_re", "psi0_im", "A")


@pytest.mark.parametrize("D", [5, 33])
@pytest.mark.parametrize("field", _FIELDS)
def test_skip_rule_covers_every_block(D, field):
    """One Inf in `field` of the gradient buffer -- its first, a middle and its last element in turn, so that at D = 33 stripes of
    nonfinite() from its first pass to its ragged third are hit -- next to a finite loss sum: the step is skipped (variables and slots
    bit-unchanged, losses[1] = NaN, losses[0] the mean loss, params_out from the unchanged variables).  (Numbers fed to a one-workgroup
    kernel: nothing here can fault.)"""
    m = U.psi_model(D, seed=6, backend=_backend(D))
    m0, v0 = U.random_slots(m, 9)
    sl = U.field_slice(m, field)
    for pos in sorted({sl.start, (sl.start + sl.stop) // 2, sl.stop - 1}):
        gs = U.grad_buffer(m, U.BATCH, seed=8)
        gs[pos] = np.inf if pos % 2 else -np.inf
        out = U.device_step(m, gs, U.BATCH, t=7, m0=m0, v0=v0)
        assert _bits(out["vars"]) == _bits(m.variables) and _bits(out["m"]) == _bits(m0) and _bits(out["v"]) == _bits(v0), (field, pos)
        assert np.isnan(out["losses"][1]) and out["losses"][0] == np.float32(37.5), (field, pos, out["losses"])
        U.check_params(f"skipped step {field}[{pos - sl.start}]", m, out["params"])
    # a NaN is caught like an Inf
    gs = U.grad_buffer(m, U.BATCH, seed=8)
    gs[sl.start] = np.nan
    out = U.device_step(m, gs, U.BATCH, t=7, m0=m0, v0=v0)
    assert _bits(out["vars"]) == _bits(m.variables) and np.isnan(out["losses"][1])


def test_nonfinite_loss_sum_applies_the_step():
    """With the loss sum non-finite as well the step is applied and follows the host: the finite part of the gradient is consumed, the
    non-finite part propagates as in the reference."""
    D = 5
    m = U.psi_model(D, seed=6, backend=_backend(D))
    gs = U.grad_buffer(m, U.BATCH, seed=8)
    gs[U.field_slice(m, "psi0_im")][-2] = np.inf
    gs[U.loss_index(D)] = np.inf
    dev = U.device_step(m, gs, U.BATCH)
    with np.errstate(all="ignore"):
        host = U.host_step(m, gs, U.BATCH)
    assert np.isinf(dev["losses"][0]) and not np.isfinite(dev["losses"][1])
    U.check_against_host("non-finite loss sum", dev, host, names=("A", "Rx", "Ry", "freqs"))
    for k in ("A", "Rx", "Ry", "freqs"):
        assert np.any(dev["vars"][k] != m.variables[k]), k
    for k in ("psi_x", "psi_y"):                                      # inv_bar = sum Re(conj(psi0bar) p) is not finite: every entry follows
        assert not np.any(np.isfinite(host["vars"][k])) and not np.any(np.isfinite(dev["vars"][k])), k
