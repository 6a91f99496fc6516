"""CPU: the float64 autograd reference of the optimiser half (tests/_step_ref.py) against itself, then the host implementation
(PsiCMPS / RhoCMPS.chain_rule + AdamOptimizer) against it -- at the bars and on the very inputs of the GPU tests of the two step
kernels (tests/test_gpu_psi_step.py, tests/test_gpu_rho_step.py), so every GPU case is known to leave the HOST inside them."""
import numpy as np
import pytest
import torch

import _step_ref as R
import _step_util as U


# ---- 1. the reference against itself --------------------------------------------------------------------------------------
def _finite_differences(m, gs, with_reg):
    """Central differences of L (float64) in every raw variable; step 1e-4 of the tensor's max: truncation ~ 1e-8 of the gradient (L
    is quadratic in R and freqs, linear in A, smooth in psi / W), rounding ~ 1e-16 |L| / step."""
    rank = U.rank_of(m)
    base = {k: np.asarray(v, dtype=np.float64).copy() for k, v in m.variables.items()}

    def L(variables):
        with torch.no_grad():
            v = {k: torch.tensor(a, dtype=torch.float64) for k, a in variables.items()}
            return float(R.objective(v, gs, U.BATCH, m.h_reg, m.r_reg, float(m._c_r), float(m._c_h), rank, with_reg)[0])

    out = {}
    for k, a in base.items():
        h = 1e-4 * float(np.max(np.abs(a))) if np.any(a) else 1e-10
        g = np.zeros(a.shape)
        for idx in np.ndindex(*a.shape) if a.shape else [()]:
            lo, hi = ({**base, k: a.copy()} for _ in range(2))
            lo[k][idx] -= h
            hi[k][idx] += h
            g[idx] = (L(hi) - L(lo)) / (2.0 * h)
        out[k] = g
    return out


@pytest.mark.parametrize("kind,with_reg", [("psi", True), ("psi", False), ("rho", True), ("floor", True), ("zero", True)])
def test_reference_gradient_matches_finite_differences(kind, with_reg):
    """backward() of the float64 restatement against central differences of the same L, per tensor within 1e-6 of the tensor's max;
    D = 3, PsiCMPS and RhoCMPS at rank 2, and inside the psi_0 floor (sum |p|^2 = 1e-13, and p = 0 exactly)."""
    D = 3
    m = U.rho_model(D, 2) if kind == "rho" else U.psi_model(D, psi={"floor": 1e-13, "zero": "zero"}.get(kind))
    gs = U.grad_buffer(m, U.BATCH, seed=5)
    _, grads = R.total_and_grads(m.variables, gs, U.BATCH, m.h_reg, m.r_reg, float(m._c_r), float(m._c_h), U.rank_of(m), with_reg)
    fd = _finite_differences(m, gs, with_reg)
    for k in grads:
        e = U._frac(grads[k], fd[k])
        print(kind, k, f"autograd vs central differences: {e:.2e} of the tensor's max")
        assert e <= 1e-6, (k, e)
    if kind in ("floor", "zero"):                      # inside the floor the map is p * 1e6: the gradient is psi0bar / B * 1e6, nothing else
        for k, f in (("psi_x", "psi0_re"), ("psi_y", "psi0_im")):
            np.testing.assert_allclose(grads[k], gs[U.field_slice(m, f)].astype(np.float64) / U.BATCH * 1e6, rtol=1e-12)
    assert np.all(np.diagonal(grads["Rx"]) != 0)       # the diagonal's column-sum term, with and without the regularisers


def test_reference_pieces():
    """D = 1: R == 0 after the diagonal removal, so the R gradients are exactly 0; ulp_distance counts floats and folds the zeros."""
    m = U.psi_model(1)
    _, grads = R.total_and_grads(m.variables, U.grad_buffer(m, U.BATCH, 1), U.BATCH, m.h_reg, m.r_reg, float(m._c_r), float(m._c_h), 0, True)
    assert grads["Rx"].tolist() == [[0.0]] and grads["Ry"].tolist() == [[0.0]]
    one = np.float32(1)
    assert R.ulp_distance(one, np.nextafter(one, np.float32(2))) == 1 and R.ulp_distance(one, np.nextafter(one, np.float32(0))) == 1
    assert R.ulp_distance(np.float32(0.0), np.float32(-0.0)) == 0
    tiny = np.float32(1e-45)                                           # the smallest subnormal: one float above +0, two above its negative
    assert R.ulp_distance(tiny, np.float32(0)) == 1 and R.ulp_distance(tiny, -tiny) == 2
    assert R.ulp_distance(np.float32(np.nan), np.float32(np.nan)) == 0 and R.ulp_distance(np.float32(np.nan), one) > 2 ** 31
    assert R.ulp_distance(np.array([1, 2], np.float32), np.array([1, 2], np.float32)).tolist() == [0, 0]


# ---- 2. the host implementation against the reference, on the GPU tests' inputs ---------------------------------------------
def _host_against_reference(label, m, gs, kw):
    host, ref = U.host_step(m, gs, U.BATCH, **kw), U.reference_step(m, gs, U.BATCH, **kw)
    U.check_against_reference(label, host, ref, from_zero_slots=kw["t"] == 1)
    # the host's own float32 gradient, without the detour through m
    for k in sorted(ref["grads"]):
        e = U._frac(host["grads"][k], ref["grads"][k])
        print(f"{label} host gradient vs float64 reference, {k}: {e:.2e} (bar {U.GRAD_REF_BAR:.1e})")
        assert e <= U.GRAD_REF_BAR, (k, e)
    return host, ref


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("D", sorted(set(U.PSI_SHAPES) | {12}))
def test_psi_host_step_matches_reference(D, mode):
    m, gs, kw = U.psi_case(D, mode=mode)
    host, _ = _host_against_reference(f"psi D={D} {mode}", m, gs, kw)
    if D == 1:
        assert not np.any(host["grads"]["Rx"]) and not np.any(host["grads"]["Ry"])


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("D,given,with_reg,psi", U.PSI_BRANCHES)
def test_psi_host_step_branches_match_reference(D, given, with_reg, psi, mode):
    """Mixed scaling (R_in only, freqs_in only, both), with_reg = 0, the psi_0 floor (p = 0 and sum |p|^2 = 1e-13)."""
    m, gs, kw = U.psi_case(D, given, with_reg, psi, mode)
    assert (float(m._c_r) == 1.0) == (given in ("R", True)) and (float(m._c_h) == 1.0) == (given in ("freqs", True))
    host, ref = _host_against_reference(f"psi D={D} given={given} with_reg={with_reg} psi={psi} {mode}", m, gs, kw)
    if not with_reg:
        assert host["losses"][1] == host["losses"][0]
        # no 2 r_reg R term: off the diagonal the R gradient is c_r Rbar / B alone; on it the column sum is still taken off
        zbar = gs[U.field_slice(m, "R_re")].astype(np.float64).reshape(D, D) / U.BATCH
        want = float(m._c_r) * (zbar - np.diag(zbar.sum(axis=0)))
        np.testing.assert_allclose(ref["grads"]["Rx"], want, rtol=1e-12, atol=1e-12)
        assert np.all(np.abs(np.diagonal(want)) > 0)
    if psi is not None:
        for k, f in (("psi_x", "psi0_re"), ("psi_y", "psi0_im")):
            np.testing.assert_allclose(ref["grads"][k], gs[U.field_slice(m, f)].astype(np.float64) / U.BATCH * 1e6, rtol=1e-12)


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("D,rank,given", U.RHO_SHAPES)
def test_rho_host_step_matches_reference(D, rank, given, mode):
    m, gs, kw = U.rho_case(D, rank, given, mode)
    _host_against_reference(f"rho D={D} rank={rank} given={given} {mode}", m, gs, kw)
