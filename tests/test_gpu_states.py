"""The state read-outs on the MI355X against the float64 oracle, for every stash layout they decode.

cmps_psi_states (k_states, cmps_block.hip) and cmps_rho_states (k_states_rho, cmps_rho.hip) turn what the forward scan stashed into what
the reference's psi_evolve_with_data / rho_evolve_with_data return (model.py:231-240, 76-84).  Each layout has its own lane, row,
component and clip-of-a-pair arithmetic; the reverse scans read the same rows through decoders of their own, so no loss or gradient test
sees a wrong one.  Cases, inputs and the reference (f64t32: float64 on the float32 time grid) are in tests/_states_ref.py; that the
cases can tell rows, steps and clips apart, and that the float32 oracle itself sits well inside the bars, is checked on the CPU in
tests/test_states_host.py.

Bars:
  * pure state: max |hip - f64t32| <= 1e-5 over clips, steps and components (unit vectors; the figure of the kernel-against-kernel state
    checks of test_gpu_parity.py / test_gpu_wide.py), a constant because d32 <= 2e-6; the pair kernels (bf16 mat-vec operands) 5e-3, the
    figure of test_gpu_pair.py.
  * RhoCMPS: rel_inf(hip, f64t32) <= max(1e-5, 3 d32) for rho and, built the same way from the reference purity, for tr rho^2
    (test_gpu_rho.py::_check_elastic's construction).

Not tested: the `direct` mode of launch_states_rho (columns read from the stash when they do not fit RHO_LDS_MAX = 160 KB).  The request
is ((rank D + D) float2 + 128) bytes; at the largest accepted shape, rank = D = 128, that is (128 * 128 + 128) * 8 + 128 = 132 224 bytes,
below 163 840, so no accepted call reaches the mode (the (128, 128) case below is that largest request)."""
import numpy as np
import pytest

import _states_ref as SR

pytestmark = pytest.mark.gpu


def _bits(a):
    assert a.dtype in (np.float32, np.complex64)
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------
# pure state
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.PSI_CASES, ids=lambda c: c.id)
def test_psi_states_match_f64_oracle(case):
    ref, _ = SR.case_reference(case)
    out = SR.run_psi_case(case)
    psi = out["states"]
    # the intended kernel family wrote the stash: the resolved variant, the options, and the forward kernel by name
    assert out["variant"] == SR.PSI_VARIANT[case.layout]
    for name, value in case.options:
        assert out[name] == value
    assert SR.psi_fwd_kernel(case) in out["kernels"], out["kernels"]
    assert psi.shape == (case.B, case.T - 1, case.D) and psi.dtype == np.complex64
    assert np.all(np.isfinite(psi))
    err = SR.max_abs(psi, ref)
    print(f"{case.id}: max |hip - f64t32| {err:.3e}  bar {case.bar:.0e}  d32 {SR.psi_d32(case):.2e}")
    assert err <= case.bar
    np.testing.assert_array_equal(_bits(out["again"]), _bits(psi))       # a second read of the same saved forward: the same bits


@pytest.mark.parametrize("variant", SR.FLOOR_VARIANTS)
def test_psi_states_through_the_normalisation_floor(variant):
    """tests/test_gpu_parity.py::test_normalisation_floor_branch's clip: (1 + s R) u = 0 at step 0, so |y|^2 = 0 <= 1e-12 (model.py:332)
    and psi stays exactly zero from there on; its neighbours in the workgroup are ordinary clips."""
    ref, _ = SR.floor_reference()
    out = SR.run_psi(*SR.floor_inputs(), variant=variant)
    psi = out["states"]
    assert out["variant"] == variant
    assert ("k_fwd_block" if variant == SR.BLOCK else "k_fwd_wave16") in out["kernels"], out["kernels"]
    assert psi.shape == ref.shape
    assert not np.any(np.isnan(psi.view(np.float32)))
    assert np.all(psi[1] == 0), float(np.max(np.abs(psi[1])))
    err = SR.max_abs(psi[[0, 2]], ref[[0, 2]])
    print(f"floor variant {variant}: clips 0, 2 max |hip - f64t32| {err:.3e}")
    assert err <= SR.PSI_BAR


# ---------------------------------------------------------------------------------------------------
# RhoCMPS
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.RHO_CASES, ids=lambda c: c.id)
def test_rho_states_match_f64_oracle(case):
    ref, pur_ref, _ = SR.case_reference(case)
    bar_rho, bar_pur = SR.rho_bars(case)
    out = SR.run_rho_case(case)
    rho, pur = out["rho"], out["purity"]
    assert SR.RHO_FWD_KERNEL[case.layout] in out["kernels"], out["kernels"]
    assert not (set(SR.RHO_FWD_KERNEL.values()) - {SR.RHO_FWD_KERNEL[case.layout]}) & out["kernels"], out["kernels"]
    assert rho.shape == ref.shape and rho.dtype == np.complex64 and pur.shape == pur_ref.shape
    assert np.all(np.isfinite(rho)) and np.all(np.isfinite(pur))
    e_rho, e_pur = SR.rel_inf(rho, ref), SR.rel_inf(pur, pur_ref)
    d_rho, d_pur = SR.rho_d32(case)
    print(f"{case.id}: rho rel_inf {e_rho:.3e} (bar {bar_rho:.2e}, d32 {d_rho:.2e})  purity rel_inf {e_pur:.3e} (bar {bar_pur:.2e}, d32 {d_pur:.2e})")
    assert e_rho <= bar_rho
    assert e_pur <= bar_pur
    # the same saved forward read again, with and without the matrices: the same bits
    np.testing.assert_array_equal(_bits(out["rho2"]), _bits(rho))
    np.testing.assert_array_equal(_bits(out["purity_only"]), _bits(pur))
