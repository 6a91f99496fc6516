"""Conditions on the inputs of the state read-out tests (tests/test_gpu_states.py), checked without a GPU for every case of the tables in
tests/_states_ref.py.  They are conditions, not measurements: a case that breaks one gets another T, amplitude, R scale or draw; the
caps and factors stay.

  * d32 caps: the float32 oracle is within 2e-6 (pure state, max abs on unit vectors) / 1e-5 (RhoCMPS, relative to max |rho|) of
    f64t32, so the pure-state bar of 1e-5 is a constant >= 5 d32 and no elastic RhoCMPS bar exceeds 3e-5.
  * discrimination: every clip's reference moves by >= 10 x the case's bar between two consecutive steps somewhere, and every two clips
    of a case differ by >= 10 x the bar somewhere.  A read of the wrong stash row, the wrong time-table entry or the wrong clip of a
    pair (or of a four-clip workgroup) therefore fails the GPU test.
  * the regime is the intended one: |Q|_F <= 2^-19 at the reference's initialisation (the Q-free instance of k_fwd_chain16), above it
    at sigma = 0.3.
  * the reference is self-consistent: unit norm / unit trace, purity in [1 / D, 1], finite losses (the case stays inside 1 + z > 0)."""
import itertools

import numpy as np
import pytest

import _states_ref as SR


def _moves(states):
    """(smallest over clips of the largest step-to-step change, smallest over pairs of clips of their largest difference)."""
    B = states.shape[0]
    flat = states.reshape(B, states.shape[1], -1)
    step = min(float(np.max(np.abs(flat[b, 1:] - flat[b, :-1]))) for b in range(B))
    pair = min(float(np.max(np.abs(flat[a] - flat[b]))) for a, b in itertools.combinations(range(B), 2))
    return step, pair


def test_tables_cover_every_layout_and_option():
    """What the issue's tables ask for is in the tables (a dropped row would otherwise go unnoticed)."""
    psi = {}
    for c in SR.PSI_CASES:
        psi.setdefault(c.layout, set()).add((c.D, c.T, c.options, (c.sigma, c.rscale)))
        assert c.B % 2 == 1 and c.B >= (5 if c.layout in ("wave16", "wave32") else 3)
        assert (c.B == 3) == (c.layout in ("wide", "pair", "block"))
    assert set(psi) == {"wave16", "wave32", "wide", "pair", "block"}
    regimes = {SR.INIT, SR.VISIBLE}
    for layout, want_D in (("wave16", {3, 16}), ("wave32", {9, 17, 24, 32}), ("wide", {33, 64, 72, 128}), ("pair", {40, 128}),
                           ("block", {1, 2, 65, 128})):
        assert {k[0] for k in psi[layout]} == want_D
        for D in want_D:
            assert {k[3] for k in psi[layout] if k[0] == D} == regimes, (layout, D)
    assert {k[1] for k in psi["wave16"]} == {66} and {k[1] for k in psi["pair"]} == {67} == {k[1] for k in psi["block"]}
    for D in (9, 17, 24, 32):
        assert {k[1] for k in psi["wave32"] if k[0] == D} == {34, 66, 131}
        modes = {dict(k[2])["rank1"] for k in psi["wave32"] if k[0] == D}
        assert modes == ({SR.RANK1_DEFAULT, SR.RANK1_BF16X3} if D in (17, 32) else {SR.RANK1_DEFAULT})
    for D in (33, 64, 72, 128):
        assert {k[1] for k in psi["wide"] if k[0] == D} == {10, 67}
        for T in (10, 67):
            assert {dict(k[2])["wide_chain"] for k in psi["wide"] if k[:2] == (D, T)} == {SR.CHAIN_VALU, SR.CHAIN_MFMA, SR.CHAIN_MFMA_FWD}
    rho = {}
    for c in SR.RHO_CASES:
        rho.setdefault(c.layout, set()).add((c.D, c.rank, c.T))
        assert c.B == 3 and (c.sigma, c.rscale) in regimes
        # the family the dispatch of cmps_rho_loss_fwd gives the case (cmps_capi.hip)
        # (a forward that saves for the virtual-clip reverse sweep, the default, runs the GEMM kernel from rank 3; WAVE32 keeps the column kernels)
        want = "block" if c.variant == SR.BLOCK else "wide" if c.D > 32 else "wave" if c.variant == SR.WAVE32 or c.rank <= 2 else "mfma"
        assert c.layout == want and c.variant in (SR.AUTO, SR.BLOCK, SR.WAVE32)
    for layout, pairs in (("wave", {(7, 3), (12, 1), (32, 8)}), ("mfma", {(20, 9), (24, 17), (32, 32), (7, 3), (32, 8)}),
                          ("wide", {(40, 7), (64, 1), (64, 16), (96, 9), (48, 48), (128, 24)}), ("block", {(7, 7), (40, 3), (72, 5), (128, 128)})):
        assert {k[:2] for k in rho[layout]} == pairs
        assert any(c.layout == layout and (c.sigma, c.rscale) == SR.INIT for c in SR.RHO_CASES)
        for D, r in pairs:
            Ts = {k[2] for k in rho[layout] if k[:2] == (D, r)}
            if layout == "wave" or (layout == "mfma" and r > 8):
                assert Ts == {66, 131}
            elif layout == "mfma":                         # what AUTO runs at 3 <= rank <= 8: in addition to the issue's table
                assert Ts == {66}
            else:
                assert Ts == {6} if (D, r) == (128, 128) else max(Ts) <= 40


@pytest.mark.parametrize("case", SR.PSI_CASES, ids=lambda c: c.id)
def test_pure_state_case_conditions(case):
    hp, var, audio = SR.case_inputs(case)
    ref, loss = SR.case_reference(case)
    ref32, loss32 = SR.case_reference(case, "f32")
    assert ref.shape == (case.B, case.T - 1, case.D) and ref.dtype == np.complex128 and ref32.dtype == np.complex64
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(loss)) and np.all(np.isfinite(loss32))
    d32 = SR.psi_d32(case)
    step, pair = _moves(ref)
    q = SR.q_frobenius(hp, var)
    print(f"{case.id}: d32 {d32:.2e} (cap {SR.PSI_D32_CAP:.0e}), step {step:.2e}, clips {pair:.2e} (need {10 * case.bar:.0e}), |Q|_F {q:.2e}")
    assert d32 <= SR.PSI_D32_CAP
    np.testing.assert_allclose(np.linalg.norm(ref, axis=-1), 1.0, rtol=0, atol=1e-13)
    if case.D == 1:
        # a normalised one-component state has nowhere to move: R = Z - diag(Z) is 0 at D = 1 (model.py:42) and psi_k = psi_0 for every
        # clip and step.  The case is in the table for the smallest workgroup of k_states; it cannot tell rows or clips apart.
        assert step == 0.0 and pair == 0.0
        return
    assert step >= 10 * case.bar and pair >= 10 * case.bar
    if (case.sigma, case.rscale) == SR.INIT:
        assert q <= SR.QFLAG_LIMIT
    else:
        assert q > SR.QFLAG_LIMIT


def test_floor_case_conditions():
    """Clip 1 is annihilated at step 0 and stays exactly zero in every precision (0 / sqrt(1e-12) = 0, and (1 + s R) 0 = 0); clips 0 and 2
    are ordinary: normalised, moving, different from each other, and the float32 oracle within the cap."""
    ref, loss = SR.floor_reference()
    ref32, loss32 = SR.floor_reference("f32")
    assert ref.shape == (3, SR.FLOOR_T - 1, 2)
    for r, l in ((ref, loss), (ref32, loss32)):
        assert np.all(np.isfinite(r)) and np.all(np.isfinite(l)) and np.all(r[1] == 0)
    live = ref[[0, 2]]
    np.testing.assert_allclose(np.linalg.norm(live, axis=-1), 1.0, rtol=0, atol=1e-13)
    assert SR.max_abs(ref32, ref) <= SR.PSI_D32_CAP
    step, pair = _moves(live)
    assert step >= 10 * SR.PSI_BAR and pair >= 10 * SR.PSI_BAR


@pytest.mark.parametrize("case", SR.RHO_CASES, ids=lambda c: c.id)
def test_rho_case_conditions(case):
    D = case.D
    ref, pur, loss = SR.case_reference(case)
    ref32, pur32, loss32 = SR.case_reference(case, "f32")
    assert ref.shape == (case.B, case.T - 1, D, D) and pur.shape == (case.B, case.T - 1) and ref.dtype == np.complex128
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(loss)) and np.all(np.isfinite(loss32))
    d_rho, d_pur = SR.rho_d32(case)
    bar_rho, bar_pur = SR.rho_bars(case)
    scale = float(np.max(np.abs(ref)))
    step, pair = _moves(ref)
    print(f"{case.id}: d32 rho {d_rho:.2e} purity {d_pur:.2e} (cap {SR.RHO_D32_CAP:.0e}), bars {bar_rho:.2e} {bar_pur:.2e}, "
          f"step {step / scale:.2e}, clips {pair / scale:.2e} of max |rho| = {scale:.2e}, purity {pur.min():.4f} ... {pur.max():.4f}")
    assert d_rho <= SR.RHO_D32_CAP and d_pur <= SR.RHO_D32_CAP
    assert bar_rho <= 3e-5 and bar_pur <= 3e-5
    assert step >= 10 * bar_rho * scale and pair >= 10 * bar_rho * scale
    np.testing.assert_allclose(np.trace(ref, axis1=2, axis2=3), 1.0, rtol=0, atol=1e-12)
    assert SR.max_abs(ref, np.conj(np.swapaxes(ref, 2, 3))) <= 1e-14
    # rank(rho_k) <= rank(rho_0): 1 / min(rank, D) <= tr rho^2 <= 1, and = 1 for a rank-1 rho_0
    assert np.all(pur <= 1 + 1e-12) and np.all(pur >= 1.0 / min(case.rank, D) - 1e-12) and np.all(pur >= 1.0 / D - 1e-12)
    if case.rank == 1:
        np.testing.assert_allclose(pur, 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", [c for c in SR.PSI_CASES if c.layout == "pair"], ids=lambda c: c.id)
def test_pair_cases_are_as_quiet_as_discrimination_allows(case):
    """The rule behind PAIR_AMP: the smallest even factor at which the reference moves by PAIR_MOTION = 1.2 x 10 x the bar; the next
    smaller one does not reach it."""
    assert case.amp == SR.PAIR_AMP[case.D, (case.sigma, case.rscale)] and case.amp % 2 == 0
    assert SR.PAIR_MOTION == pytest.approx(12 * SR.PAIR_BAR)
    assert min(_moves(SR.case_reference(case)[0])) >= SR.PAIR_MOTION
    quieter = case._replace(amp=case.amp - 2)
    assert min(_moves(SR.case_reference(quieter)[0])) < SR.PAIR_MOTION
