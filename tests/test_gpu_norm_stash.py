"""The normalised stash rows (STASH_WAVE32N) and the two-wave reverse scan's short pre stage on them (cmps_wave2.hip, cmps_wave_bwd2.hip).

When the reverse pass of a handle will be k_bwd_wave2w, k_fwd_wave2's loss wave writes (yhat_k, 2 ebar_k H y_k) instead of (y_k, H y_k)
and the chain wave of k_bwd_wave2w takes the partner component from LDS, the radial term from the scalar stage (q_k) and ybar_k as one
FMA.  Same algebra, rounding points moved: the bars are the existing ones, built exactly as in
tests/test_gpu_parity.py::test_two_wave_reverse_scan_matches_oracle_and_one_wave (GRAD_RTOL, widened by three times the float32
oracle's own distance from f64t32), and gradient sums go through strict_grad_sums.  Which rows a saved forward holds is read with
cmps_get_option(CMPS_OPT_SAVED_ROWS)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from _util import c_oracle_run, elastic_check, make_audio, rel_inf, strict_grad_sums
import _states_ref as SR

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-4                  # tests/test_gpu_parity.py
LOSS_RTOL = 1e-5
WAVE, WAVE32 = 2, 4
KEYS = ("Rbar", "fbar", "psi0bar", "Abar")


def _model(D, T, B, variant=WAVE, seed=0):
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D, sigma=1e-4)
    audio = make_audio(B, T, hp.delta_t, seed)
    if B >= 3:
        audio[2] = audio[2, 0]            # a constant clip between ordinary ones: x_k = 0, hence ebar_k = 0 and p_k = 0 on every step
    return PsiCMPS(hp, data_iterator=audio, seed=seed, backend=HipScan(D, variant=variant)), audio


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


def _oracle_grads(m, audio):
    D = m.bond_d
    return tuple(C.unpack_grad(c_oracle_run(m, audio, d)["grad"], D) for d in ("f32", "f64t32", "f64"))


def _check(label, g, other, gr, gt, g64):
    for k in KEYS:
        bar, bar64 = max(GRAD_RTOL, 3 * rel_inf(gr[k], gt[k])), max(GRAD_RTOL, 3 * rel_inf(gr[k], g64[k]))
        e = rel_inf(g[k], other[k])
        elastic_check(f"{k} {label}", e, bar, e, bar64)


# N = T - 1: step 0 alone; a lone top octet (step 1 above step 0); (N - 1) & 7 = 7, 0; a 32-row chunk boundary; (N - 1) & 7 = 7 at 64 steps;
# a 64-step scalar chunk boundary (q_63 takes rad_64 from the chunk above); two scalar chunks and a partial third
@pytest.mark.parametrize("N", [1, 2, 8, 9, 33, 64, 65, 130])
@pytest.mark.parametrize("B", [1, 5])          # ragged against four clips per workgroup
@pytest.mark.parametrize("D", [17, 32])        # D = 17: padded components, the partner read must see exact zeros
def test_normalised_rows_match_oracle_and_one_wave(D, B, N):
    m, audio = _model(D, N + 1, B, seed=D + N)
    g2, names2, rows2 = _grads(m, audio, 2)
    assert "k_fwd_wave2" in names2 and "k_bwd_wave2w" in names2, names2
    assert rows2 == 1                            # the forward wrote normalised rows for the two-wave scan
    g1, names1, rows1 = _grads(m, audio, 1)
    assert "k_bwd_wave" in names1 and "k_bwd_wave2w" not in names1, names1
    assert rows1 == 0                            # ... and (y, H y) rows for the one-wave scan: same handle, same settings otherwise
    gr, gt, g64 = _oracle_grads(m, audio)
    _check("vs oracle", g2, gr, gr, gt, g64)
    _check("vs one wave", g2, g1, gr, gt, g64)


def test_clip_below_the_normalisation_floor():
    """tests/test_gpu_parity.py::test_normalisation_floor_branch's construction (what tests/_states_ref.py::floor_inputs reads out): clip
    1's first step annihilates the state, n_0 = 0 <= 1e-12, so [n > 1e-12] = 0 there: q_0 = 0, the row's yhat is y 1e6 = 0, and the
    gradient stays finite.  The 32-row kernels on D = 2 (CMPS_VARIANT_WAVE32); loss and gradient at that test's own bars."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    a, A = 2.0, 4.0
    hp = HParams(minibatch_size=3, bond_dim=2, sigma=0.0, A=A)
    R = np.array([[0, a], [a, 0]], dtype=np.complex64)
    m = PsiCMPS(hp, R_in=R, freqs_in=np.array([3.0, -5.0], dtype=np.float32), psi_in=np.array([1, 1], dtype=np.complex64),
                backend=HipScan(2, variant=WAVE32))
    audio = make_audio(3, 40, hp.delta_t, 77, noise=0.05)
    audio[1, 0] = 0.0
    audio[1, 1] = -A / a
    ref = c_oracle_run(m, audio, "f32")
    per = m.loss_per_clip(audio)
    assert np.all(np.isfinite(ref["loss_per_clip"])) and np.all(np.isfinite(per))
    assert np.max(np.abs(per - ref["loss_per_clip"])) <= LOSS_RTOL * max(1.0, np.max(np.abs(ref["loss_per_clip"])))
    g, names, rows = _grads(m, audio, 2)
    assert "k_bwd_wave2w" in names and rows == 1
    gr = C.unpack_grad(ref["grad"], 2)
    for k in KEYS:
        e = rel_inf(g[k], gr[k])
        print(f"floor clip {k}: rel err {e:.3e} (bar 1e-3)")
        assert e <= 1e-3, k


@pytest.mark.parametrize("D,T", [(17, 66), (32, 66), (17, 131), (32, 131)])
def test_states_read_normalised_rows(D, T):
    """cmps_psi_states through the new row kind (k_states: y = yhat sqrt(max(n, 1e-12)), n from the scalar rows), 65 and 130 steps, against
    tests/_states_ref.py's f64t32 reference at its bar."""
    case = next(c for c in SR.PSI_CASES if c.layout == "wave32" and (c.D, c.T) == (D, T) and dict(c.options)["rank1"] == SR.RANK1_DEFAULT
                and (c.sigma, c.rscale) == SR.VISIBLE)
    ref, _ = SR.case_reference(case)
    m = SR.psi_model(*SR.case_inputs(case), case.variant, case.options)
    be = m._get_backend()
    psi = m.psi_evolve_with_data()
    assert _saved_rows(be) == 1
    assert psi.shape == ref.shape and np.all(np.isfinite(psi))
    err = SR.max_abs(psi, ref)
    print(f"{case.id}: max |hip - f64t32| {err:.3e}  bar {case.bar:.0e}")
    assert err <= case.bar


@pytest.mark.parametrize("change", ["waves 2->1", "rank1 default->bf16x3", "waves 1->2"])
def test_options_changed_between_forward_and_backward(change):
    """The reverse pass follows the saved-forward record: a forward that wrote normalised rows is followed by k_bwd_wave2w whatever the
    options say by then (never by a kernel that would read the rows as (y, H y)), a forward that wrote (y, H y) rows by a kernel that
    reads those.  The gradient is correct at the usual bars either way."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import unpack_grad
    D, T, B = 32, 131, 5
    m, audio = _model(D, T, B, seed=5)
    be = m._get_backend()
    be.set_params(m.effective_params(), B, T, train=True)
    d_audio = torch.from_numpy(audio).to(be.device)
    if change == "waves 1->2":
        _set(be, _capi.CMPS_OPT_BWD_WAVES, 1)
    be.forward(d_audio, save_for_bwd=True)
    assert _saved_rows(be) == (0 if change == "waves 1->2" else 1)
    if change == "rank1 default->bf16x3":
        be.set_rank1(_capi.CMPS_RANK1_BF16X3)
    else:
        _set(be, _capi.CMPS_OPT_BWD_WAVES, 2 if change == "waves 1->2" else 1)
    be.kernel_events(True)
    flat = be.backward().cpu().numpy()
    names = set(be.kernel_times())
    be.kernel_events(False)
    assert "k_bwd_wave2w" in names, names        # normalised rows: their one reader; (y, H y) rows with the options now at two waves: its other instance
    assert np.all(np.isfinite(flat))
    g = unpack_grad(flat, D)
    gr, gt, g64 = _oracle_grads(m, audio)
    _check(f"[{change}] vs oracle", g, gr, gr, gt, g64)


@pytest.mark.parametrize("waves", [2, 1])
def test_rho_virtual_clips_keep_their_rows(waves):
    """RhoCMPS D = 32, rank 3: the row-array GEMM forward's RHO_STASH_MFMA rows feed the pure-state reverse scan on virtual clips, which
    must go on reading them as (y, H y): against the matrix-form oracle at tests/test_gpu_rho.py's bars, both CMPS_OPT_BWD_WAVES settings."""
    from audio_mps_amd import _capi
    from oracle import cmps_oracle as O
    import test_gpu_rho as TR
    m, audio = TR._rho_model(32, 66, 3, rank=3, sigma=0.2, seed=98, rscale=0.5)
    be = m._get_backend()
    ohp, ov, Wx, Wy = TR._oracle_side(m)
    ref = O.rho_loss_and_grads(ohp, ov, Wx, Wy, audio, "f32")
    reft, ref64 = (TR._rho_ref64(ohp, ov, Wx, Wy, audio, d) for d in ("f64t32", "f64"))
    _set(be, _capi.CMPS_OPT_BWD_WAVES, waves)
    be.kernel_events(True)
    _, g = m.loss_and_grads()
    names = set(be.kernel_times())
    be.kernel_events(False)
    assert "k_fwd_rho_mfma" in names and ("k_bwd_wave2w" if waves == 2 else "k_bwd_wave") in names, names
    assert _saved_rows(be) == 0
    TR._check_elastic(g, ref, reft, ref64, ("A", "Rx", "Ry", "freqs", "Wx", "Wy"), f"virtual, {waves} wave(s) ")
