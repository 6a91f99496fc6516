"""Primed sampling for RhoCMPS without a GPU: the expected values the GPU tests use (tests/_rho_primed_ref.py) are validated against two
independent formulations, the GPU cases' inputs are shown to leave that reference well inside the GPU bars, and the host layer
(RhoCMPS.sample(prime=...), continue_clip, predict_increments, rho_evolve_with_sampling / purity (prime=...), and
`python -m audio_mps_amd.sample` on a rho_mps checkpoint) runs on a stand-in backend that answers from the composition.
The kernels themselves are tested in tests/test_gpu_rho_primed.py."""
import os

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import OracleBackend, make_audio, rel_inf
import _primed_ref as PR
import _rho_primed_ref as RR

from audio_mps_amd import HParams, PsiCMPS, RhoCMPS
from audio_mps_amd import sample as S


# ---------------------------------------------------------------------------------------------------
# 1-3: the reference itself
# ---------------------------------------------------------------------------------------------------
def test_rank1_composition_equals_pure_state_composition():
    """rho_0 = psi_0 psi_0^dagger (W = the row psi_0^dagger, so that W^dagger W = psi_0 psi_0^dagger): the density-matrix composition
    and tests/_primed_ref.py's pure-state one are two formulations of one scan.  Bar: float32 rounding, taken as 4 x the pair's own
    float32 - float64 distance (the triangle inequality needs 2 x the larger one, given that the float64 runs agree)."""
    D, P, length, n = 6, 40, 30, 3
    hp = PR.case_hparams(D, n)
    var = PR.case_variables(D, n)
    prime, noise = PR.case_inputs(D, P, length, n)
    Wx, Wy = var.psi_x[None, :], -var.psi_y[None, :]                  # W = conj(psi)^T un-normalised: rho_0 divides by the trace
    res = {}
    for dt in ("f32", "f64"):
        wt = np.float32 if dt == "f32" else np.float64
        res["psi", dt] = PR.primed_reference(hp, var, prime, noise, dt)
        res["rho", dt] = RR.rho_primed_reference(hp, var, Wx.astype(wt), Wy.astype(wt), prime, noise, dt)[:2]
    for i, what in enumerate(("out", "pred")):
        scale = float(np.max(np.abs(res["psi", "f64"][i])))
        d64 = float(np.max(np.abs(res["rho", "f64"][i] - res["psi", "f64"][i])))
        d_rho = float(np.max(np.abs(res["rho", "f32"][i] - res["rho", "f64"][i])))
        d_psi = float(np.max(np.abs(res["psi", "f32"][i] - res["psi", "f64"][i])))
        d32 = float(np.max(np.abs(res["rho", "f32"][i].astype(np.float64) - res["psi", "f32"][i])))
        print(f"{what}: f64 pair {d64:.2e}, f32 pair {d32:.2e}, rho f32-f64 {d_rho:.2e}, psi f32-f64 {d_psi:.2e}, scale {scale:.2e}")
        assert d64 <= 1e-11 * scale
        assert d32 <= 4.0 * max(d_rho, d_psi)
    assert res["rho", "f32"][0].shape == (n, length) and res["rho", "f32"][1].shape == (n, P)


def test_composition_continues_rho_sample():
    """Priming the composition on the first P samples of O.rho_sample's waveform, with the rest of its noise, gives the rest of that
    waveform: the time grid and the frame run through the hand-over.  In float64 the clip's differences are the run's own increments
    to rounding, so the bar is 1e-9 of the waveform (a slipped time step shows at 1e-2)."""
    D, rank, P, length, n = 5, 2, 37, 45, 2
    m = RR.case_model(D, rank)
    ohp, ov, Wx, Wy = RR.oracle_side(m)
    ov, Wx, Wy = ov.astype(np.float64), Wx.astype(np.float64), Wy.astype(np.float64)
    noise = O.sample_noise(ohp, n, P + length, temp=0.5, seed=3).astype(np.float64)
    w, rr, pp = O.rho_sample(ohp, ov, Wx, Wy, noise, "f64")
    A = float(ov.A)
    prime = np.concatenate([np.zeros((n, 1)), w[:, :P] / A], axis=1)                # X_0 = 0 (model.py:105)
    out, pred, rhos, pur = RR.rho_primed_reference(ohp, ov, Wx, Wy, prime, noise[P:], "f64")
    ref = w[:, P:] - w[:, P - 1:P]
    assert np.max(np.abs(out - ref)) <= 1e-9 * np.max(np.abs(w))
    assert rel_inf(rhos, rr) <= 1e-9 and np.max(np.abs(pur - pp)) <= 1e-9
    # pred_k + noise_k is the increment the unprimed run took at step k
    incs = np.diff(np.concatenate([np.zeros((n, 1)), w / A], axis=1), axis=1)[:, :P]
    assert np.max(np.abs(pred + noise[:P].T - incs)) <= 1e-9 * np.max(np.abs(incs))


@pytest.mark.parametrize("D,rank,P,length,n", RR.GPU_CASES)
def test_gpu_case_inputs_leave_the_reference_inside_the_bars(D, rank, P, length, n):
    """For every GPU case the float32 composition is finite and at most a quarter of the GPU test's bar from the float64 one: out against
    2e-4 max |ref|, states and purity against 2e-4 (pred's bar is built from this very distance)."""
    o32, p32, r32, u32 = RR.case_reference(D, rank, P, length, n, "f32")
    o64, p64, r64, u64 = RR.case_reference(D, rank, P, length, n, "f64")
    assert all(np.all(np.isfinite(x)) for x in (o32, p32, r32, u32))
    assert o32.shape == (n, length) and p32.shape == (n, P) and r32.shape == (n, P + length, D, D) and u32.shape == (n, P + length)
    d_out, bar_out = float(np.max(np.abs(o32 - o64))), 2e-4 * float(np.max(np.abs(o32)))
    d_pred = float(np.max(np.abs(p32 - p64)))
    print(f"D={D} rank={rank} P={P} length={length} n={n}: out {d_out:.2e} (bar {bar_out:.2e}), pred {d_pred:.2e} of {np.max(np.abs(p64)):.2e}, "
          f"rho {rel_inf(r32, r64):.2e}, purity {np.max(np.abs(u32 - u64) / np.abs(u64)):.2e}")
    assert d_out <= 0.25 * bar_out
    assert rel_inf(r32, r64) <= 0.25 * 2e-4
    assert np.all(np.abs(u32 - u64) <= 0.25 * (2e-4 * np.abs(u64) + 1e-6))
    assert np.all(u64 <= 1 + 1e-9) and np.all(u64 >= 1.0 / D - 1e-9)


# ---------------------------------------------------------------------------------------------------
# 4: plumbing on an injected backend
# ---------------------------------------------------------------------------------------------------
class RhoPrimedBackend(OracleBackend):
    """OracleBackend plus the sampler entries of HipScan that RhoCMPS calls, answered from the oracle (O.rho_sample) and from the
    composition, with cmps_rho_sample_primed's table-length check; records what it is given."""

    def __init__(self, D, dtype="f32"):
        super().__init__(D, dtype)
        self.prepared, self.primes, self.states = [], [], None

    def set_params(self, p, B, T, train=True):
        super().set_params(p, B, T, train)
        self.T = T

    def rho_set_state(self, phi, B, T, train=True):
        super().rho_set_state(phi, B, T, train)
        self.prepared.append((B, T, train))
        self.train = train

    def _model(self, n):
        hp, var, Wx, Wy, _ = self._rho_model(np.zeros((n, 2), np.float32))
        return hp, var, Wx, Wy

    def rho_sample(self, noise, save_states=False):
        assert noise.shape[0] + 1 <= self.T and (self.train or not save_states)
        w, rhos, pur = O.rho_sample(*self._model(noise.shape[1]), noise, self.dtype)
        self.states = (rhos, pur) if save_states else None
        return w.astype(np.float32)

    def rho_sample_primed(self, prime, noise, want_pred=False, save_states=False):
        prime = np.asarray(prime)
        assert prime.ndim == 2 and prime.dtype == np.float32 and prime.shape[0] in (1, noise.shape[1])
        assert prime.shape[1] + noise.shape[0] <= self.T, "cmps_rho_sample_primed: T of set_params too small"
        assert self.train or not save_states
        self.primes.append(prime.shape)
        out, pred, rhos, pur = RR.rho_primed_reference(*self._model(noise.shape[1]), prime, noise, self.dtype)
        self.states = (rhos, pur) if save_states else None
        out, pred = out.astype(np.float32), pred.astype(np.float32)
        return (out, pred) if want_pred else out

    def rho_states(self, B, steps, want_rho=True, want_purity=False):
        rhos, pur = self.states
        assert rhos.shape[:2] == (B, steps)
        out = ([rhos.astype(np.complex64)] if want_rho else []) + ([pur.astype(np.float32)] if want_purity else [])
        return out[0] if len(out) == 1 else tuple(out)


def _model(D=5, rank=2, n=3, **kw):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=0.1, initial_rank=rank, A=5.0)
    be = RhoPrimedBackend(D)
    m = RhoCMPS(hp, seed=2, backend=be, **kw)
    m.variables["Rx"] *= np.float32(0.3)
    m.variables["Ry"] *= np.float32(0.3)
    return m, be


def test_rho_sample_prime_plumbing():
    n, Tp, length = 3, 17, 11
    m, be = _model(n=n)
    D = m.bond_d
    clips = make_audio(n, Tp, m.hparams.delta_t, 4)
    noise = O.sample_noise(O.HParams(**m.hparams.values()), n, length, temp=0.5, seed=1)
    # prime=None: today's call, untouched
    w = m.sample(n, length, noise=noise)
    assert w.shape == (n, length) and be.prepared[-1] == (n, length + 1, False) and be.primes == []
    # 1-D and [1, T'] primes are one clip shared by all paths; [n, T'] one clip per path; T handed to _prepare = prime_T + length
    a = m.sample(n, length, noise=noise, prime=clips[0])
    assert be.prepared[-1] == (n, Tp + length, False) and be.primes[-1] == (1, Tp)
    b = m.sample(n, length, noise=noise, prime=clips[:1])
    assert be.primes[-1] == (1, Tp)
    c = m.sample(n, length, noise=noise, prime=np.tile(clips[:1], (n, 1)))
    assert be.primes[-1] == (n, Tp)
    assert a.shape == (n, length) and np.array_equal(a, b) and np.array_equal(a, c)
    d, pred = m.sample(n, length, noise=noise, prime=clips.astype(np.float64), return_pred=True)      # any float array
    assert be.primes[-1] == (n, Tp) and d.shape == (n, length) and pred.shape == (n, Tp - 1)
    assert np.array_equal(d[0], a[0]) and not np.array_equal(d[1], a[1])
    ref = RR.rho_primed_reference(*be._model(n), clips, noise)
    assert np.array_equal(d, ref[0]) and np.array_equal(pred, ref[1])
    # states and purity across the hand-over: all P + length steps, forced ones first, from a train=True workspace of prime_T + length
    rhos = m.rho_evolve_with_sampling(n, length, noise=noise, prime=clips)
    assert be.prepared[-1] == (n, Tp + length, True)
    assert rhos.shape == (n, Tp - 1 + length, D, D) and np.array_equal(rhos, ref[2].astype(np.complex64))
    pur = m.purity(n, length, noise=noise, prime=clips)
    assert pur.shape == (n, Tp - 1 + length) and np.array_equal(pur, ref[3].astype(np.float32))
    assert m.rho_evolve_with_sampling(n, length, noise=noise).shape == (n, length, D, D)               # unprimed: as before
    assert m.purity(n, length, noise=noise).shape == (n, length)
    for bad in (clips[:2], clips[None], clips[:, :1], np.float32(1.0)):
        with pytest.raises(ValueError):
            m.sample(n, length, noise=noise, prime=bad)
    with pytest.raises(ValueError):
        m.sample(n, length, noise=noise, return_pred=True)
    with pytest.raises(ValueError):
        m.sample(n, length, noise=noise[:-1], prime=clips)                     # the noise check is the unprimed one


def test_rho_continue_clip_and_predict_increments_units():
    n, Tp, length = 2, 23, 9
    m, be = _model(n=n)
    clips = make_audio(n, Tp, m.hparams.delta_t, 6)
    out = m.sample(n, length, seed=3, prime=clips)
    cont = m.continue_clip(clips, n, length, seed=3)
    assert cont.shape == (n, length) and cont.dtype == np.float32
    np.testing.assert_array_equal(cont, (clips[:, -1:] + out / m.A).astype(np.float32))
    one = m.continue_clip(clips[1], n, length, seed=3)                         # 1-D clip: its last sample under every path
    np.testing.assert_array_equal(one[1], cont[1])
    pred = m.predict_increments(clips)
    assert pred.shape == (n, Tp - 1) and pred.dtype == np.float32 and be.prepared[-1] == (n, Tp + 1, False)
    pref = RR.rho_primed_reference(*be._model(n), clips, np.zeros((1, n), np.float32))[1]
    np.testing.assert_array_equal(pred, pref.astype(np.float32))
    # pred_k is Re tr(X rho) dt on the state BEFORE step k: entry 0 is rho_0's
    ohp, ov, Wx, Wy = be._model(n)
    R, freqs, _, _ = O.effective_params(ohp, ov)
    e0 = np.einsum('ab,ba->', R + np.conj(R.T), O.rho_0(Wx, Wy)).real.astype(np.float32) * np.float32(ohp.delta_t)
    np.testing.assert_allclose(pred[:, 0], e0, rtol=1e-5, atol=1e-9)
    m2 = RhoCMPS(m.hparams, data_iterator=lambda: clips, seed=2, backend=be)
    m2.variables.update(m.variables)
    np.testing.assert_array_equal(m2.predict_increments(), pred)
    with pytest.raises(ValueError):
        m.predict_increments()                                                 # no batch anywhere
    # the helpers are one piece of code for both models, reachable under the names callers use
    assert PsiCMPS._prime is RhoCMPS._prime and PsiCMPS.continue_clip is RhoCMPS.continue_clip
    assert PsiCMPS.predict_increments is RhoCMPS.predict_increments


# ---------------------------------------------------------------------------------------------------
# 5: python -m audio_mps_amd.sample on a rho_mps checkpoint
# ---------------------------------------------------------------------------------------------------
def test_sample_main_on_a_rho_checkpoint(tmp_path):
    from audio_mps_amd.train import Trainer
    D, rank, n, dur, Tp = 4, 3, 2, 40, 30
    hp = HParams(minibatch_size=4, bond_dim=D, initial_rank=rank)
    m = RhoCMPS(hp, data_iterator=make_audio(4, 32, hp.delta_t, 1), seed=0, backend=OracleBackend(D))
    tr = Trainer(m, hp)
    tr.step()
    ckdir = os.path.join(tmp_path, "run")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    common = ["--sample_duration", str(dur), "--num_samples", str(n), "--seed", "7", "--temp", "0.5"]
    ref = RhoCMPS(hp, seed=3, backend=RhoPrimedBackend(D))
    ref.variables.update(m.variables)                                       # the checkpoint's variables

    # without a prime: sample(...) / A; bond_dim and initial_rank come from the checkpoint (rank != D)
    be = RhoPrimedBackend(D)
    out1 = os.path.join(tmp_path, "o1")
    w1 = S.main(common + ["--modeldir", ckdir, "--out_dir", out1], backend=be)
    assert be.prepared[-1] == (n, dur + 1, False) and be.primes == [] and be.phi.shape == (rank, D)
    assert w1.shape == (n, dur) and w1.dtype == np.float32
    assert sorted(os.listdir(out1)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
    np.testing.assert_array_equal(np.load(os.path.join(out1, "samples.npy")), w1)
    np.testing.assert_array_equal(w1, (ref.sample(n, dur, temp=0.5, seed=7) / ref.A).astype(np.float32))

    # with a .wav prime: the clip, then continue_clip(...)
    clip = 0.5 * O.damped_sine(1, Tp, hp.delta_t, seed=3)[0]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, clip, 16000)
    q, _ = S.read_wav(wav)
    be = RhoPrimedBackend(D)
    out2 = os.path.join(tmp_path, "o2")
    w2 = S.main(common + ["--modeldir", ckdir, "--prime", wav, "--out_dir", out2], backend=be)
    assert be.prepared[-1] == (n, Tp + dur, False) and be.primes[-1] == (1, Tp) and be.phi.shape == (rank, D)
    assert w2.shape == (n, Tp + dur)
    for i in range(n):
        np.testing.assert_array_equal(w2[i, :Tp], q)                        # the first prime_T samples are the prime
    np.testing.assert_array_equal(w2[:, Tp:], ref.continue_clip(q, n, dur, temp=0.5, seed=7))
    assert sorted(os.listdir(out2)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
    y, rate = S.read_wav(os.path.join(out2, "sample_1.wav"))
    assert rate == 16000 and y.shape == (Tp + dur,)

    # a checkpoint with neither psi_x nor Wx is still refused; so is one whose shapes contradict --hparams
    other = os.path.join(tmp_path, "other.npz")
    np.savez(other, **{"model/A": np.float32(1), "model/Rx": np.zeros((D, D), np.float32)})
    with pytest.raises(ValueError):
        S.main(common + ["--modeldir", other], backend=RhoPrimedBackend(D))
    with pytest.raises(ValueError):
        S.main(common + ["--modeldir", ckdir, "--hparams", "initial_rank=2"], backend=RhoPrimedBackend(D))
