"""Host layer of primed sampling without a GPU: PsiCMPS.sample(prime=...), continue_clip, predict_increments and the
`python -m audio_mps_amd.sample` entry, on a stand-in backend that answers `sample` / `sample_primed` from the oracle composition
(tests/_primed_ref.py).  The kernels themselves are tested in tests/test_gpu_primed.py."""
import os
import wave

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import OracleBackend, make_audio
import _primed_ref as PR

from audio_mps_amd import HParams, PsiCMPS
from audio_mps_amd import sample as S


class PrimedBackend(OracleBackend):
    """OracleBackend plus the two sampler entries of HipScan, with cmps_psi_sample_primed's table-length check; records what it is given."""

    def __init__(self, D, dtype="f32"):
        super().__init__(D, dtype)
        self.prepared, self.primes = [], []

    def set_params(self, p, B, T, train=True):
        super().set_params(p, B, T, train)
        self.T = T
        self.prepared.append((B, T, train))

    def _oracle_model(self, n):
        """The effective parameters as oracle variables of the R_in / freqs_in kind (no scaling; R arrives with a zero diagonal)."""
        p = self.p
        R, psi0 = np.asarray(p.R), np.asarray(p.psi0)
        hp = O.HParams(minibatch_size=n, bond_dim=self.D, delta_t=p.delta_t, sigma=p.sigma, A=p.A)
        var = O.Variables(np.float32(p.A), R.real.astype(np.float32), R.imag.astype(np.float32), np.asarray(p.freqs, dtype=np.float32),
                          psi0.real.astype(np.float32), psi0.imag.astype(np.float32), scaled_R=False, scaled_freqs=False)
        return hp, var

    def sample(self, noise):
        assert noise.shape[0] + 1 <= self.T
        hp, var = self._oracle_model(noise.shape[1])
        return O.psi_sample(hp, var, noise, self.dtype).astype(np.float32)

    def sample_primed(self, prime, noise, want_pred=False):
        prime = np.asarray(prime)
        assert prime.ndim == 2 and prime.dtype == np.float32 and prime.shape[0] in (1, noise.shape[1])
        assert prime.shape[1] + noise.shape[0] <= self.T, "cmps_psi_sample_primed: T of set_params too small"
        self.primes.append(prime.shape)
        hp, var = self._oracle_model(noise.shape[1])
        out, pred = PR.primed_reference(hp, var, prime, noise, self.dtype)
        out, pred = out.astype(np.float32), pred.astype(np.float32)
        return (out, pred) if want_pred else out


def _model(D=5, n=3, **kw):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    be = PrimedBackend(D)
    m = PsiCMPS(hp, seed=2, backend=be, **kw)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    return m, be


def test_sample_prime_plumbing():
    n, Tp, length = 3, 17, 11
    m, be = _model(n=n)
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
    # the composition's hand-over: out starts from zero, one increment in
    hp, var = be._oracle_model(n)
    ref, pref = PR.primed_reference(hp, var, clips, noise)
    assert np.array_equal(d, ref) and np.array_equal(pred, pref)
    for bad in (clips[:2], clips[None], clips[:, :1], np.float32(1.0)):
        with pytest.raises(ValueError):
            m.sample(n, length, noise=noise, prime=bad)
    with pytest.raises(ValueError):
        m.sample(n, length, noise=noise, return_pred=True)
    with pytest.raises(ValueError):
        m.sample(n, length, noise=noise[:-1], prime=clips)                     # the noise check is the unprimed one


def test_continue_clip_and_predict_increments_units():
    n, Tp, length = 2, 23, 9
    m, be = _model(n=n)
    clips = make_audio(n, Tp, m.hparams.delta_t, 6)
    out = m.sample(n, length, seed=3, prime=clips)
    cont = m.continue_clip(clips, n, length, seed=3)
    assert cont.shape == (n, length) and cont.dtype == np.float32
    np.testing.assert_array_equal(cont, (clips[:, -1:] + out / m.A).astype(np.float32))
    one = m.continue_clip(clips[1], n, length, seed=3)                         # 1-D clip: its last sample under every path
    np.testing.assert_array_equal(one[1], cont[1])
    # the first continued sample sits one (expected + noise) increment behind the clip: small against the clip's own scale
    assert np.max(np.abs(cont[:, 0] - clips[:, -1])) < 0.1
    pred = m.predict_increments(clips)
    assert pred.shape == (n, Tp - 1) and pred.dtype == np.float32 and be.prepared[-1] == (n, Tp + 1, False)
    hp, var = be._oracle_model(n)
    _, pref = PR.primed_reference(hp, var, clips, np.zeros((1, n), np.float32))
    np.testing.assert_array_equal(pred, pref.astype(np.float32))
    # pred_k is 2 Re<psi|R|psi> dt on the state BEFORE step k: entry 0 is psi_0's
    R, freqs, _, _ = O.effective_params(hp, var)
    e0 = O.expectation(np.tile(O.psi_0(var)[None, :], (n, 1)), np.float32(0), R, freqs) * np.float32(hp.delta_t)
    np.testing.assert_array_equal(pred[:, 0], e0)
    m2 = PsiCMPS(m.hparams, data_iterator=lambda: clips, seed=2, backend=be)
    m2.variables.update(m.variables)
    np.testing.assert_array_equal(m2.predict_increments(), pred)
    with pytest.raises(ValueError):
        m.predict_increments()                                                 # no batch anywhere


def test_wav_round_trip_and_rejections(tmp_path):
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-1, 1, 500), [-1.0, 1.0, 1.5, -1.5, 0.0, 32767 / 32768]]).astype(np.float32)
    path = os.path.join(tmp_path, "x.wav")
    S.write_wav(path, x, 22050)
    y, rate = S.read_wav(path)
    assert rate == 22050 and y.dtype == np.float32 and y.shape == x.shape
    assert np.max(np.abs(y - np.clip(x, -1.0, 32767 / 32768))) <= 1 / 32768                  # clipped to [-1, 1), half an LSB of rounding
    assert y.min() == -1.0 and y.max() == np.float32(32767 / 32768)
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, len(x))
    for name, ch, width in (("stereo.wav", 2, 2), ("eight.wav", 1, 1)):
        p = os.path.join(tmp_path, name)
        with wave.open(p, "wb") as w:
            w.setnchannels(ch)
            w.setsampwidth(width)
            w.setframerate(16000)
            w.writeframes(bytes(64))
        with pytest.raises(ValueError) as ei:
            S.read_wav(p)
        assert f"{ch} channel" in str(ei.value) and f"{8 * width}-bit" in str(ei.value)      # says what it found
    with pytest.raises(ValueError):
        S.load_prime(path, 16000)                                                           # 22050 Hz file for a 16 kHz model
    with pytest.raises(ValueError):
        S.load_prime(os.path.join(tmp_path, "clip.txt"), 16000)


def test_sample_main_with_and_without_prime(tmp_path):
    from audio_mps_amd.train import Trainer
    D, n, dur, Tp = 4, 2, 40, 30
    hp = HParams(minibatch_size=4, bond_dim=D)
    m = PsiCMPS(hp, data_iterator=make_audio(4, 32, hp.delta_t, 1), seed=0, backend=OracleBackend(D))
    tr = Trainer(m, hp)
    tr.step()
    ckdir = os.path.join(tmp_path, "run")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    a = S.build_parser().parse_args([])
    assert (a.sample_duration, a.sample_rate, a.modeldir) == (2 ** 16, 16000, "./data")      # the reference's names and defaults
    common = ["--sample_duration", str(dur), "--num_samples", str(n), "--seed", "7", "--temp", "0.5"]

    # without a prime: sample(...) / A; --modeldir may be the directory or the file
    be = PrimedBackend(D)
    out1 = os.path.join(tmp_path, "o1")
    w1 = S.main(common + ["--modeldir", ckdir, "--out_dir", out1], backend=be)
    assert be.prepared[-1] == (n, dur + 1, False) and be.primes == []
    assert w1.shape == (n, dur) and w1.dtype == np.float32
    assert sorted(os.listdir(out1)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
    np.testing.assert_array_equal(np.load(os.path.join(out1, "samples.npy")), w1)
    ref = PsiCMPS(hp, seed=3, backend=PrimedBackend(D))
    ref.variables.update(m.variables)                                       # the checkpoint's variables
    np.testing.assert_array_equal(w1, (ref.sample(n, dur, temp=0.5, seed=7) / ref.A).astype(np.float32))
    for i in range(n):
        y, rate = S.read_wav(os.path.join(out1, f"sample_{i}.wav"))
        assert rate == 16000 and y.shape == (dur,) and np.max(np.abs(y - np.clip(w1[i], -1, 32767 / 32768))) <= 1 / 32768
    w1f = S.main(common + ["--modeldir", os.path.join(ckdir, S.CKPT_NAME), "--out_dir", out1], backend=PrimedBackend(D))
    np.testing.assert_array_equal(w1f, w1)

    # with a .wav prime: the clip, then continue_clip(...)
    clip = 0.5 * O.damped_sine(1, Tp, hp.delta_t, seed=3)[0]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, clip, 16000)
    q, _ = S.read_wav(wav)
    be = PrimedBackend(D)
    out2 = os.path.join(tmp_path, "o2")
    w2 = S.main(common + ["--modeldir", ckdir, "--prime", wav, "--out_dir", out2], backend=be)
    assert be.prepared[-1] == (n, Tp + dur, False) and be.primes[-1] == (1, Tp)
    assert w2.shape == (n, Tp + dur)
    for i in range(n):
        np.testing.assert_array_equal(w2[i, :Tp], q)                        # the first prime_T samples are the prime
    np.testing.assert_array_equal(w2[:, Tp:], ref.continue_clip(q, n, dur, temp=0.5, seed=7))
    assert sorted(os.listdir(out2)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
    with wave.open(os.path.join(out2, "sample_1.wav"), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, Tp + dur)

    # with a .npy prime of one clip per path
    clips = make_audio(n, Tp, hp.delta_t, 9)
    npy = os.path.join(tmp_path, "clips.npy")
    np.save(npy, clips)
    be = PrimedBackend(D)
    w3 = S.main(common + ["--modeldir", ckdir, "--prime", npy, "--out_dir", os.path.join(tmp_path, "o3")], backend=be)
    assert be.primes[-1] == (n, Tp)
    np.testing.assert_array_equal(w3[:, :Tp], clips)
    np.testing.assert_array_equal(w3[:, Tp:], ref.continue_clip(clips, n, dur, temp=0.5, seed=7))

    with pytest.raises(FileNotFoundError):
        S.main(common + ["--modeldir", os.path.join(tmp_path, "nowhere")], backend=PrimedBackend(D))
    with pytest.raises(ValueError):
        S.main(common + ["--modeldir", ckdir, "--hparams", "bond_dim=6"], backend=PrimedBackend(6))
