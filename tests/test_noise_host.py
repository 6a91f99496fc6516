"""Device-drawn noise without a GPU: the numpy restatement of the definition in include/cmps.h (tests/_noise_ref.py) against its known
answers and its statistics, and the host layer (CMPS._noise, sample(device_noise=True), SampleStream.generate, python -m
audio_mps_amd.sample --device_noise) on a stand-in backend whose `draw_noise` IS that reference and records its calls.  The kernel is tied
to the reference in tests/test_gpu_noise.py."""
import math
import os

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import OracleBackend, make_audio
import _noise_ref as NR
from test_stream_host import StreamBackend
from test_rho_stream_host import RhoStreamBackend

from audio_mps_amd import HParams, PsiCMPS, RhoCMPS
from audio_mps_amd import sample as S


# ---------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = NR.philox4x32_10([np.uint64(c) for c in counter], key)
    assert " ".join("%08x" % int(x) for x in got) == want


def test_a_cut_is_exact_across_the_32_bit_counter_word():
    whole = NR.normals(5, 3, 2 ** 34 - 3, 11)
    assert whole.shape == (11,) and np.array_equal(whole[5:], NR.normals(5, 3, 2 ** 34 + 2, 6))
    assert np.array_equal(whole[:5], NR.normals(5, 3, 2 ** 34 - 3, 5))
    # the last steps a 64-bit index reaches, and the seed's high word matters
    end = NR.normals(2 ** 64 - 1, 1, 2 ** 64 - 6, 6)
    assert np.all(np.isfinite(end)) and np.array_equal(end[2:], NR.normals(2 ** 64 - 1, 1, 2 ** 64 - 4, 4))
    assert not np.array_equal(NR.normals(1, 0, 0, 8), NR.normals(1 + 2 ** 32, 0, 0, 8))


def test_statistics_of_the_reference():
    """Four standard errors each, N = 2^20 (observed: mean -1.3e-3, var - 1 3.5e-3, E z^4 - 3 1.9e-2, max |z| 5.17; products <= 7.8e-4)."""
    N = 2 ** 20
    z = NR.normals(20261019, 0, 0, N, np.float64)
    assert z.dtype == np.float64 and z.shape == (N,)
    assert float(np.max(np.abs(z))) <= 5.7682
    se = 4.0 / math.sqrt(N)
    assert abs(float(np.mean(z))) <= se
    assert abs(float(np.var(z)) - 1.0) <= 4.0 * math.sqrt(2.0 / N)
    assert abs(float(np.mean(z ** 4)) - 3.0) <= 4.0 * math.sqrt(96.0 / N)
    for lag in (1, 2, 4):
        assert abs(float(np.mean(z[:-lag] * z[lag:]))) <= se, lag
    assert abs(float(np.mean(z * NR.normals(20261019, 1, 0, N)))) <= se                 # path 0 x path 1
    assert abs(float(np.mean(z * NR.normals(20261020, 0, 0, N)))) <= se                 # seed x seed + 1
    # the float32 evaluation stays within float32 rounding of it (its trig argument pi * v alone carries 2^-24 * 2 pi)
    z32 = NR.normals(20261019, 0, 0, N, np.float32)
    assert z32.dtype == np.float32 and float(np.max(np.abs(z32 - z))) <= 4e-6


# ---------------------------------------------------------------------------------------------------
# the host layer on a stand-in backend
# ---------------------------------------------------------------------------------------------------
class _Draws:
    """`draw_noise` from the reference, recording its calls, and the three sampler entries resolving a NoisePlan through it."""

    def draw_noise(self, seed, first_step, n, length, std, first_path=0):
        self.draws.append((seed, first_step, n, length, std, first_path))
        return NR.noise(seed, first_step, n, length, std, first_path, np.float32)       # [n, length], like HipScan's tensor

    def _host(self, noise, length, n):
        from audio_mps_amd.scan import NoisePlan
        if isinstance(noise, NoisePlan):
            return np.ascontiguousarray(self.draw_noise(noise.seed, noise.first_step, n, length, noise.std).T)
        assert length is None                                                            # an array brings its own shape
        return noise


class NoiseBackend(_Draws, StreamBackend):
    def __init__(self, D):
        super().__init__(D)
        self.draws = []

    def sample(self, noise, length=None, n=None):
        return super().sample(self._host(noise, length, n))

    def sample_primed(self, prime, noise, want_pred=False, length=None, n=None):
        return super().sample_primed(prime, self._host(noise, length, n), want_pred)

    def stream(self, state_in, state_out, k0, audio, noise, want_pred=False, n=None, length=None):
        return super().stream(state_in, state_out, k0, audio, None if noise is None else self._host(noise, length, n), want_pred, n=n)


class RhoNoiseBackend(_Draws, RhoStreamBackend):
    def __init__(self, D):
        super().__init__(D)
        self.draws = []

    def rho_sample(self, noise, save_states=False, length=None, n=None):
        return super().rho_sample(self._host(noise, length, n), save_states)

    def rho_sample_primed(self, prime, noise, want_pred=False, save_states=False, length=None, n=None):
        return super().rho_sample_primed(prime, self._host(noise, length, n), want_pred, save_states)

    def rho_stream(self, state_in, state_out, k0, audio, noise, want_pred=False, n=None, save_states=False, length=None):
        return super().rho_stream(state_in, state_out, k0, audio, None if noise is None else self._host(noise, length, n), want_pred, n=n,
                                  save_states=save_states)


def _model(D=5, n=3, backend=NoiseBackend):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    be = backend(D)
    m = PsiCMPS(hp, seed=2, backend=be)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    return m, be


def _rho_model(D=5, rank=2, n=3):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=0.1, initial_rank=rank, A=5.0)
    be = RhoNoiseBackend(D)
    m = RhoCMPS(hp, seed=2, backend=be)
    m.variables["Rx"] *= np.float32(0.3)
    m.variables["Ry"] *= np.float32(0.3)
    return m, be


def test_stream_draws_at_its_position_and_a_cut_changes_no_bit():
    n, temp = 3, 0.5
    m, be = _model(n=n)
    clip = make_audio(n, 41, m.hparams.delta_t, 4)                                       # the anchor and 40 followed steps
    std = float(m.sigma) * math.sqrt(temp * float(m.delta_t))
    st = m.open_stream(n, 100, temp=temp, seed=7, device_noise=True)
    assert st.device_noise and st.noise_seed == 7 and be.draws == []
    st.follow(clip)
    a, b = st.generate(30), st.generate(1)
    assert be.draws == [(7, 40, n, 30, std, 0), (7, 70, n, 1, std, 0)] and st.position == 71
    st.generate(2)
    assert be.draws[-1] == (7, 71, n, 2, std, 0)
    st2 = m.open_stream(n, 100, temp=temp, seed=7, device_noise=True)
    st2.follow(clip[:, :20])
    st2.follow(clip[:, 20:])
    whole = st2.generate(31)
    assert be.draws[-1] == (7, 40, n, 31, std, 0)
    assert whole.dtype == np.float32 and np.array_equal(whole, np.concatenate([a, b], axis=1))
    assert not np.array_equal(whole[0], whole[1])                                        # a path is a counter word
    other = m.open_stream(n, 100, temp=temp, seed=8, device_noise=True)
    other.follow(clip)
    assert not np.array_equal(other.generate(31), whole)
    # the primed sampler draws at the same table rows: the noise the stream used, hence its waveform
    k = len(be.draws)
    cont = m.continue_clip(clip, n, 31, temp=temp, seed=7, device_noise=True)
    assert be.draws[k:] == [(7, 40, n, 31, std, 0)] and np.array_equal(cont, whole)
    out = m.sample(n, 31, temp=temp, seed=7, prime=clip, device_noise=True)
    assert be.draws[-1] == (7, 40, n, 31, std, 0) and np.array_equal((clip[:, -1:] + out / m.A).astype(np.float32), whole)
    # unprimed: table row 0, which is where a fresh stream generates
    plain = m.sample(n, 12, temp=temp, seed=7, device_noise=True)
    assert be.draws[-1] == (7, 0, n, 12, std, 0)
    fresh = m.open_stream(n, 12, temp=temp, seed=7, device_noise=True)
    assert np.array_equal(np.concatenate([fresh.generate(5), fresh.generate(7)], axis=1), plain / m.A)
    # fill_gaps generates through the same call
    known = np.ones(60, bool)
    known[20:35] = False
    g = m.open_stream(n, 60, temp=temp, seed=7, device_noise=True)
    g.fill_gaps(make_audio(1, 60, m.hparams.delta_t, 8)[0], known)
    assert be.draws[-1] == (7, 19, n, 15, std, 0)


def test_explicit_noise_wins_and_the_defaults_never_draw():
    n, length = 3, 9
    m, be = _model(n=n)
    noise = O.sample_noise(O.HParams(**m.hparams.values()), n, length, temp=0.5, seed=1)
    clip = make_audio(n, 12, m.hparams.delta_t, 6)
    want = m.sample(n, length, noise=noise)
    assert np.array_equal(m.sample(n, length, noise=noise, device_noise=True, seed=3), want)
    assert np.array_equal(m.continue_clip(clip, n, length, noise=noise, device_noise=True), m.continue_clip(clip, n, length, noise=noise))
    st = m.open_stream(n, length, seed=3, device_noise=True)
    assert np.array_equal(st.generate(length, noise=noise), want / m.A)
    # device_noise=False everywhere: numpy's Generator, as before
    m.sample(n, length, seed=3)
    m.continue_clip(clip, n, length, seed=3)
    st = m.open_stream(n, 40, seed=3)
    assert st.noise_seed is None and not st.device_noise
    st.follow(clip)
    st.generate(length)
    st.fill_gaps(clip[0], np.array([True] * 6 + [False] * 6))
    assert be.draws == []
    with pytest.raises(ValueError):
        m.sample(n, length, noise=noise[:-1], device_noise=True)                         # the shape check is the host path's


def test_seeds():
    m, be = _model()
    a, b = m.open_stream(3, 8, device_noise=True), m.open_stream(3, 8, device_noise=True)
    for st in (a, b):
        assert isinstance(st.noise_seed, int) and 0 <= st.noise_seed < 2 ** 63
    assert a.noise_seed != b.noise_seed
    a.generate(3)
    a.generate(2)
    assert [d[:2] for d in be.draws] == [(a.noise_seed, 0), (a.noise_seed, 3)]          # drawn once, kept
    m.sample(3, 4, device_noise=True)
    assert 0 <= be.draws[-1][0] < 2 ** 63
    big = m.open_stream(3, 8, seed=2 ** 64 - 1, device_noise=True)
    assert big.noise_seed == 2 ** 64 - 1
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            m.open_stream(3, 8, seed=bad, device_noise=True)


def test_a_backend_without_draw_noise_is_a_value_error():
    m, be = _model(backend=StreamBackend)
    clip = make_audio(3, 12, m.hparams.delta_t, 6)
    k = len(be.prepared)
    with pytest.raises(ValueError, match="draw_noise"):
        m.open_stream(3, 8, seed=1, device_noise=True)
    with pytest.raises(ValueError, match="draw_noise"):
        m.sample(3, 8, seed=1, device_noise=True)
    with pytest.raises(ValueError, match="draw_noise"):
        m.continue_clip(clip, 3, 8, seed=1, device_noise=True)
    assert len(be.prepared) == k                                                         # before anything ran
    assert m.sample(3, 8, seed=1).shape == (3, 8)


def test_rho_model_draws_the_same_way():
    n, temp = 2, 0.5
    m, be = _rho_model(n=n)
    clip = make_audio(n, 21, m.hparams.delta_t, 4)
    std = float(m.sigma) * math.sqrt(temp * float(m.delta_t))
    st = m.open_stream(n, 40, temp=temp, seed=9, device_noise=True)
    st.follow(clip)
    got = np.concatenate([st.generate(7), st.generate(6)], axis=1)
    assert be.draws == [(9, 20, n, 7, std, 0), (9, 27, n, 6, std, 0)]
    assert np.array_equal(m.continue_clip(clip, n, 13, temp=temp, seed=9, device_noise=True), got)
    assert be.draws[-1] == (9, 20, n, 13, std, 0)
    m.sample(n, 5, temp=temp, seed=9, device_noise=True)
    assert be.draws[-1] == (9, 0, n, 5, std, 0)
    rho = m.rho_evolve_with_sampling(n, 5, temp=temp, seed=9, device_noise=True)
    pur = m.purity(n, 5, temp=temp, seed=9, prime=clip, device_noise=True)
    assert be.draws[-2:] == [(9, 0, n, 5, std, 0), (9, 20, n, 5, std, 0)]
    assert rho.shape == (n, 5, 5, 5) and pur.shape == (n, 25)
    k = len(be.draws)
    m.sample(n, 5, seed=9)
    m.purity(n, 5, seed=9)
    assert len(be.draws) == k


def test_sample_main_device_noise(tmp_path):
    from audio_mps_amd.train import Trainer
    D, n, dur, Tp = 4, 2, 120, 130
    hp = HParams(minibatch_size=4, bond_dim=D)
    m = PsiCMPS(hp, data_iterator=make_audio(4, 32, hp.delta_t, 1), seed=0, backend=OracleBackend(D))
    tr = Trainer(m, hp)
    tr.step()
    ckdir = os.path.join(tmp_path, "run")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    common = ["--sample_duration", str(dur), "--num_samples", str(n), "--seed", "7", "--temp", "0.5", "--modeldir", ckdir]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, 0.5 * O.damped_sine(1, Tp, hp.delta_t, seed=3)[0], 16000)
    std = float(hp.sigma) * math.sqrt(0.5 * hp.delta_t)
    for extra, first in (([], 0), (["--prime", wav], Tp - 1)):
        out = os.path.join(tmp_path, "o" + str(first))
        host = S.main(common + extra + ["--out_dir", out], backend=NoiseBackend(D))
        be = NoiseBackend(D)
        one = S.main(common + extra + ["--out_dir", out, "--device_noise"], backend=be)
        assert be.draws == [(7, first, n, dur, std, 0)]
        assert one.shape == host.shape and not np.array_equal(one, host)                 # another generator
        be = NoiseBackend(D)
        seg = S.main(common + extra + ["--out_dir", out, "--device_noise", "--segment", "50"], backend=be)
        assert [d[1] for d in be.draws] == [first, first + 50, first + 100] and [d[3] for d in be.draws] == [50, 50, 20]
        assert np.array_equal(seg, one)                                                  # the cut changes no bit
    with pytest.raises(ValueError, match="device_noise"):
        S.main(common + ["--out_dir", out, "--device_noise", "--score", wav], backend=NoiseBackend(D))
    with pytest.raises(ValueError, match="draw_noise"):
        S.main(common + ["--out_dir", out, "--device_noise"], backend=StreamBackend(D))
