"""Primed sampling on a real MI355X: cmps_psi_sample_primed (teacher-force a clip, then sample on in the same scan) in the wave, wide
and block kernels, against the composition of the oracle's step primitives (tests/_primed_ref.py), against the unprimed sampler,
and through the host layer (PsiCMPS.sample(prime=...), continue_clip, predict_increments, python -m audio_mps_amd.sample).

Bars (stated once):
  * out: |hip - composition_f32| <= 2e-5 * max(1, max |composition_f32|): the bar of the existing sampler tests
    (tests/test_gpu_parity.py::test_sampling_matches_oracle); the float32 composition is 1e-7 .. 5e-7 from its float64 run.
  * pred: max |hip - composition_f64| <= 4 * max |composition_f32 - composition_f64| + 2e-6 * max |composition_f64|: the kernels sum in
    another order than numpy (factor 4); the floor is the accuracy tests' own.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O
from _util import oracle_hparams, oracle_variables
import _primed_ref as PR

pytestmark = pytest.mark.gpu

AUTO, BLOCK, WAVE, WIDE = 0, 1, 2, 5
OUT_RTOL = 2e-5

# (D, P, length, n, variant): P and P + length on both sides of the 64-step chunks of the wave and wide kernels; odd n in the wide kernel
CASES = [(20, 1, 3, 1, WAVE), (8, 63, 70, 3, WAVE), (32, 64, 130, 4, WAVE), (32, 65, 64, 2, WAVE), (32, 100, 130, 3, BLOCK),
         (48, 65, 100, 3, AUTO), (128, 33, 40, 2, WIDE), (48, 70, 66, 2, BLOCK)]


def _model(D, n, variant):
    """The model of test_sampling_matches_oracle: sigma = 1, A = 10, Rx, Ry *= 0.05; checked against the oracle-side copy the shared
    references are computed from."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    m = PsiCMPS(hp, seed=D, backend=HipScan(D, variant=variant))
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    ov, cv = oracle_variables(m), PR.case_variables(D, n)
    assert oracle_hparams(hp) == PR.case_hparams(D, n)
    assert all(np.array_equal(getattr(ov, k), getattr(cv, k)) for k in O.Variables.NAMES) and ov.scaled_R and ov.scaled_freqs
    return m


def _expected_family(D, variant):
    return {AUTO: WAVE if D <= 32 else WIDE, WAVE: WAVE, WIDE: WIDE, BLOCK: BLOCK}[variant]


@pytest.mark.parametrize("D,P,length,n,variant", CASES)
def test_primed_out_matches_composition(D, P, length, n, variant):
    """(a) out of the primed run against the float32 composition of the oracle's primitives."""
    m = _model(D, n, variant)
    assert m._get_backend().variant == _expected_family(D, variant)
    prime, noise = PR.case_inputs(D, P, length, n)
    ref, _ = PR.case_reference(D, P, length, n, "f32")
    out = m.sample(n, length, noise=noise, prime=prime)
    assert out.shape == (n, length) and np.all(np.isfinite(out))
    err, bar = float(np.max(np.abs(out - ref))), OUT_RTOL * max(1.0, float(np.max(np.abs(ref))))
    print(f"out D={D} P={P} length={length} n={n} variant={variant}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("D,P,length,n,variant", CASES)
def test_primed_pred_matches_f64_composition(D, P, length, n, variant):
    """(b) pred against the float64 composition, in units of the float32 composition's own distance from it.

    Measured on an MI355X (cases in the order of CASES; the largest ratio is 1.25 against the bar's factor 4):
      D   P   len n variant   |hip - f64|  |o32 - f64|  ratio  max |pred|  bar
      20  1   3   1 WAVE      1.533e-13    5.758e-12    0.03   4.885e-06   3.280e-11
      8   63  70  3 WAVE      2.262e-10    1.905e-10    1.19   4.644e-05   8.548e-10
      32  64  130 4 WAVE      4.291e-10    4.364e-10    0.98   6.210e-05   1.870e-09
      32  65  64  2 WAVE      5.900e-10    6.082e-10    0.97   6.160e-05   2.556e-09
      32  100 130 3 BLOCK     7.842e-10    7.626e-10    1.03   6.429e-05   3.179e-09
      48  65  100 3 AUTO      4.462e-10    4.394e-10    1.02   6.705e-05   1.892e-09
      128 33  40  2 WIDE      1.086e-10    8.664e-11    1.25   7.511e-05   4.968e-10
      48  70  66  2 BLOCK     4.588e-10    4.534e-10    1.01   6.716e-05   1.948e-09"""
    m = _model(D, n, variant)
    prime, noise = PR.case_inputs(D, P, length, n)
    _, p32 = PR.case_reference(D, P, length, n, "f32")
    _, p64 = PR.case_reference(D, P, length, n, "f64")
    _, pred = m.sample(n, length, noise=noise, prime=prime, return_pred=True)
    assert pred.shape == (n, P) and np.all(np.isfinite(pred))
    d_hip = float(np.max(np.abs(pred.astype(np.float64) - p64)))
    d_o32 = float(np.max(np.abs(p32.astype(np.float64) - p64)))
    scale = float(np.max(np.abs(p64)))
    bar = 4.0 * d_o32 + 2e-6 * scale
    print(f"pred D={D} P={P} length={length} n={n} variant={variant}: |hip - f64| {d_hip:.3e}  |o32 - f64| {d_o32:.3e}  "
          f"ratio {d_hip / max(d_o32, 1e-300):.2f}  max |pred| {scale:.3e}  bar {bar:.3e}")
    assert d_hip <= bar


@pytest.mark.parametrize("D,P,length,n", [(8, 100, 200, 3), (32, 70, 130, 4), (48, 65, 100, 2)])
def test_primed_continues_the_unprimed_sampler(D, P, length, n):
    """(c) priming on the first P samples of an unprimed run and sampling on with the rest of its noise gives the rest of that run."""
    m = _model(D, n, AUTO)
    A = np.float32(m.A)
    noise = O.sample_noise(oracle_hparams(m.hparams), n, P + length, temp=0.5, seed=D + 1)
    w = m.sample(n, P + length, noise=noise)
    prime = np.concatenate([np.zeros((n, 1), np.float32), (w[:, :P] / A).astype(np.float32)], axis=1)      # X_0 = 0 (model.py:244)
    out = m.sample(n, length, noise=noise[P:], prime=prime)
    ref = w[:, P:] - w[:, P - 1:P]
    err, bar = float(np.max(np.abs(out - ref))), OUT_RTOL * max(1.0, float(np.max(np.abs(ref))))
    print(f"self-consistency D={D} P={P} length={length} n={n}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("D,P,length,n,variant", [(32, 65, 70, 3, WAVE), (48, 65, 70, 3, WIDE), (48, 20, 30, 3, BLOCK)])
def test_shared_prime_equals_tiled_prime(D, P, length, n, variant):
    """(d) n_prime = 1 reads the one clip for every path: bit-identical to n copies of it (odd n in the wide kernel), and
    (e) pred_dev = NULL changes nothing in out."""
    m = _model(D, n, variant)
    prime, noise = PR.case_inputs(D, P, length, n)
    one = np.ascontiguousarray(prime[1:2])
    out_s, pred_s = m.sample(n, length, noise=noise, prime=one, return_pred=True)
    out_v, pred_v = m.sample(n, length, noise=noise, prime=one[0], return_pred=True)             # 1-D: shared too
    out_t, pred_t = m.sample(n, length, noise=noise, prime=np.tile(one, (n, 1)), return_pred=True)
    assert np.array_equal(out_s, out_t) and np.array_equal(pred_s, pred_t)
    assert np.array_equal(out_v, out_t) and np.array_equal(pred_v, pred_t)
    assert not np.array_equal(out_s[0], out_s[1])                                                # one clip, a noise row per path
    out_n = m.sample(n, length, noise=noise, prime=one)                                          # pred_dev = NULL
    assert np.array_equal(out_n, out_s)
    out_p, pred_p = m.sample(n, length, noise=noise, prime=prime, return_pred=True)              # per-path clips, with and without pred
    assert np.array_equal(m.sample(n, length, noise=noise, prime=prime), out_p)
    assert not np.array_equal(pred_p[0], pred_p[1])


@pytest.mark.parametrize("D,variant", [(8, AUTO), (48, AUTO), (48, BLOCK)])
def test_sample_kernel_names(D, variant):
    """cmps_psi_sample and cmps_psi_sample_primed are each recorded once, under the family the variant resolves to and their own mode."""
    n = 2
    m = _model(D, n, variant)
    be = m._get_backend()
    be.set_params(m.effective_params(), n, 8, train=False)
    family = {WAVE: "k_sample_wave", WIDE: "k_sample_wide", BLOCK: "k_sample_block"}[_expected_family(D, variant)]
    rng = np.random.default_rng(D)
    noise = (0.01 * rng.standard_normal((3, n))).astype(np.float32)
    prime = (0.1 * rng.standard_normal((1, 4))).astype(np.float32)
    be.kernel_events(True)
    out = be.sample(noise)
    times = be.kernel_times()
    assert list(times) == [family] and times[family][1] == 1 and np.all(np.isfinite(out))
    out_p = be.sample_primed(prime, noise)
    times = be.kernel_times()
    assert list(times) == [family + "_primed"] and times[family + "_primed"][1] == 1 and np.all(np.isfinite(out_p))


def test_primed_error_returns():
    """(f) argument and call-order checks of the C entry."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import HipScan
    D, n, prime_T, length = 8, 3, 5, 4
    m = _model(D, n, AUTO)
    be = m._get_backend()
    lib, h = be._lib, be._h
    dev = be.device
    prime = torch.zeros((n, prime_T), dtype=torch.float32, device=dev)
    noise = torch.zeros((n, length), dtype=torch.float32, device=dev)
    out = torch.empty((n, length), dtype=torch.float32, device=dev)
    pred = torch.empty((n, prime_T - 1), dtype=torch.float32, device=dev)

    def call(n_prime=n, pT=prime_T, n_=n, length_=length, prime_p=prime.data_ptr(), noise_p=noise.data_ptr(), out_p=out.data_ptr()):
        return lib.cmps_psi_sample_primed(h, prime_p, n_prime, pT, noise_p, n_, length_, out_p, pred.data_ptr(), be._stream())

    fresh = HipScan(D)
    assert fresh._lib.cmps_psi_sample_primed(fresh._h, prime.data_ptr(), n, prime_T, noise.data_ptr(), n, length, out.data_ptr(), None,
                                             fresh._stream()) == _capi.CMPS_ERR_STATE               # before cmps_set_params
    be.set_params(m.effective_params(), n, prime_T + length - 1, train=False)                        # T one short
    assert call() == _capi.CMPS_ERR_BAD_ARG
    msg = lib.cmps_last_error(h).decode()
    assert f"T >= {prime_T + length}" in msg, msg
    be.set_params(m.effective_params(), n, prime_T + length, train=False)                            # exactly sufficient
    assert call() == _capi.CMPS_OK
    torch.cuda.synchronize()
    assert call(n_prime=1) == _capi.CMPS_OK
    assert call(n_prime=2) == _capi.CMPS_ERR_BAD_ARG
    assert call(pT=1) == _capi.CMPS_ERR_BAD_ARG
    assert call(n_=0, n_prime=0) == _capi.CMPS_ERR_BAD_ARG
    assert call(length_=0) == _capi.CMPS_ERR_BAD_ARG
    assert call(prime_p=None) == _capi.CMPS_ERR_BAD_ARG
    assert call(noise_p=None) == _capi.CMPS_ERR_BAD_ARG
    assert call(out_p=None) == _capi.CMPS_ERR_BAD_ARG
    assert lib.cmps_psi_sample_primed(None, prime.data_ptr(), n, prime_T, noise.data_ptr(), n, length, out.data_ptr(), None,
                                      None) == _capi.CMPS_ERR_BAD_ARG
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    R = (0.1 * rng.standard_normal((D, D))).astype(np.float32)
    Q = (0.01 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64)
    be.legacy_set_params(R, Q, 1e-3, n, prime_T + length, train=False)
    assert call() == _capi.CMPS_ERR_STATE
    assert "legacy" in lib.cmps_last_error(h).decode()


def test_continue_clip_and_predict_increments():
    """(g) the host layer's units and shapes on one small case: continue_clip = the clip's last sample + out / A,
    predict_increments = pred of the whole batch."""
    D, P, length, n, variant = 8, 63, 70, 3, WAVE
    m = _model(D, n, variant)
    prime, noise = PR.case_inputs(D, P, length, n)
    ref, _ = PR.case_reference(D, P, length, n, "f32")
    _, p32 = PR.case_reference(D, P, length, n, "f32")
    _, p64 = PR.case_reference(D, P, length, n, "f64")
    A = float(m.A)
    cont = m.continue_clip(prime, n, length, noise=noise)
    assert cont.shape == (n, length) and cont.dtype == np.float32
    want = prime[:, -1:].astype(np.float64) + ref.astype(np.float64) / A
    assert np.max(np.abs(cont - want)) <= OUT_RTOL * max(1.0, float(np.max(np.abs(ref)))) / A + 1e-7 * max(1.0, float(np.max(np.abs(want))))
    shared = m.continue_clip(prime[0], 2, length, noise=noise[:, :2])             # a 1-D clip for two paths
    assert shared.shape == (2, length) and np.array_equal(shared[0], cont[0]) and not np.array_equal(shared[1], cont[1])
    pred = m.predict_increments(prime)
    assert pred.shape == (n, P) and pred.dtype == np.float32
    bar = 4.0 * float(np.max(np.abs(p32 - p64))) + 2e-6 * float(np.max(np.abs(p64)))
    assert float(np.max(np.abs(pred - p64))) <= bar
    m.data_iterator = prime
    assert np.array_equal(m.predict_increments(), pred)                           # the model's own batch by default
    with pytest.raises(ValueError):
        m.sample(n, length, noise=noise, prime=prime[:2])                         # two clips for three paths
    with pytest.raises(ValueError):
        m.sample(n, length, noise=noise, return_pred=True)                        # predictions without a prime


def test_sample_main_continues_a_wav_on_the_gpu(tmp_path):
    """(g) python -m audio_mps_amd.sample end to end: a checkpoint written by a 2-step Trainer, a 300-sample .wav prime, 200 steps, 2 paths."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd import sample as S
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    from _util import make_audio
    hp = HParams(minibatch_size=4, bond_dim=8)
    m = PsiCMPS(hp, data_iterator=make_audio(4, 128, hp.delta_t, 5), seed=0, backend=HipScan(8))
    tr = Trainer(m, hp)
    tr.step()
    tr.step()
    ckdir = os.path.join(tmp_path, "model")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    clip = 0.5 * O.damped_sine(1, 300, hp.delta_t, seed=2)[0]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, clip, 16000)
    out_dir = os.path.join(tmp_path, "out")
    waves = S.main(["--modeldir", ckdir, "--prime", wav, "--sample_duration", "200", "--num_samples", "2", "--seed", "4",
                    "--out_dir", out_dir])
    assert waves.shape == (2, 500) and np.all(np.isfinite(waves))
    assert sorted(os.listdir(out_dir)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
    assert np.array_equal(np.load(os.path.join(out_dir, "samples.npy")), waves)
    q, rate = S.read_wav(wav)
    assert rate == 16000 and np.max(np.abs(q - clip)) <= 1 / 32768
    assert np.array_equal(waves[0, :300], q) and np.array_equal(waves[1, :300], q)
    assert not np.array_equal(waves[0, 300:], waves[1, 300:])                      # two paths, two noise draws
    # the continuation is the model's own: the same call through the model, and its first sample one increment from the clip's last
    m2 = PsiCMPS(hp, seed=4, backend=HipScan(8))
    for k, v in m.variables.items():
        m2.variables[k] = v
    assert np.array_equal(m2.continue_clip(q, 2, 200, temp=1.0, seed=4), waves[:, 300:])
    w0, r0 = S.read_wav(os.path.join(out_dir, "sample_0.wav"))
    assert r0 == 16000 and w0.shape == (500,) and np.max(np.abs(w0 - np.clip(waves[0], -1, 32767 / 32768))) <= 1 / 32768
