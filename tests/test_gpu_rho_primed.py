"""Primed sampling for RhoCMPS on a real MI355X: cmps_rho_sample_primed (teacher-force a clip, then sample on in the same scan) in the
row-array GEMM kernel (k_sample_rho_mfma, both arithmetics) and the block kernel (k_sample_rho, both column homes), against the
composition of the oracle's step functions (tests/_rho_primed_ref.py), against the unprimed sampler, against PsiCMPS at rank 1, and
through the host layer (RhoCMPS.sample(prime=...), rho_evolve_with_sampling / purity (prime=...), python -m audio_mps_amd.sample).

Bars (stated once):
  * out: |hip - composition_f32| <= 2e-4 * max |composition_f32|: the bar of tests/test_gpu_rho.py::test_rho_sampling_matches_oracle.
  * pred: max |hip - composition_f64| <= 4 * max |composition_f32 - composition_f64| + 8 * 2^-22 * |R|_F * delta_t.  The kernels sum in
    another order than numpy (factor 4, as in tests/test_gpu_primed.py); the floor is the split arithmetics' stated product error,
    <= 2^-22 |a| |b|, applied to e = 2 sum U . (U W_R) at unit trace (2 * 2^-22 |R|_F), with the same factor 4.
  * states: rel_inf(rho) <= 2e-4, purity rtol 2e-4 / atol 1e-6, purity in [1/D - 1e-4, 1 + 1e-4] (test_rho_sampling_matches_oracle).
  * pairwise (two kernels / arithmetics on one input): 1e-4 * scale (test_rho_gemm_sampler_matches_block_sampler).
"""
import os

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O
from _util import rel_inf
import _rho_primed_ref as RR

pytestmark = pytest.mark.gpu

AUTO, BLOCK = 0, 1
BF16X3 = 2
OUT_RTOL = 2e-4
# (D, rank, P, length, n) of RR.GPU_CASES with the handle's (variant, rank1 option) and the kernel that must run
KERNELS = [(AUTO, None, "k_sample_rho_mfma_primed"), (AUTO, None, "k_sample_rho_mfma_primed"), (AUTO, None, "k_sample_rho_mfma_primed"),
           (AUTO, BF16X3, "k_sample_rho_mfma_primed"), (BLOCK, None, "k_sample_rho_primed"), (AUTO, None, "k_sample_rho_primed"),
           (AUTO, None, "k_sample_rho_primed")]
CASES = [c + k for c, k in zip(RR.GPU_CASES, KERNELS)]


def _model(D, rank, variant=AUTO, rank1=None):
    """The case's model on a HipScan of its own; checked against the copy the shared references are computed from."""
    from audio_mps_amd.scan import HipScan
    m = RR.case_model(D, rank, backend=HipScan(D, variant=variant, rank1=rank1))
    ref = RR.case_model(D, rank)
    assert all(np.array_equal(m.variables[k], ref.variables[k]) for k in m.variables) and m.rank_rho_0 == rank
    return m


@pytest.mark.parametrize("D,rank,P,length,n,variant,rank1,kernel", CASES)
def test_rho_primed_out_matches_composition(D, rank, P, length, n, variant, rank1, kernel):
    """(a) out of the primed run against the float32 composition; the kernel that ran is the one the case names."""
    m = _model(D, rank, variant, rank1)
    be = m._get_backend()
    prime, noise = RR.case_inputs(D, rank, P, length, n)
    ref = RR.case_reference(D, rank, P, length, n, "f32")[0]
    be.kernel_events(True)
    out = m.sample(n, length, noise=noise, prime=prime)
    assert [k for k in be.kernel_times() if k.startswith("k_sample")] == [kernel]
    be.kernel_events(False)
    assert out.shape == (n, length) and np.all(np.isfinite(out))
    err, bar = float(np.max(np.abs(out - ref))), OUT_RTOL * float(np.max(np.abs(ref)))
    print(f"out D={D} rank={rank} P={P} length={length} n={n} {kernel}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("D,rank,P,length,n,variant,rank1,kernel", CASES)
def test_rho_primed_pred_matches_f64_composition(D, rank, P, length, n, variant, rank1, kernel):
    """(b) pred against the float64 composition, in units of the float32 composition's own distance from it plus the split
    arithmetics' product-error floor.

    Measured on an MI355X (cases in the order of CASES; the largest ratio is 1.00 against the bar's factor 4, and the floor was not
    needed: |hip - f64| <= |o32 - f64| in every case):
      D   rank P   len n kernel                    |hip - f64|  |o32 - f64|  ratio  max |pred|  bar
      7   7    1   3   1 k_sample_rho_mfma_primed  3.768e-13    8.562e-12    0.04   5.809e-06   1.731e-09
      20  9    63  70  3 k_sample_rho_mfma_primed  1.953e-09    1.953e-09    1.00   1.034e-03   1.214e-08
      32  32   64  130 5 k_sample_rho_mfma_primed  1.706e-09    2.057e-09    0.83   1.100e-03   1.550e-08
      32  4    65  64  2 k_sample_rho_mfma_primed  1.532e-09    1.541e-09    0.99   9.840e-04   1.343e-08
      32  32   100 40  3 k_sample_rho_primed       1.795e-09    2.087e-09    0.86   1.100e-03   1.561e-08
      40  3    33  40  2 k_sample_rho_primed       3.043e-10    4.881e-10    0.62   1.179e-03   1.143e-08
      96  96   5   7   2 k_sample_rho_primed       1.578e-10    3.559e-10    0.44   1.428e-03   2.288e-08"""
    m = _model(D, rank, variant, rank1)
    prime, noise = RR.case_inputs(D, rank, P, length, n)
    p32 = RR.case_reference(D, rank, P, length, n, "f32")[1]
    p64 = RR.case_reference(D, rank, P, length, n, "f64")[1]
    _, pred = m.sample(n, length, noise=noise, prime=prime, return_pred=True)
    assert pred.shape == (n, P) and np.all(np.isfinite(pred))
    d_hip = float(np.max(np.abs(pred.astype(np.float64) - p64)))
    d_o32 = float(np.max(np.abs(p32.astype(np.float64) - p64)))
    bar = 4.0 * d_o32 + 8.0 * 2.0 ** -22 * RR.R_fro(D, rank) * float(m.hparams.delta_t)
    print(f"pred D={D} rank={rank} P={P} length={length} n={n} {kernel}: |hip - f64| {d_hip:.3e}  |o32 - f64| {d_o32:.3e}  "
          f"ratio {d_hip / max(d_o32, 1e-300):.2f}  max |pred| {np.max(np.abs(p64)):.3e}  bar {bar:.3e}")
    assert d_hip <= bar


def test_rho_primed_loud_clip_all_arithmetics_agree():
    """(c) a clip so loud that max |s_k| |R|_F = 1 at D = 32, rank 32: the fp16 x 2 kernel has no data-dependent scale (s multiplies
    float32 accumulators behind the MFMAs), so it must stay finite and agree with the bf16 x 3 form and the block kernel."""
    D, rank, P, length, n = 32, 32, 70, 40, 2
    prime, noise = RR.case_inputs(D, rank, P, length, n, loud=True)
    A = float(RR.case_model(D, rank).A)
    assert np.max(np.abs(np.diff(prime.astype(np.float64), axis=1))) / A * RR.R_fro(D, rank) == pytest.approx(1.0, rel=1e-4)
    res = {}
    for name, variant, rank1 in (("f16x2", AUTO, None), ("bf16x3", AUTO, BF16X3), ("block", BLOCK, None)):
        res[name] = _model(D, rank, variant, rank1).sample(n, length, noise=noise, prime=prime, return_pred=True)
        assert all(np.all(np.isfinite(x)) for x in res[name]), name
    for i, what in enumerate(("out", "pred")):
        scale = max(float(np.max(np.abs(res["block"][i]))), 1e-6)
        for a, b in (("f16x2", "block"), ("bf16x3", "block"), ("f16x2", "bf16x3")):
            err = float(np.max(np.abs(res[a][i] - res[b][i])))
            print(f"loud clip {what}: {a} against {b}: {err:.3e}, bar {1e-4 * scale:.3e}")
            assert err <= 1e-4 * scale, (what, a, b)


@pytest.mark.parametrize("D,rank,P,length,n,variant,rank1,kernel", CASES)
def test_rho_primed_states_match_composition(D, rank, P, length, n, variant, rank1, kernel):
    """(d) rho and purity after every one of the P + length steps, forced ones first."""
    m = _model(D, rank, variant, rank1)
    prime, noise = RR.case_inputs(D, rank, P, length, n)
    _, _, rr, rp = RR.case_reference(D, rank, P, length, n, "f32")
    rhos = m.rho_evolve_with_sampling(n, length, noise=noise, prime=prime)
    pur = m.purity(n, length, noise=noise, prime=prime)
    assert rhos.shape == (n, P + length, D, D) and pur.shape == (n, P + length)
    print(f"states D={D} rank={rank} P={P} length={length} n={n} {kernel}: rho {rel_inf(rhos, rr):.3e}, purity {np.max(np.abs(pur - rp) / rp):.3e}")
    assert rel_inf(rhos, rr) <= 2e-4
    np.testing.assert_allclose(pur, rp, rtol=2e-4, atol=1e-6)
    assert np.all(pur <= 1 + 1e-4) and np.all(pur >= 1.0 / D - 1e-4)


@pytest.mark.parametrize("D,rank,P,length,n", [(8, 3, 70, 130, 3), (32, 32, 70, 130, 3)])
def test_rho_primed_continues_the_unprimed_sampler(D, rank, P, length, n):
    """(e) priming on the first P samples of an unprimed run and sampling on with the rest of its noise gives the rest of that run."""
    m = _model(D, rank)
    A = np.float32(m.A)
    noise = O.sample_noise(RR.oracle_side(m)[0], n, P + length, temp=0.5, seed=D + 1)
    w = m.sample(n, P + length, noise=noise)
    prime = np.concatenate([np.zeros((n, 1), np.float32), (w[:, :P] / A).astype(np.float32)], axis=1)      # X_0 = 0 (model.py:105)
    out = m.sample(n, length, noise=noise[P:], prime=prime)
    ref = w[:, P:] - w[:, P - 1:P]
    err, bar = float(np.max(np.abs(out - ref))), OUT_RTOL * float(np.max(np.abs(ref)))
    print(f"self-consistency D={D} rank={rank} P={P} length={length} n={n}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar


def test_rank1_rho_primed_matches_psi_primed():
    """(f) rho_0 = psi_0 psi_0^dagger: RhoCMPS primed and PsiCMPS primed are the same scan, on different kernels."""
    from audio_mps_amd import HParams, PsiCMPS, RhoCMPS
    from audio_mps_amd.scan import HipScan
    D, P, length, n = 20, 65, 70, 3
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=0.1, A=5.0, initial_rank=1)
    psi = PsiCMPS(hp, seed=17, backend=HipScan(D))
    psi.variables["Rx"] *= np.float32(0.3)
    psi.variables["Ry"] *= np.float32(0.3)
    rho = RhoCMPS(hp, W_in=np.conj(psi.psi_0)[None, :], seed=17, backend=HipScan(D))
    for k in ("A", "Rx", "Ry", "freqs"):
        rho.variables[k] = psi.variables[k].copy()
    prime = O.damped_sine(n, P + 1, hp.delta_t, seed=D)
    noise = O.sample_noise(O.HParams(**hp.values()), n, length, temp=0.5, seed=D)
    oa, pa = rho.sample(n, length, noise=noise, prime=prime, return_pred=True)
    ob, pb = psi.sample(n, length, noise=noise, prime=prime, return_pred=True)
    err, bar = float(np.max(np.abs(oa - ob))), OUT_RTOL * float(np.max(np.abs(ob)))
    perr, pbar = float(np.max(np.abs(pa - pb))), OUT_RTOL * float(np.max(np.abs(pb)))
    print(f"rank-1 rho against psi: out {err:.3e} (bar {bar:.3e}), pred {perr:.3e} (bar {pbar:.3e})")
    assert err <= bar and perr <= pbar


@pytest.mark.parametrize("D,rank,P,length,n,variant", [(32, 32, 65, 70, 3, AUTO), (40, 3, 20, 30, 3, AUTO), (32, 5, 65, 70, 3, BLOCK)])
def test_rho_shared_prime_equals_tiled_prime(D, rank, P, length, n, variant):
    """(g) n_prime = 1 reads the one clip for every path: bit-identical to n copies of it; pred_dev = NULL changes nothing in out."""
    m = _model(D, rank, variant)
    prime, noise = RR.case_inputs(D, rank, P, length, n)
    one = np.ascontiguousarray(prime[1:2])
    out_s, pred_s = m.sample(n, length, noise=noise, prime=one, return_pred=True)
    out_v, pred_v = m.sample(n, length, noise=noise, prime=one[0], return_pred=True)             # 1-D: shared too
    out_t, pred_t = m.sample(n, length, noise=noise, prime=np.tile(one, (n, 1)), return_pred=True)
    assert np.array_equal(out_s, out_t) and np.array_equal(pred_s, pred_t)
    assert np.array_equal(out_v, out_t) and np.array_equal(pred_v, pred_t)
    assert not np.array_equal(out_s[0], out_s[1])                                                # one clip, a noise row per path
    assert np.array_equal(m.sample(n, length, noise=noise, prime=one), out_s)                    # pred_dev = NULL
    out_p, pred_p = m.sample(n, length, noise=noise, prime=prime, return_pred=True)              # per-path clips, with and without pred
    assert np.array_equal(m.sample(n, length, noise=noise, prime=prime), out_p)
    assert not np.array_equal(pred_p[0], pred_p[1])


def test_rho_primed_error_returns():
    """(h) argument, call-order and workspace checks of the C entry."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import HipScan
    D, rank, n, prime_T, length = 8, 3, 3, 5, 4
    m = _model(D, rank)
    be = m._get_backend()
    lib, h, dev = be._lib, be._h, be.device
    prime = torch.zeros((n, prime_T), dtype=torch.float32, device=dev)
    noise = torch.zeros((n, length), dtype=torch.float32, device=dev)
    out = torch.empty((n, length), dtype=torch.float32, device=dev)
    pred = torch.empty((n, prime_T - 1), dtype=torch.float32, device=dev)

    def call(n_prime=n, pT=prime_T, n_=n, length_=length, prime_p=prime.data_ptr(), noise_p=noise.data_ptr(), out_p=out.data_ptr(),
             save=0, b=be):
        return b._lib.cmps_rho_sample_primed(b._h, prime_p, n_prime, pT, noise_p, n_, length_, out_p, pred.data_ptr(), save, b._stream())

    fresh = HipScan(D)
    assert call(b=fresh) == _capi.CMPS_ERR_STATE                                                     # before cmps_set_params
    fresh.set_params(m.effective_params(), n, prime_T + length, train=False)
    assert call(b=fresh) == _capi.CMPS_ERR_STATE                                                     # before cmps_rho_set_state
    be.set_params(m.effective_params(), n, prime_T + length - 1, train=False)                        # T one short
    be.rho_set_state(m.columns(), n, prime_T + length - 1, train=False)
    assert call() == _capi.CMPS_ERR_BAD_ARG
    msg = lib.cmps_last_error(h).decode()
    assert f"T >= {prime_T + length}" in msg, msg
    be.set_params(m.effective_params(), n, prime_T + length, train=False)                            # exactly sufficient
    be.rho_set_state(m.columns(), n, prime_T + length, train=False)
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
    assert lib.cmps_rho_sample_primed(None, prime.data_ptr(), n, prime_T, noise.data_ptr(), n, length, out.data_ptr(), None, 0,
                                      None) == _capi.CMPS_ERR_BAD_ARG
    # save_states: a forward-only rho workspace has no rows; a TRAIN one sized for a shorter scan has too few
    assert call(save=1) == _capi.CMPS_ERR_WORKSPACE
    be.rho_set_state(m.columns(), n, prime_T + length - 1, train=True)
    assert call(save=1) == _capi.CMPS_ERR_WORKSPACE
    be.rho_set_state(m.columns(), n, prime_T + length, train=True)
    assert call(save=1) == _capi.CMPS_OK
    pur = be.rho_states(n, prime_T - 1 + length, want_rho=False, want_purity=True)                   # the record holds P + length steps
    assert pur.shape == (n, prime_T - 1 + length) and np.all(np.isfinite(pur))
    with pytest.raises(_capi.CmpsError):
        be.rho_states(n, length, want_rho=False, want_purity=True)
    torch.cuda.synchronize()
    # columns in the workspace (rank * D above the LDS limit): n must not exceed B_max
    m96 = _model(96, 96)
    b96 = m96._get_backend()
    b96.set_params(m96.effective_params(), 2, prime_T + length, train=False)
    b96.rho_set_state(m96.columns(), 2, prime_T + length, train=False)
    assert call(b=b96) == _capi.CMPS_ERR_WORKSPACE                                                   # n = 3 > B_max = 2
    assert call(b=b96, n_=2, n_prime=2) == _capi.CMPS_OK
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    R = (0.1 * rng.standard_normal((D, D))).astype(np.float32)
    Q = (0.01 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64)
    be.legacy_set_params(R, Q, 1e-3, n, prime_T + length, train=False)
    assert call() == _capi.CMPS_ERR_STATE
    assert "legacy" in lib.cmps_last_error(h).decode()


def test_sample_main_continues_a_wav_from_a_rho_checkpoint(tmp_path):
    """(i) python -m audio_mps_amd.sample end to end: a checkpoint written by a 2-step device-resident Trainer(RhoCMPS), a 300-sample
    .wav prime, 200 steps, 2 paths."""
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd import sample as S
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    from _util import make_audio
    D, rank = 8, 3
    hp = HParams(minibatch_size=4, bond_dim=D, initial_rank=rank)
    m = RhoCMPS(hp, data_iterator=make_audio(4, 128, hp.delta_t, 5), seed=0, backend=HipScan(D))
    tr = Trainer(m, hp, device_step=True)
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
    assert rate == 16000 and np.array_equal(waves[0, :300], q) and np.array_equal(waves[1, :300], q)
    assert not np.array_equal(waves[0, 300:], waves[1, 300:])                      # two paths, two noise draws
    m2 = RhoCMPS(hp, seed=4, backend=HipScan(D))
    for k, v in m.variables.items():
        m2.variables[k] = v
    assert m2.variables["Wx"].shape == (rank, D)
    assert np.array_equal(m2.continue_clip(q, 2, 200, temp=1.0, seed=4), waves[:, 300:])
    plain = S.main(["--modeldir", ckdir, "--sample_duration", "100", "--num_samples", "2", "--seed", "4",
                    "--out_dir", os.path.join(tmp_path, "plain")])
    assert np.array_equal(plain, (m2.sample(2, 100, temp=1.0, seed=4) / m2.A).astype(np.float32))
