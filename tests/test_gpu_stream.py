"""The resumable sampler on a real MI355X: cmps_psi_stream in the wave, wide and block kernels.  (a) cutting a run into more segments
changes no bit of out, pred or the state record; (b) the run against the oracle composition for a plan (tests/_stream_ref.py); (c) against
cmps_psi_sample_primed and cmps_psi_sample; (d) the error returns; (e) the kernel names; (f) the host layer (open_stream, fill_gaps,
python -m audio_mps_amd.sample --segment).

Bars (those of tests/test_gpu_primed.py, stated there):
  * out:  |hip - composition_f32| <= 2e-5 * max(1, max |composition_f32|)
  * pred: max |hip - composition_f64| <= 4 * max |composition_f32 - composition_f64| + 2e-6 * max |composition_f64|
"""
import os

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O
import _primed_ref as PR
import _stream_ref as SR
from test_gpu_primed import AUTO, BLOCK, WAVE, WIDE, OUT_RTOL, _expected_family, _model

pytestmark = pytest.mark.gpu

# (D, variant, n, plan): segment ends on both sides of the 64-step chunks, single-step segments, forced-only and sampled-only segments,
# forced after sampled, padded D, an odd path count in the pair-of-paths kernel
CASES = [(20, WAVE, 1, ((1, 0), (0, 3))),
         (8, WAVE, 3, ((63, 0), (1, 0), (0, 1), (0, 63), (37, 70))),
         (32, WAVE, 4, ((64, 0), (0, 64), (65, 65))),
         (48, AUTO, 3, ((65, 0), (0, 1), (0, 99), (30, 34))),
         (128, WIDE, 2, ((33, 40), (1, 1))),
         (48, BLOCK, 2, ((70, 0), (0, 66))),
         (32, BLOCK, 3, ((100, 30), (0, 100)))]
FAMILY_NAME = {WAVE: "k_sample_wave_stream", WIDE: "k_sample_wide_stream", BLOCK: "k_sample_block_stream"}


def run_plan(m, plan, clip, noise, n, same_state=False, null_final=False, repeat_params=False):
    """The plan call by call through HipScan.stream, segment s on clip[:, f0 : f0 + forced + 1] and noise[l0 : l0 + sampled]: (out [n, L],
    pred [n, F], the final state record as bytes, or None with null_final).  The state alternates between two tensors, or (same_state)
    is read and written in place; repeat_params calls set_params again, with the same arguments, behind the first segment."""
    be = m._get_backend()
    F, L = SR.plan_steps(plan)
    be.set_params(m.effective_params(), n, F + L + 1, train=False)
    states = [be.stream_state(n), be.stream_state(n)]
    outs, preds, cur, k0, f0, l0 = [], [], None, 0, 0, 0
    for idx, (f, s) in enumerate(plan):
        if idx == len(plan) - 1 and null_final:
            nxt = None
        elif same_state:
            nxt = states[0]
        else:
            nxt = states[1] if cur is states[0] else states[0]
        out, pred = be.stream(cur, nxt, k0, clip[:, f0:f0 + f + 1] if f else None, noise[l0:l0 + s] if s else None, True, n=n)
        assert out.shape == (n, s) and pred.shape == (n, f)
        outs.append(out)
        preds.append(pred)
        cur, k0, f0, l0 = nxt, k0 + f + s, f0 + f, l0 + s
        if repeat_params and idx == 0:
            be.set_params(m.effective_params(), n, F + L + 1, train=False)
    return np.concatenate(outs, axis=1), np.concatenate(preds, axis=1), (None if cur is None else cur.cpu().numpy())


@pytest.mark.parametrize("D,variant,n,plan", CASES)
def test_refinement_is_bit_exact(D, variant, n, plan):
    """(a) the plan as written against the plan with every call cut again (middle of the forced part, the hand-over, one step into the
    sampled part): out, pred and the final record; the same with the state updated in place, a NULL final state_out, set_params repeated
    between two segments, and one shared signal against its tiled copy."""
    m = _model(D, n, variant)
    assert m._get_backend().variant == _expected_family(D, variant)
    clip, noise = SR.case_inputs(D, plan, n)
    fine = tuple(SR.refine(plan))
    assert len(fine) > len(plan)
    out, pred, rec = run_plan(m, plan, clip, noise, n)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(pred)) and rec.any()
    for kw in ({}, {"same_state": True}, {"repeat_params": True}, {"null_final": True}):
        o2, p2, r2 = run_plan(m, fine, clip, noise, n, **kw)
        assert np.array_equal(o2, out) and np.array_equal(p2, pred), kw
        assert (r2 is None) if kw.get("null_final") else np.array_equal(r2, rec), kw
    one = np.ascontiguousarray(clip[n - 1:n])
    o_s, p_s, r_s = run_plan(m, fine, one, noise, n)                                   # n_audio = 1
    o_t, p_t, r_t = run_plan(m, plan, np.tile(one, (n, 1)), noise, n)
    assert np.array_equal(o_s, o_t) and np.array_equal(p_s, p_t) and np.array_equal(r_s, r_t)
    if n > 1 and out.shape[1]:
        assert not np.array_equal(o_s[0], o_s[1])                                        # one signal, a noise row per path


@pytest.mark.parametrize("D,variant,n,plan", CASES)
def test_plan_matches_oracle_composition(D, variant, n, plan):
    """(b) out against the float32 composition, pred against the float64 one in units of the float32 composition's own distance from it.

    Measured on an MI355X (cases in the order of CASES):
      D   variant n  steps  out err    out bar    |hip - f64|  |o32 - f64|  ratio  pred bar
      20  WAVE    1  4      0.000e+00  2.000e-05  1.533e-13    5.758e-12    0.03   3.280e-11
      8   WAVE    3  235    2.384e-07  3.037e-05  1.235e-09    1.232e-09    1.00   5.022e-09
      32  WAVE    4  258    5.960e-08  2.000e-05  3.079e-09    3.045e-09    1.01   1.233e-08
      48  AUTO    3  229    2.980e-08  2.000e-05  2.196e-09    2.192e-09    1.00   8.903e-09
      128 WIDE    2  75     7.451e-09  2.000e-05  1.006e-10    9.687e-11    1.04   5.380e-10
      48  BLOCK   2  136    5.960e-08  2.062e-05  4.661e-10    4.534e-10    1.03   1.948e-09
      32  BLOCK   3  230    1.788e-07  2.065e-05  7.662e-10    7.626e-10    1.00   3.179e-09"""
    m = _model(D, n, variant)
    clip, noise = SR.case_inputs(D, plan, n)
    o32, p32 = SR.case_reference(D, plan, n, "f32")
    _, p64 = SR.case_reference(D, plan, n, "f64")
    out, pred, _ = run_plan(m, plan, clip, noise, n)
    err, bar = float(np.max(np.abs(out - o32))), OUT_RTOL * max(1.0, float(np.max(np.abs(o32))))
    d_hip = float(np.max(np.abs(pred.astype(np.float64) - p64)))
    d_o32 = float(np.max(np.abs(p32.astype(np.float64) - p64)))
    pbar = 4.0 * d_o32 + 2e-6 * float(np.max(np.abs(p64)))
    print(f"stream D={D} variant={variant} n={n} steps={sum(SR.plan_steps(plan))}: out err {err:.3e} bar {bar:.3e}  |hip - f64| {d_hip:.3e}  "
          f"|o32 - f64| {d_o32:.3e}  ratio {d_hip / max(d_o32, 1e-300):.2f}  pred bar {pbar:.3e}")
    assert err <= bar
    assert d_hip <= pbar


@pytest.mark.parametrize("D,P,length,n,variant", [(32, 65, 64, 2, WAVE), (48, 65, 100, 3, AUTO), (48, 70, 66, 2, BLOCK)])
def test_one_call_equals_the_existing_entries(D, P, length, n, variant):
    """(c) one stream call with k0 = 0 and a primed run's arguments against cmps_psi_sample_primed, and a sampled-only call against
    cmps_psi_sample: the step arithmetic is the same source, so bit-identity is expected; asserted are the bars of (b), printed is
    whether the bits agree.  Measured on an MI355X: wave (D = 32) and wide (D = 48) bit-identical to both entries; the block kernel
    (D = 48) bit-identical to cmps_psi_sample and 5.96e-08 (out) / 3.27e-11 (pred) from cmps_psi_sample_primed."""
    m = _model(D, n, variant)
    be = m._get_backend()
    prime, noise = PR.case_inputs(D, P, length, n)
    o32, p32 = PR.case_reference(D, P, length, n, "f32")
    _, p64 = PR.case_reference(D, P, length, n, "f64")
    be.set_params(m.effective_params(), n, P + length + 1, train=False)
    out_p, pred_p = be.sample_primed(prime, noise, want_pred=True)
    out_s, pred_s = be.stream(None, None, 0, prime, noise, True, n=n)
    bar = OUT_RTOL * max(1.0, float(np.max(np.abs(o32))))
    pbar = 4.0 * float(np.max(np.abs(p32 - p64))) + 2e-6 * float(np.max(np.abs(p64)))
    d_out, d_pred = float(np.max(np.abs(out_s - out_p))), float(np.max(np.abs(pred_s - pred_p)))
    print(f"stream vs primed D={D} variant={variant}: out {'bit-identical' if np.array_equal(out_s, out_p) else f'max diff {d_out:.3e}'}, "
          f"pred {'bit-identical' if np.array_equal(pred_s, pred_p) else f'max diff {d_pred:.3e}'}")
    assert float(np.max(np.abs(out_s - o32))) <= bar and d_out <= bar
    assert float(np.max(np.abs(pred_s - p64))) <= pbar and d_pred <= pbar
    be.set_params(m.effective_params(), n, length + 1, train=False)
    w = be.sample(noise)
    w_s, none = be.stream(None, None, 0, None, noise, False, n=n)
    d_w = float(np.max(np.abs(w_s - w)))
    print(f"stream vs sample D={D} variant={variant}: out {'bit-identical' if np.array_equal(w_s, w) else f'max diff {d_w:.3e}'}")
    assert none is None and d_w <= OUT_RTOL * max(1.0, float(np.max(np.abs(w))))


def test_stream_error_returns():
    """(d) every error return of the contract."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import HipScan
    D, n, forced, length, k0 = 8, 3, 4, 5, 6
    m = _model(D, n, AUTO)
    be = m._get_backend()
    lib, h, dev = be._lib, be._h, be.device
    audio = torch.zeros((n, forced + 1), dtype=torch.float32, device=dev)
    noise = torch.zeros((n, length), dtype=torch.float32, device=dev)
    out = torch.empty((n, length), dtype=torch.float32, device=dev)
    pred = torch.empty((n, forced), dtype=torch.float32, device=dev)
    st = be.stream_state(n)
    OK, BAD, STATE = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE

    def call(sin=st.data_ptr(), sout=st.data_ptr(), k0_=k0, audio_p=audio.data_ptr(), n_audio=n, forced_=forced, noise_p=noise.data_ptr(),
             length_=length, n_=n, out_p=out.data_ptr(), lib_=lib, h_=h):
        return lib_.cmps_psi_stream(h_, sin, sout, k0_, audio_p, n_audio, forced_, noise_p, length_, n_, out_p, pred.data_ptr(), be._stream())

    fresh = HipScan(D)
    assert call(lib_=fresh._lib, h_=fresh._h) == STATE                                  # before cmps_set_params
    be.set_params(m.effective_params(), n, k0 + forced + length, train=False)          # one row short
    assert call() == BAD
    msg = lib.cmps_last_error(h).decode()
    assert f"T >= {k0 + forced + length + 1}" in msg, msg
    be.set_params(m.effective_params(), n, k0 + forced + length + 1, train=False)      # exactly enough rows
    assert call(sin=None, sout=st.data_ptr(), k0_=0, forced_=forced, length_=2) == OK   # (a start, so that the record read below is a state)
    assert call() == OK
    assert call(sout=None) == OK and call(n_audio=1) == OK
    assert call(forced_=0, audio_p=None) == OK and call(length_=0, noise_p=None, out_p=None) == OK
    torch.cuda.synchronize()
    assert call(sin=None) == BAD and call(k0_=0) == BAD                                 # state_in == NULL <=> k0 == 0
    assert call(sin=None, k0_=0) == OK
    assert call(n_=0, n_audio=0) == BAD
    assert call(forced_=-1) == BAD and call(length_=-1) == BAD and call(k0_=-1) == BAD
    assert call(forced_=0, length_=0) == BAD
    assert call(audio_p=None) == BAD                                                    # forced > 0
    assert call(noise_p=None) == BAD and call(out_p=None) == BAD                        # length > 0
    assert call(n_audio=2) == BAD
    assert call(k0_=k0 + 1) == BAD and "T >=" in lib.cmps_last_error(h).decode()
    assert lib.cmps_psi_stream(None, None, None, 0, audio.data_ptr(), n, forced, noise.data_ptr(), length, n, out.data_ptr(), None,
                               None) == BAD
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    R = (0.1 * rng.standard_normal((D, D))).astype(np.float32)
    Q = (0.01 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64)
    be.legacy_set_params(R, Q, 1e-3, n, k0 + forced + length + 1, train=False)
    assert call() == STATE
    assert "legacy" in lib.cmps_last_error(h).decode()


@pytest.mark.parametrize("D,variant", [(8, AUTO), (32, WAVE), (48, AUTO), (128, WIDE), (48, BLOCK), (8, BLOCK)])
def test_stream_kernel_names(D, variant):
    """(e) the launch is recorded under the family the variant resolves to."""
    n = 2
    m = _model(D, n, variant)
    be = m._get_backend()
    be.set_params(m.effective_params(), n, 8, train=False)
    be.kernel_events(True)
    st = be.stream_state(n)
    be.stream(None, st, 0, np.zeros((1, 3), np.float32), np.zeros((2, n), np.float32), True, n=n)
    be.stream(st, st, 4, None, np.zeros((3, n), np.float32), False, n=n)
    times = be.kernel_times()
    assert list(times) == [FAMILY_NAME[_expected_family(D, variant)]] and times[list(times)[0]][1] == 2


def test_open_stream_follow_generate_matches_continue_clip():
    """(f) open_stream -> follow -> generate against continue_clip (another T of the tables: the bar, not the bits)."""
    D, P, length, n = 8, 63, 70, 3
    m = _model(D, n, WAVE)
    prime, noise = PR.case_inputs(D, P, length, n)
    ref, _ = PR.case_reference(D, P, length, n, "f32")
    want = m.continue_clip(prime, n, length, noise=noise)
    pred_want = m.predict_increments(prime)
    st = m.open_stream(n, 300)
    pred = np.concatenate([st.follow(prime[:, :10]), st.follow(prime[:, 10:])], axis=1)
    got = np.concatenate([st.generate(1, noise=noise[:1]), st.generate(length - 1, noise=noise[1:])], axis=1)
    assert st.position == P + length and got.dtype == np.float32 and got.shape == (n, length)
    bar = OUT_RTOL * max(1.0, float(np.max(np.abs(ref)))) / float(m.A)
    assert float(np.max(np.abs(got - want))) <= bar
    assert float(np.max(np.abs(pred - pred_want))) <= 2e-6 * float(np.max(np.abs(pred_want)))
    with pytest.raises(ValueError):
        st.generate(300 - P - length + 1)


def test_fill_gaps_on_the_gpu():
    """(f) D = 8, T = 200, one gap of 40 samples: the known samples come back unchanged, the gap is finite and differs between two paths."""
    D, T, n = 8, 200, 2
    m = _model(D, n, AUTO)
    clip = O.damped_sine(1, T, m.hparams.delta_t, seed=3)[0]
    known = np.ones(T, bool)
    known[90:130] = False
    wave = m.open_stream(n, T, temp=0.5, seed=1).fill_gaps(clip, known)
    assert wave.shape == (n, T) and np.array_equal(wave[:, known], np.tile(clip[known], (n, 1)))
    gap = wave[:, 90:130]
    assert np.all(np.isfinite(gap)) and not np.array_equal(gap[0], gap[1])


def test_sample_main_segment_on_the_gpu(tmp_path):
    """(f) python -m audio_mps_amd.sample --segment 64 on the checkpoint recipe of test_sample_main_continues_a_wav_on_the_gpu: the clip,
    then the stream's continuation, which is the one-shot command's within the out bar (the same noise; tables of the same T)."""
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
    args = ["--modeldir", ckdir, "--prime", wav, "--sample_duration", "200", "--num_samples", "2", "--seed", "4"]
    one = S.main(args + ["--out_dir", os.path.join(tmp_path, "one")])
    out_dir = os.path.join(tmp_path, "seg")
    seg = S.main(args + ["--out_dir", out_dir, "--segment", "64"])
    assert seg.shape == (2, 500) and np.all(np.isfinite(seg))
    assert sorted(os.listdir(out_dir)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
    assert np.array_equal(np.load(os.path.join(out_dir, "samples.npy")), seg)
    assert np.array_equal(seg[:, :300], one[:, :300]) and not np.array_equal(seg[0, 300:], seg[1, 300:])
    A = float(m.A)
    assert float(np.max(np.abs(seg - one))) <= OUT_RTOL * max(1.0, A * float(np.max(np.abs(one[:, 300:] - one[:, 299:300])))) / A
