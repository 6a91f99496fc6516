"""The scored stream on a real MI355X: cmps_psi_stream_score in the wave, wide and block kernels.  (a) cutting a scored run into more
segments changes no bit of nll, loss, pred or the state record; (b) scoring perturbs nothing: pred and the record are cmps_psi_stream's on
the same segments; (c) nll and the totals against the oracle composition (tests/_score_ref.py); (d) the totals against cmps_psi_loss_fwd;
(e) score / generate / score anchored; (f) error returns, kernel names, the memory contract, the host layer.

Bars:
  * nll per step:  max |hip - nll64| <= 4 * max |nll32 - nll64| + 2^-22   (the factor of the pred bar of tests/test_gpu_stream.py; the floor
                   is two roundings of 1 + z at 1)
  * totals:        |loss - total32| <= 1e-5 * max(|l|, 1)                 (the project's loss bar)
  * forward:       |loss - cmps_psi_loss_fwd| <= 2e-5 * max(|l|, 1)       (both within 1e-5 of the same oracle)
"""
import os

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O
import _guard as G
import _primed_ref as PR
import _score_ref as SC
from test_gpu_primed import AUTO, BLOCK, WAVE, WIDE, OUT_RTOL, _expected_family, _model
from test_gpu_stream import run_plan as run_followed

pytestmark = pytest.mark.gpu

# (D, variant, n, scored segments): a padded D, single-step segments, both sides of the 64-step chunk, an odd path count in the
# pair-of-paths kernel, every family
CASES = [(20, WAVE, 1, (1, 3)),
         (8, WAVE, 3, (63, 1, 1, 65)),
         (32, WAVE, 4, (64, 64, 65)),
         (48, AUTO, 3, (65, 1, 99)),
         (128, WIDE, 2, (33, 37)),
         (48, BLOCK, 2, (70, 66)),
         (32, BLOCK, 3, (100, 100))]
FAMILY_NAME = {WAVE: "k_sample_wave_score", WIDE: "k_sample_wide_score", BLOCK: "k_sample_block_score"}
NLL_FLOOR = 2.0 ** -22
LOSS_RTOL = 1e-5


def refine(segments):
    """Every segment cut again at its middle and one step in."""
    return tuple(m for _, m, _ in SC.refine([(SC.SCORE, s) for s in segments]))


def run_scored(m, segments, clip, n, same_state=False, null_final=False, repeat_params=False):
    """The segments call by call through HipScan.stream_score, segment s on clip[:, f0 : f0 + steps + 1]: (nll [n, F], loss [n] behind
    the last segment, pred [n, F], the final state record as bytes, or None with null_final).  The state alternates between two tensors, or
    (same_state) is read and written in place; repeat_params calls set_params again, with the same arguments, behind the first segment."""
    be = m._get_backend()
    F = sum(segments)
    be.set_params(m.effective_params(), n, F + 1, train=False)
    states = [be.stream_state(n), be.stream_state(n)]
    nlls, preds, cur, f0 = [], [], None, 0
    loss = np.full(n, np.nan, np.float32)                          # (not read at k0 = 0)
    for idx, f in enumerate(segments):
        if idx == len(segments) - 1 and null_final:
            nxt = None
        elif same_state:
            nxt = states[0]
        else:
            nxt = states[1] if cur is states[0] else states[0]
        nll, loss, pred = be.stream_score(cur, nxt, f0, clip[:, f0:f0 + f + 1], want_nll=True, want_pred=True, n=n, loss=loss)
        assert nll.shape == (n, f) and pred.shape == (n, f) and loss.shape == (n,)
        nlls.append(nll)
        preds.append(pred)
        cur, f0 = nxt, f0 + f
        if repeat_params and idx == 0:
            be.set_params(m.effective_params(), n, F + 1, train=False)
    return np.concatenate(nlls, axis=1), loss, np.concatenate(preds, axis=1), (None if cur is None else cur.cpu().numpy())


def _clip(D, n, segments):
    return SC.case_clip(D, n, sum(segments) + 1)


@pytest.mark.parametrize("D,variant,n,segments", CASES)
def test_cuts_are_bit_exact(D, variant, n, segments):
    """(a) the plan as written against the plan with every segment cut again: nll, loss, pred and the final record; the same with the
    state updated in place, a NULL final state_out, set_params repeated between two segments, and one shared signal against its tiled copy."""
    m = _model(D, n, variant)
    assert m._get_backend().variant == _expected_family(D, variant)
    clip = _clip(D, n, segments)
    fine = refine(segments)
    assert len(fine) > len(segments) and sum(fine) == sum(segments)
    nll, loss, pred, rec = run_scored(m, segments, clip, n)
    assert np.all(np.isfinite(nll)) and np.all(np.isfinite(loss)) and np.all(np.isfinite(pred)) and rec.any() and nll.any()
    for kw in ({}, {"same_state": True}, {"repeat_params": True}, {"null_final": True}):
        n2, l2, p2, r2 = run_scored(m, fine, clip, n, **kw)
        assert np.array_equal(n2, nll) and np.array_equal(l2, loss) and np.array_equal(p2, pred), kw
        assert (r2 is None) if kw.get("null_final") else np.array_equal(r2, rec), kw
    one = np.ascontiguousarray(clip[n - 1:n])
    a = run_scored(m, fine, one, n)                                                      # n_audio = 1
    b = run_scored(m, segments, np.tile(one, (n, 1)), n)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(a[0][0], a[0][j]) for j in range(n))                       # one signal: every path scores it alike


@pytest.mark.parametrize("D,variant,n,segments", CASES)
def test_scoring_perturbs_nothing(D, variant, n, segments):
    """(b) pred and the final record of the scored run are cmps_psi_stream's on the same followed segments, bit for bit, in every family
    (measured on an MI355X: identical in all seven cases)."""
    m = _model(D, n, variant)
    clip = _clip(D, n, segments)
    _, _, pred, rec = run_scored(m, segments, clip, n)
    _, pred_f, rec_f = run_followed(m, tuple((f, 0) for f in segments), clip, None, n)
    assert np.array_equal(pred, pred_f) and np.array_equal(rec, rec_f)


@pytest.mark.parametrize("D,variant,n,segments", CASES)
def test_scores_match_oracle_composition(D, variant, n, segments):
    """(c) nll against the float64 composition in units of the float32 composition's own distance from it, loss against the float32 total;
    (d) loss against cmps_psi_loss_fwd on the same clips.

    Measured on an MI355X (cases in the order of CASES; total err and vs fwd relative to max(|l|, 1), bars 1e-05 and 2e-05):
      D   variant n  steps  max|nll|   |hip - f64|  |o32 - f64|  ratio  nll bar    total err  vs fwd
      20  WAVE    1  4      1.752e-03  5.385e-08    5.397e-08    1.00   4.543e-07  4.657e-10  0.000e+00
      8   WAVE    3  130    7.605e-03  2.198e-07    1.997e-07    1.10   1.037e-06  2.906e-07  1.788e-07
      32  WAVE    4  193    1.236e-02  4.076e-07    4.076e-07    1.00   1.869e-06  3.576e-07  4.172e-07
      48  AUTO    3  165    1.148e-02  2.465e-07    2.465e-07    1.00   1.225e-06  5.960e-08  1.192e-07
      128 WIDE    2  70     1.229e-02  1.763e-07    1.768e-07    1.00   9.455e-07  7.451e-08  0.000e+00
      48  BLOCK   2  136    1.020e-02  1.906e-07    1.910e-07    1.00   1.003e-06  1.788e-07  1.192e-07
      32  BLOCK   3  200    1.151e-02  4.196e-07    4.196e-07    1.00   1.917e-06  2.682e-07  2.384e-07"""
    m = _model(D, n, variant)
    clip = _clip(D, n, segments)
    nll32, total32, _ = SC.case_reference(D, n, segments, "f32")
    nll64, total64, _ = SC.case_reference(D, n, segments, "f64")
    nll, loss, _, _ = run_scored(m, segments, clip, n)
    d_hip = float(np.max(np.abs(nll.astype(np.float64) - nll64)))
    d_o32 = float(np.max(np.abs(nll32.astype(np.float64) - nll64)))
    bar = 4.0 * d_o32 + NLL_FLOOR
    scale = np.maximum(np.abs(total32), 1.0)
    d_tot = float(np.max(np.abs(loss - total32) / scale))
    fwd = m.loss_per_clip(clip)
    d_fwd = float(np.max(np.abs(loss - fwd) / np.maximum(np.abs(fwd), 1.0)))
    print(f"score D={D} variant={variant} n={n} steps={sum(segments)}: max|nll| {float(np.max(np.abs(nll))):.3e}  |hip - f64| {d_hip:.3e}  "
          f"|o32 - f64| {d_o32:.3e}  nll bar {bar:.3e}  total err {d_tot:.3e} (bar {LOSS_RTOL:.0e})  |hip - f64| total "
          f"{float(np.max(np.abs(loss - total64))):.3e}  vs fwd {d_fwd:.3e} (bar {2 * LOSS_RTOL:.0e})")
    assert d_o32 > 0 and float(np.max(np.abs(nll32))) > 1e-3                             # the bars are not vacuous
    assert d_hip <= bar
    assert d_tot <= LOSS_RTOL
    assert d_fwd <= 2 * LOSS_RTOL


@pytest.mark.parametrize("D,variant", [(32, WAVE), (48, WIDE)])
def test_score_generate_score(D, variant):
    """(e) score 40 steps, generate 30, score 50 anchored, against the composition: out at the stream tests' bar, nll and the total as in
    (c); the generated run leaves the total alone.  Measured on an MI355X: WAVE D = 32 out err 4.470e-08, nll |hip - f64| 1.472e-07
    (|o32 - f64| 1.472e-07), total err 1.788e-07; WIDE D = 48 out err 5.960e-08, nll 1.079e-07 (1.079e-07), total err 2.682e-07."""
    n = 3
    m = _model(D, n, variant)
    be = m._get_backend()
    hp, var = PR.case_hparams(D, n), PR.case_variables(D, n)
    plan = [(SC.SCORE, 40), (SC.SAMPLE, 30), (SC.SCORE, 50, True)]
    clip = SC.case_clip(D, n, SC.clip_columns(plan))
    assert clip.shape == (n, 92)
    noise = O.sample_noise(hp, n, 30, temp=0.5, seed=D)
    nll32, total32, pred32, out32, _ = SC.score_reference(hp, var, plan, clip, noise, "f32")
    nll64, _, pred64, _, _ = SC.score_reference(hp, var, plan, clip, noise, "f64")
    be.set_params(m.effective_params(), n, 121, train=False)
    st = be.stream_state(n)
    a, loss_a, pa = be.stream_score(None, st, 0, clip[:, :41], want_pred=True, n=n)
    out, none = be.stream(st, st, 40, None, noise, False, n=n)
    b, loss_b, pb = be.stream_score(st, st, 70, clip[:, 41:], want_pred=True, n=n, loss=loss_a)
    nll, pred = np.concatenate([a, b], axis=1), np.concatenate([pa, pb], axis=1)
    seq = loss_a.copy()
    for j in range(50):
        seq = (seq + b[:, j]).astype(np.float32)
    assert none is None and np.array_equal(seq, loss_b)                                  # continued from loss_a: nothing added in between
    d_hip, d_o32 = float(np.max(np.abs(nll - nll64))), float(np.max(np.abs(nll32 - nll64)))
    err = float(np.max(np.abs(out - out32)))
    print(f"mixed D={D} variant={variant}: out err {err:.3e}  nll |hip - f64| {d_hip:.3e}  |o32 - f64| {d_o32:.3e}  total err "
          f"{float(np.max(np.abs(loss_b - total32))):.3e}")
    assert err <= OUT_RTOL * max(1.0, float(np.max(np.abs(out32))))
    assert d_hip <= 4.0 * d_o32 + NLL_FLOOR
    assert float(np.max(np.abs(loss_b - total32) / np.maximum(np.abs(total32), 1.0))) <= LOSS_RTOL
    assert float(np.max(np.abs(pred - pred64))) <= 4.0 * float(np.max(np.abs(pred32 - pred64))) + 2e-6 * float(np.max(np.abs(pred64)))
    # the same run with the scored segments followed: the waveform keeps its bits
    st2 = be.stream_state(n)
    be.stream(None, st2, 0, clip[:, :41], None, True, n=n)
    out2, _ = be.stream(st2, st2, 40, None, noise, False, n=n)
    assert np.array_equal(out2, out)


def test_score_error_returns():
    """(f) every error return of the contract."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import HipScan
    D, n, forced, k0 = 8, 3, 4, 6
    m = _model(D, n, AUTO)
    be = m._get_backend()
    lib, h, dev = be._lib, be._h, be.device
    audio = torch.zeros((n, forced + 1), dtype=torch.float32, device=dev)
    nll = torch.empty((n, forced), dtype=torch.float32, device=dev)
    pred = torch.empty((n, forced), dtype=torch.float32, device=dev)
    loss = torch.zeros(n, dtype=torch.float32, device=dev)
    st = be.stream_state(n)
    OK, BAD, STATE = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE

    def call(sin=st.data_ptr(), sout=st.data_ptr(), k0_=k0, audio_p=audio.data_ptr(), n_audio=n, forced_=forced, n_=n, nll_p=nll.data_ptr(),
             loss_p=loss.data_ptr(), pred_p=pred.data_ptr(), lib_=lib, h_=h):
        return lib_.cmps_psi_stream_score(h_, sin, sout, k0_, audio_p, n_audio, forced_, n_, nll_p, loss_p, pred_p, be._stream())

    fresh = HipScan(D)
    assert call(lib_=fresh._lib, h_=fresh._h) == STATE                                  # before cmps_set_params
    be.set_params(m.effective_params(), n, k0 + forced, train=False)                   # one row short
    assert call() == BAD
    msg = lib.cmps_last_error(h).decode()
    assert f"T >= {k0 + forced + 1}" in msg and "cmps_psi_stream_score" in msg, msg
    be.set_params(m.effective_params(), n, k0 + forced + 1, train=False)               # exactly enough rows
    assert call(sin=None, k0_=0) == OK                                                  # (a start, so that the record read below is a state)
    assert call() == OK
    assert call(sout=None) == OK and call(n_audio=1) == OK and call(nll_p=None) == OK and call(pred_p=None) == OK
    torch.cuda.synchronize()
    assert call(sin=None) == BAD and call(k0_=0) == BAD                                 # state_in == NULL <=> k0 == 0
    assert call(n_=0, n_audio=0) == BAD
    assert call(forced_=0) == BAD and call(forced_=-1) == BAD and call(k0_=-1) == BAD   # a scored segment makes one step at least
    assert call(audio_p=None) == BAD
    assert call(loss_p=None) == BAD and "loss_dev" in lib.cmps_last_error(h).decode()
    assert call(n_audio=2) == BAD
    assert call(k0_=k0 + 1) == BAD and "T >=" in lib.cmps_last_error(h).decode()
    assert lib.cmps_psi_stream_score(None, None, None, 0, audio.data_ptr(), n, forced, n, None, loss.data_ptr(), None, None) == BAD
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    R = (0.1 * rng.standard_normal((D, D))).astype(np.float32)
    Q = (0.01 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64)
    be.legacy_set_params(R, Q, 1e-3, n, k0 + forced + 1, train=False)
    assert call() == STATE
    assert "legacy" in lib.cmps_last_error(h).decode()


@pytest.mark.parametrize("D,variant", [(8, AUTO), (32, WAVE), (48, AUTO), (128, WIDE), (48, BLOCK), (8, BLOCK)])
def test_score_kernel_names(D, variant):
    """(f) the launch is recorded under the family the variant resolves to, next to the followed segment's."""
    n = 2
    m = _model(D, n, variant)
    be = m._get_backend()
    be.set_params(m.effective_params(), n, 8, train=False)
    be.kernel_events(True)
    st = be.stream_state(n)
    _, loss, _ = be.stream_score(None, st, 0, np.zeros((1, 3), np.float32), n=n)
    be.stream_score(st, st, 2, np.zeros((n, 4), np.float32), want_nll=False, n=n, loss=loss)
    times = be.kernel_times()
    assert list(times) == [FAMILY_NAME[_expected_family(D, variant)]] and times[list(times)[0]][1] == 2


@pytest.mark.parametrize("D,variant,n", [(8, WAVE, 3), (48, AUTO, 3), (128, WIDE, 1), (48, BLOCK, 2)])
def test_score_memory_contract(D, variant, n):
    """(f) red zones round nll, loss, pred, the audio and both records under both fill patterns (loss_dev holds the NaN pattern at k0 = 0: it
    is not read there); nll_dev == NULL and pred_dev == NULL segments; every documented output fully written; the same bits as HipScan."""
    from test_gpu_memory_contract import both_fills, as_f32, psi_carried, sampler_model
    segments = (65, 1, 40)
    F = sum(segments)
    clip = SC.case_clip(D, n, F + 1)
    m = sampler_model(D, n)
    carried = psi_carried(D, variant)
    recs = {}

    def run(fill):
        drv = G.Driver(D, fill, variant)
        G.set_params(drv, m, n, F + 1, train=False)
        nbytes = int(drv.lib.cmps_psi_stream_state_bytes(drv.h, n))
        assert nbytes > 0 and nbytes % 16 == 0
        states = [drv.new("state_a", nbytes), drv.new("state_b", nbytes)]
        loss = drv.new("loss", 4 * n, out=torch.float32)
        names, f0 = ["loss"], 0
        for idx, f in enumerate(segments):
            a = drv.load(f"audio_{idx}", np.ascontiguousarray(clip[:, f0:f0 + f + 1], dtype=np.float32))
            nll = drv.new(f"nll_{idx}", 4 * n * f, out=torch.float32) if idx != 1 else None
            pred = drv.new(f"pred_{idx}", 4 * n * f, out=torch.float32) if idx != 2 else None
            names += [f"nll_{idx}"] * (nll is not None) + [f"pred_{idx}"] * (pred is not None)
            drv.call("cmps_psi_stream_score", states[(idx + 1) % 2] if idx else None, states[idx % 2], f0, a, n, f, n, nll, loss, pred)
            f0 += f
        drv.finish()
        recs[fill] = [(s.numpy(np.float32).reshape(n, -1), s.untouched_mask(torch.float32).cpu().numpy().reshape(n, -1)) for s in states]
        return drv.result(names)
    res = both_fills(run, f"cmps_psi_stream_score D={D}")
    for (ra, left), (rb, _) in zip(recs[G.NAN_FILL], recs[G.ZERO_FILL]):
        assert not left[:, :carried].any() and left[:, carried:].all()                   # the carried floats, and nothing behind them
        assert np.array_equal(ra[:, :carried].view(np.uint32), rb[:, :carried].view(np.uint32))
    from audio_mps_amd.scan import HipScan
    nll_h, loss_h, pred_h, rec_h = run_scored(sampler_model(D, n, backend=HipScan(D, variant=variant)), segments, clip, n)
    assert np.array_equal(as_f32(res, "loss"), loss_h)
    assert np.array_equal(as_f32(res, "nll_0", (n, 65)), nll_h[:, :65]) and np.array_equal(as_f32(res, "nll_2", (n, 40)), nll_h[:, 66:])
    assert np.array_equal(as_f32(res, "pred_0", (n, 65)), pred_h[:, :65]) and np.array_equal(as_f32(res, "pred_1", (n, 1)), pred_h[:, 65:66])
    final = recs[G.NAN_FILL][0][0]                                                       # segment 2 wrote state_a
    assert np.array_equal(final[:, :carried].view(np.uint32), rec_h.view(np.float32).reshape(n, -1)[:, :carried].view(np.uint32))


def test_sample_stream_score_matches_loss_per_clip():
    """(f) SampleStream.score / total_nll and nll_per_step(segment=...) against loss_per_clip (another kernel: the bar of (d))."""
    D, n, T = 8, 3, 200
    m = _model(D, n, WAVE)
    clip = SC.case_clip(D, n, T)
    want = m.loss_per_clip(clip)
    st = m.open_stream(n, T - 1)
    parts = [st.score(clip[:, :10]), st.score(clip[:, 10:11]), st.score(clip[:, 11:])]
    nll = np.concatenate(parts, axis=1)
    assert nll.shape == (n, T - 1) and nll.dtype == np.float32 and st.position == T - 1 and st.last_pred.shape == (n, T - 11)
    assert float(np.max(np.abs(st.total_nll - want) / np.maximum(np.abs(want), 1.0))) <= 2 * LOSS_RTOL
    with pytest.raises(ValueError):
        st.score(clip[:, :1])                                                            # one step past max_steps
    whole, cut = m.nll_per_step(clip), m.nll_per_step(clip, segment=64)
    assert np.array_equal(whole, nll) and np.array_equal(cut, nll)                       # (tables of the same T: the same bits)
    rows = whole.astype(np.float64).sum(axis=1)
    assert float(np.max(np.abs(rows - want) / np.maximum(np.abs(want), 1.0))) <= 2 * LOSS_RTOL
    # unscored steps leave the total alone, scored ones behind them continue it
    st = m.open_stream(n, 300, seed=1)
    st.score(clip[:, :120])
    t = st.total_nll.copy()
    st.generate(5)
    st.follow(clip[:, :4], anchor=True)
    assert np.array_equal(st.total_nll, t) and st.position == 119 + 5 + 3
    more = st.score(clip[:, 4:40])
    seq = t.copy()
    for j in range(36):
        seq = (seq + more[:, j]).astype(np.float32)
    assert more.shape == (n, 36) and np.array_equal(st.total_nll, seq) and not np.array_equal(seq, t)


def test_sample_main_score_on_the_gpu(tmp_path, capsys):
    """(f) python -m audio_mps_amd.sample --score on the checkpoint recipe of test_sample_main_segment_on_the_gpu, whole and in segments."""
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
    one = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", os.path.join(tmp_path, "one")])
    assert "total nll" in capsys.readouterr().out
    out_dir = os.path.join(tmp_path, "seg")
    seg = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", out_dir, "--segment", "64"])
    assert one.shape == (1, 299) and np.all(np.isfinite(one)) and np.array_equal(seg, one)
    assert sorted(os.listdir(out_dir)) == ["nll.npy", "pred.npy"]
    assert np.array_equal(np.load(os.path.join(out_dir, "nll.npy")), one) and np.load(os.path.join(out_dir, "pred.npy")).shape == (1, 299)
