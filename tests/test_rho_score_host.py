"""Host layer of the scored RhoCMPS stream without a GPU: the oracle composition (tests/_rho_score_ref.py), the C symbol
cmps_rho_stream_score and its argument errors that need no device, SampleStream.score / total_nll / last_pred / states / purity and
RhoCMPS.nll_per_step on a stand-in backend that answers `rho_stream_score` from the composition, and
`python -m audio_mps_amd.sample --score` on a rho_mps checkpoint.  The kernels are tested in tests/test_gpu_rho_stream_score.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import OracleBackend, make_audio
import _rho_primed_ref as RR
import _rho_stream_ref as RS
import _rho_score_ref as RC
from test_rho_stream_host import RhoStreamBackend

from audio_mps_amd import HParams, RhoCMPS, _capi
from audio_mps_amd import sample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RhoScoreBackend(RhoStreamBackend):
    """RhoStreamBackend plus HipScan.rho_stream_score: the same state dicts (rho, running sum, step), the running loss handed in and out."""

    def __init__(self, D, dtype="f32"):
        super().__init__(D, dtype)
        self.scored = []

    def rho_stream_score(self, state_in, state_out, k0, audio, want_nll=True, want_pred=False, n=None, loss=None, save_states=False):
        assert (state_in is None) == (k0 == 0)
        audio = np.asarray(audio)
        forced = audio.shape[1] - 1
        assert forced >= 1 and audio.shape[0] in (1, n) and k0 + forced <= self.T - 1, "cmps_rho_stream_score: T of set_params too small"
        assert not save_states or (self.train and n * forced <= self.rho_B * (self.rho_T - 1)), "CMPS_ERR_WORKSPACE"
        start = None
        if state_in is not None:
            rho, run, k = state_in["carry"]
            assert k == k0 and state_in["n"] == n
            start = (rho, run, k, np.zeros(n, np.float32) if loss is None else np.asarray(loss, np.float32))
        self.scored.append((k0, forced, audio.shape[0]))
        nll, total, pred, _, rhos, pur, carry = RC.rho_score_reference(*self._model(n), [(RC.SCORE, forced)], audio, None, self.dtype,
                                                                       start=start, n=n)
        if state_out is not None:
            state_out["carry"] = carry[:3]
        self.states = (rhos, pur) if save_states else None
        self.launches += 1
        return ((nll.astype(np.float32) if want_nll else None), total.astype(np.float32), (pred.astype(np.float32) if want_pred else None))


def _model(D=5, rank=2, n=3):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=0.1, initial_rank=rank, A=5.0)
    be = RhoScoreBackend(D)
    m = RhoCMPS(hp, seed=2, backend=be)
    m.variables["Rx"] *= np.float32(0.3)
    m.variables["Ry"] *= np.float32(0.3)
    return m, be


# ---------------------------------------------------------------------------------------------------
# the oracle composition
# ---------------------------------------------------------------------------------------------------
def test_composition_does_not_depend_on_the_segmentation():
    D, rank, n = 5, 2, 2
    ohp, ov, Wx, Wy = RR.oracle_side(RR.case_model(D, rank))
    plan = [(RC.SCORE, 5), (RC.FOLLOW, 3), (RC.SAMPLE, 4), (RC.SCORE, 6, True), (RC.SAMPLE, 2), (RC.FOLLOW, 2, True)]
    assert RC.plan_counts(plan) == (11, 5, 6, 2) and RC.clip_columns(plan) == 19
    clip = RC.case_clip(D, rank, n, RC.clip_columns(plan))
    noise = O.sample_noise(ohp, n, 6, temp=0.5, seed=D)
    fine = RC.refine(plan)
    assert len(fine) > len(plan)
    for dtype in ("f32", "f64"):
        nll, total, pred, out, rhos, pur, carry = RC.rho_score_reference(ohp, ov, Wx, Wy, plan, clip, noise, dtype)
        assert nll.shape == (n, 11) and total.shape == (n,) and pred.shape == (n, 16) and out.shape == (n, 6) and carry[2] == 22
        assert rhos.shape == (n, 22, D, D) and pur.shape == (n, 22) and np.array_equal(carry[0], rhos[:, -1])
        assert np.all(np.isfinite(nll)) and np.all(nll != 0)
        r2 = RC.rho_score_reference(ohp, ov, Wx, Wy, fine, clip, noise, dtype)
        assert all(np.array_equal(a, b) for a, b in zip((nll, total, pred, out, rhos, pur, carry[0]), (*r2[:6], r2[6][0])))
        # the total is the sequential sum of the increments, and resuming from a carry continues the same run
        seq = np.zeros(n, dtype=nll.dtype)
        for j in range(nll.shape[1]):
            seq = (seq + nll[:, j]).astype(nll.dtype)
        assert np.array_equal(seq, total)
        a = RC.rho_score_reference(ohp, ov, Wx, Wy, plan[:3], clip[:, :9], noise[:4], dtype)
        assert a[6][4] == 8                                                  # the cursor: 8 forced steps read columns 0 .. 8
        b = RC.rho_score_reference(ohp, ov, Wx, Wy, plan[3:], clip[:, 8:], noise[4:], dtype, start=a[6])
        assert np.array_equal(np.concatenate([a[0], b[0]], 1), nll) and np.array_equal(b[1], total)
        assert np.array_equal(np.concatenate([a[2], b[2]], 1), pred) and np.array_equal(np.concatenate([a[3], b[3]], 1), out)
        assert np.array_equal(np.concatenate([a[4], b[4]], 1), rhos) and np.array_equal(np.concatenate([a[5], b[5]], 1), pur)
        assert np.array_equal(b[6][0], carry[0]) and b[6][2] == carry[2]


def test_nothing_scored_is_the_rho_stream_reference():
    D, rank, n = 5, 2, 2
    ohp, ov, Wx, Wy = RR.oracle_side(RR.case_model(D, rank))
    plan = ((5, 0), (0, 4), (3, 6))
    clip, noise = RS.case_inputs(D, rank, plan, n)
    mine = [(kind, m) for f, s in plan for kind, m in ((RC.FOLLOW, f), (RC.SAMPLE, s)) if m]
    for dtype in ("f32", "f64"):
        out, pred, rhos, pur, carry = RS.rho_stream_reference(ohp, ov, Wx, Wy, plan, clip, noise, dtype)
        nll, total, pred2, out2, rhos2, pur2, carry2 = RC.rho_score_reference(ohp, ov, Wx, Wy, mine, clip, noise, dtype)
        assert nll.shape == (n, 0) and not total.any()
        assert np.array_equal(out2, out) and np.array_equal(pred2, pred) and np.array_equal(rhos2, rhos) and np.array_equal(pur2, pur)
        assert np.array_equal(carry2[0], carry[0]) and np.array_equal(carry2[1], carry[1]) and carry2[2] == carry[2]
        # scoring the forced steps instead changes neither
        scored = [(RC.SCORE if kind == RC.FOLLOW else kind, m) for kind, m in mine]
        r3 = RC.rho_score_reference(ohp, ov, Wx, Wy, scored, clip, noise, dtype)
        assert np.array_equal(r3[3], out) and np.array_equal(r3[2], pred) and np.array_equal(r3[4], rhos) and r3[0].shape == (n, 8)


@pytest.mark.parametrize("D,rank,variant,rank1,n,segments", RC.GPU_CASES)
def test_total_over_a_clip_is_rho_loss_per_clip(D, rank, variant, rank1, n, segments):
    """The float32 total of a clip scored from k0 = 0 equals O.rho_loss_per_clip bit for bit, on the inputs of the GPU cases, and these
    inputs keep every assertion of tests/test_gpu_rho_stream_score.py non-vacuous (1 + z away from 0, increments well above the float32
    composition's own distance from the float64 one, and that distance not 0)."""
    nll32, total32, _, rhos, pur = RC.case_reference(D, rank, n, segments, "f32")
    nll64, total64 = RC.case_reference(D, rank, n, segments, "f64")[:2]
    clip = RC.case_clip(D, rank, n, sum(segments) + 1)
    ohp, ov, Wx, Wy = RR.oracle_side(RR.case_model(D, rank))
    want = O.rho_loss_per_clip(ohp, ov, Wx, Wy, clip, "f32")
    assert total32.dtype == np.float32 and np.array_equal(total32, want)
    assert np.all(np.isfinite(nll32)) and 1e-3 < float(np.max(np.abs(nll32))) < 1.0
    assert 0.5 < float(np.min(np.exp(-nll64))) and float(np.max(np.exp(-nll64))) < 2.0          # 1 + z
    assert 0.0 < float(np.max(np.abs(nll32 - nll64))) < 1e-5 and float(np.max(np.abs(total32 - total64))) < 1e-4
    assert np.max(np.abs(np.einsum('abcc->ab', rhos) - 1)) <= 1e-4 and np.all(pur <= 1 + 1e-4) and np.all(pur >= 1.0 / D - 1e-4)


# ---------------------------------------------------------------------------------------------------
# the C ABI, no device touched
# ---------------------------------------------------------------------------------------------------
def _cdll():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    _capi._declare(lib)
    return lib


def test_symbol_declared_exported_and_in_the_header():
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    lib = _cdll()
    assert "cmps_rho_stream_score" in _capi.SYMBOLS and hasattr(lib, "cmps_rho_stream_score")
    assert re.search(r"^int cmps_rho_stream_score\(cmps_handle_t h, const void\* state_in_dev, void\* state_out_dev, int k0,", header, flags=re.M)
    for word in ("k_sample_rho_mfma_score", "k_sample_rho_score", "model.py:152-158", "1 + z <= 0"):
        assert word in header, word
    assert lib.cmps_version() == 500


def test_call_order_without_a_device():
    lib = _cdll()
    assert lib.cmps_rho_stream_score(None, None, None, 0, None, 1, 1, 1, None, None, None, 0, None) == _capi.CMPS_ERR_BAD_ARG
    for D in (8, 32, 48, 128):
        h = ctypes.c_void_p()
        assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
        try:
            # a fresh handle: CMPS_ERR_STATE before any pointer or count is looked at
            assert lib.cmps_rho_stream_score(h, None, None, 0, None, 1, 0, 0, None, None, None, 0, None) == _capi.CMPS_ERR_STATE
            msg = lib.cmps_last_error(h)
            assert b"cmps_rho_stream_score" in msg and b"cmps_set_params" in msg and b"cmps_rho_set_state" in msg
            assert lib.cmps_rho_stream_state_bytes(h, 3) == 0
        finally:
            lib.cmps_destroy(h)


# ---------------------------------------------------------------------------------------------------
# SampleStream.score on the stand-in backend: all bit-exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [1, 7, 64])
def test_score_in_blocks_equals_the_loss(blk):
    n, T = 3, 150
    m, be = _model(n=n)
    clips = make_audio(n, T, m.hparams.delta_t, 4)
    want_pred = m.predict_increments(clips)
    st = m.open_stream(n, T - 1)
    want_loss = O.rho_loss_per_clip(*be._model(n), clips, "f32")            # (the numpy oracle: the composition's own primitives)
    assert st.total_nll.shape == (n,) and st.total_nll.dtype == np.float32 and not st.total_nll.any() and st.last_pred is None
    parts, preds = [], []
    for a in range(0, T, blk):
        parts.append(st.score(clips[:, a:a + blk]))
        preds.append(st.last_pred)
    assert parts[0].shape == (n, blk - 1) and preds[0].shape == (n, blk - 1)      # the anchor makes no step
    nll = np.concatenate(parts, axis=1)
    assert nll.dtype == np.float32 and nll.shape == (n, T - 1)
    assert np.array_equal(st.total_nll, want_loss) and np.array_equal(np.concatenate(preds, axis=1), want_pred)
    assert st.position == T - 1 and np.array_equal(st.last, clips[:, -1])
    assert be.scored[0] == (0, max(blk - 1, 1), n) and all(k0 > 0 for k0, _, _ in be.scored[1:])
    launches = be.launches
    with pytest.raises(ValueError):
        st.score(clips[:, :1])                                              # one step past max_steps: refused, nothing changes
    assert st.position == T - 1 and np.array_equal(st.total_nll, want_loss) and be.launches == launches
    assert np.array_equal(m.nll_per_step(clips, segment=blk), nll) and np.array_equal(m.nll_per_step(clips), nll)
    with pytest.raises(ValueError):
        m.nll_per_step(clips, segment=0)
    with pytest.raises(ValueError):
        m.nll_per_step(clips[:, :1])


def test_score_follow_generate_alternate():
    n, T = 2, 121
    m, be = _model(n=n)
    clip = make_audio(1, T, m.hparams.delta_t, 8)[0]                       # one signal under every path
    noise = O.sample_noise(O.HParams(**m.hparams.values()), n, 30, temp=0.5, seed=1)
    st = m.open_stream(n, 200)
    ref = m.open_stream(n, 200)
    a = st.score(clip[:41])
    pa = st.last_pred
    assert a.shape == (n, 40) and np.array_equal(a[0], a[1]) and be.scored[-1] == (0, 40, 1)
    assert np.array_equal(pa, ref.follow(clip[:41]))                        # scoring perturbs nothing: pred, and below the waveform
    t40 = st.total_nll.copy()
    g = st.generate(30, noise=noise)
    assert np.array_equal(g, ref.generate(30, noise=noise)) and np.array_equal(st.total_nll, t40)
    f = st.follow(clip[41:51], anchor=True)                                 # unscored steps leave the total alone
    assert np.array_equal(f, ref.follow(clip[41:51], anchor=True)) and np.array_equal(st.total_nll, t40)
    b = st.score(clip[50:], anchor=True)
    assert b.shape == (n, 70) and st.position == 40 + 30 + 9 + 70 and be.scored[-1] == (79, 70, 1)
    assert np.array_equal(st.last_pred, ref.follow(clip[50:], anchor=True))
    seq = t40.copy()
    for j in range(70):
        seq = (seq + b[:, j]).astype(np.float32)
    assert np.array_equal(st.total_nll, seq) and np.array_equal(st.last, np.full(n, clip[-1], np.float32))
    # the whole against the composition
    plan = [(RC.SCORE, 40), (RC.SAMPLE, 30), (RC.FOLLOW, 9, True), (RC.SCORE, 70, True)]
    whole = np.concatenate([clip[:51], clip[50:]])
    nll, total, pred, out, _, _, _ = RC.rho_score_reference(*be._model(n), plan, whole, noise, "f32")
    assert np.array_equal(np.concatenate([a, b], 1), nll) and np.array_equal(st.total_nll, total)
    assert np.array_equal(np.concatenate([pa, f, st.last_pred], 1), pred)
    assert np.array_equal(g, (np.float32(clip[40]) + out.astype(np.float32) / np.float32(m.A)).astype(np.float32))
    for bad in (clip[None, None], np.zeros((n + 1, 4), np.float32)):
        with pytest.raises(ValueError):
            st.score(bad)


def test_keep_states_behind_a_score_call():
    """A keep_states stream passes save_states to the scored entry too: states() / purity() behind `score` are those behind `follow`."""
    n, Tp, S_ = 2, 41, 25
    m, be = _model(n=n)
    D = m.bond_d
    clips = make_audio(n, Tp, m.hparams.delta_t, 6)
    st = m.open_stream(n, Tp - 1, keep_states=S_)
    ref = m.open_stream(n, Tp - 1, keep_states=S_)
    rhos, purs = [], []
    for a, b in ((0, 21), (21, 41)):
        st.score(clips[:, a:b])
        rhos.append(st.states())
        purs.append(st.purity())
        ref.follow(clips[:, a:b])
        assert np.array_equal(rhos[-1], ref.states()) and np.array_equal(purs[-1], ref.purity())
    assert rhos[0].shape == (n, 20, D, D) and rhos[0].dtype == np.complex64 and purs[1].shape == (n, 20) and purs[1].dtype == np.float32
    whole = RC.rho_score_reference(*be._model(n), [(RC.SCORE, Tp - 1)], clips, None, "f32")
    assert np.array_equal(np.concatenate(rhos, axis=1), whole[4]) and np.array_equal(np.concatenate(purs, axis=1), whole[5])
    assert np.array_equal(st.total_nll, whole[1])
    small = m.open_stream(n, 100, keep_states=10)
    launches = be.launches
    with pytest.raises(ValueError):
        small.score(clips[:, :12])                                          # 11 steps: refused before any launch
    assert be.launches == launches and small.position == 0 and small.last is None and not small.total_nll.any()


def test_a_backend_without_the_entry_says_so():
    """A backend with the two stream entries and no rho_stream_score: the ValueError names it, and nothing has moved."""
    m = RhoCMPS(HParams(minibatch_size=2, bond_dim=4, initial_rank=2), seed=0, backend=RhoStreamBackend(4))
    st = m.open_stream(2, 10)
    with pytest.raises(ValueError, match="rho_stream_score"):
        st.score(np.zeros(5, np.float32))
    assert st.position == 0 and st.last is None and not st.total_nll.any()
    with pytest.raises(ValueError, match="PsiCMPS-only"):
        m.nll_per_step(np.zeros((2, 5), np.float32))


# ---------------------------------------------------------------------------------------------------
# python -m audio_mps_amd.sample --score on a rho_mps checkpoint
# ---------------------------------------------------------------------------------------------------
def _checkpoint(tmp_path, D=4, rank=3):
    from audio_mps_amd.train import Trainer
    hp = HParams(minibatch_size=4, bond_dim=D, initial_rank=rank)
    m = RhoCMPS(hp, data_iterator=make_audio(4, 32, hp.delta_t, 1), seed=0, backend=OracleBackend(D))
    tr = Trainer(m, hp)
    tr.step()
    ckdir = os.path.join(tmp_path, "run")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    return hp, ckdir


def _loaded(ckdir, D, rank):
    """The model sample.main builds from the checkpoint, on a RhoScoreBackend."""
    import math
    hp = HParams(delta_t=1.0 / 16000, h_reg=200.0 / (math.pi * 16000) ** 2)
    hp.bond_dim, hp.initial_rank = D, rank
    m = RhoCMPS(hp, seed=0, backend=RhoScoreBackend(D))
    for k, v in S.load_variables(ckdir).items():
        m.variables[k] = v
    return m


def test_sample_main_score_on_a_rho_checkpoint(tmp_path, capsys):
    D, rank, Tp = 4, 3, 130
    hp, ckdir = _checkpoint(tmp_path, D, rank)
    clip = 0.5 * O.damped_sine(1, Tp, hp.delta_t, seed=3)[0]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, clip, 16000)
    o1, o2, o3 = (os.path.join(tmp_path, d) for d in "abc")
    be = RhoScoreBackend(D)
    one = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", o1], backend=be)
    said = capsys.readouterr().out
    assert one.dtype == np.float32 and one.shape == (1, Tp - 1) and be.prepared[-1] == (1, Tp, False) and len(be.scored) == 1
    assert be.phi.shape == (rank, D)
    assert sorted(os.listdir(o1)) == ["nll.npy", "pred.npy"]
    assert np.array_equal(np.load(os.path.join(o1, "nll.npy")), one) and np.load(os.path.join(o1, "pred.npy")).shape == (1, Tp - 1)
    total = float(np.sum(one, dtype=np.float64))
    assert "total nll" in said and "mean per sample" in said and f"{total:.3g}"[:4] in said
    be = RhoScoreBackend(D)
    seg = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", o2, "--segment", "50"], backend=be)
    assert np.array_equal(seg, one) and [s[:2] for s in be.scored] == [(0, 50), (50, 50), (100, 29)]
    assert np.array_equal(np.load(os.path.join(o2, "pred.npy")), np.load(os.path.join(o1, "pred.npy")))
    # a .npy batch: one path per row
    npy = os.path.join(tmp_path, "clips.npy")
    np.save(npy, np.stack([clip, 0.5 * clip]))
    two = S.main(["--modeldir", ckdir, "--score", npy, "--out_dir", o3, "--segment", "64"], backend=RhoScoreBackend(D))
    assert two.shape == (2, Tp - 1) and np.all(np.isfinite(two)) and not np.array_equal(two[0], two[1])
    assert np.array_equal(two, _loaded(ckdir, D, rank).nll_per_step(np.load(npy)))
    for bad in (["--segment", "0"], ["--prime", wav], ["--device_noise"]):
        with pytest.raises(ValueError):
            S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", o1] + bad, backend=RhoScoreBackend(D))
