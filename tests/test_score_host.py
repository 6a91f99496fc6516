"""Host layer of the scored stream without a GPU: the oracle composition (tests/_score_ref.py), the C symbol cmps_psi_stream_score and its
argument errors that need no device, SampleStream.score / total_nll / last_pred and PsiCMPS.nll_per_step on a stand-in backend that answers
`stream_score` from the composition, and `python -m audio_mps_amd.sample --score`.  The kernels are tested in tests/test_gpu_stream_score.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import make_audio
import _primed_ref as PR
import _stream_ref as SR
import _score_ref as SC
from test_stream_host import StreamBackend

from audio_mps_amd import HParams, PsiCMPS, RhoCMPS, _capi
from audio_mps_amd import sample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ScoreBackend(StreamBackend):
    """StreamBackend plus HipScan.stream_score: the same state dicts (psi, running sum, step), the running loss handed in and out."""

    def __init__(self, D, dtype="f32"):
        super().__init__(D, dtype)
        self.scored = []

    def stream_score(self, state_in, state_out, k0, audio, want_nll=True, want_pred=False, n=None, loss=None):
        assert (state_in is None) == (k0 == 0)
        audio = np.asarray(audio)
        forced = audio.shape[1] - 1
        assert forced >= 1 and audio.shape[0] in (1, n) and k0 + forced <= self.T - 1, "cmps_psi_stream_score: T of set_params too small"
        hp, var = self._oracle_model(n)
        start = None
        if state_in is not None:
            psi, run, k = state_in["carry"]
            assert k == k0 and state_in["n"] == n
            start = (psi, run, k, np.zeros(n, np.float32) if loss is None else np.asarray(loss, np.float32))
        self.scored.append((k0, forced, audio.shape[0]))
        nll, total, pred, _, carry = SC.score_reference(hp, var, [(SC.SCORE, forced)], audio, None, self.dtype, start=start, n=n)
        if state_out is not None:
            state_out["carry"] = carry[:3]
        return ((nll.astype(np.float32) if want_nll else None), total.astype(np.float32), (pred.astype(np.float32) if want_pred else None))


def _model(D=5, n=3):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    be = ScoreBackend(D)
    m = PsiCMPS(hp, seed=2, backend=be)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    return m, be


# ---------------------------------------------------------------------------------------------------
# the oracle composition
# ---------------------------------------------------------------------------------------------------
def test_composition_does_not_depend_on_the_segmentation():
    D, n = 5, 2
    hp, var = PR.case_hparams(D, n), PR.case_variables(D, n)
    plan = [(SC.SCORE, 5), (SC.FOLLOW, 3), (SC.SAMPLE, 4), (SC.SCORE, 6, True), (SC.SAMPLE, 2), (SC.FOLLOW, 2, True)]
    assert SC.plan_counts(plan) == (11, 5, 6, 2) and SC.clip_columns(plan) == 19
    clip = SC.case_clip(D, n, SC.clip_columns(plan))
    noise = O.sample_noise(hp, n, 6, temp=0.5, seed=D)
    fine = SC.refine(plan)
    assert len(fine) > len(plan)
    assert SC.refine([(SC.SCORE, 1), (SC.FOLLOW, 5, True)]) == [(SC.SCORE, 1, False), (SC.FOLLOW, 1, True), (SC.FOLLOW, 1, False),
                                                               (SC.FOLLOW, 3, False)]
    for dtype in ("f32", "f64"):
        nll, total, pred, out, carry = SC.score_reference(hp, var, plan, clip, noise, dtype)
        assert nll.shape == (n, 11) and total.shape == (n,) and pred.shape == (n, 16) and out.shape == (n, 6) and carry[2] == 22
        assert np.all(np.isfinite(nll)) and np.all(nll != 0)
        r2 = SC.score_reference(hp, var, fine, clip, noise, dtype)
        assert all(np.array_equal(a, b) for a, b in zip((nll, total, pred, out, carry[0]), (*r2[:4], r2[4][0])))
        # the total is the sequential sum of the increments, and resuming from a carry continues the same run
        seq = np.zeros(n, dtype=nll.dtype)
        for j in range(nll.shape[1]):
            seq = (seq + nll[:, j]).astype(nll.dtype)
        assert np.array_equal(seq, total)
        a = SC.score_reference(hp, var, plan[:3], clip[:, :9], noise[:4], dtype)
        assert a[4][4] == 8                                                  # the cursor: 8 forced steps read columns 0 .. 8
        b = SC.score_reference(hp, var, plan[3:], clip[:, 8:], noise[4:], dtype, start=a[4])
        assert np.array_equal(np.concatenate([a[0], b[0]], 1), nll) and np.array_equal(b[1], total)
        assert np.array_equal(np.concatenate([a[2], b[2]], 1), pred) and np.array_equal(np.concatenate([a[3], b[3]], 1), out)
        assert np.array_equal(b[4][0], carry[0]) and b[4][2] == carry[2]


def test_nothing_scored_is_the_stream_reference():
    D, n = 5, 2
    hp, var = PR.case_hparams(D, n), PR.case_variables(D, n)
    plan = ((5, 0), (0, 4), (3, 6))
    clip, noise = SR.case_inputs(D, plan, n)
    mine = [(kind, m) for f, s in plan for kind, m in ((SC.FOLLOW, f), (SC.SAMPLE, s)) if m]
    for dtype in ("f32", "f64"):
        out, pred, carry = SR.stream_reference(hp, var, plan, clip, noise, dtype)
        nll, total, pred2, out2, carry2 = SC.score_reference(hp, var, mine, clip, noise, dtype)
        assert nll.shape == (n, 0) and not total.any()
        assert np.array_equal(out2, out) and np.array_equal(pred2, pred)
        assert np.array_equal(carry2[0], carry[0]) and np.array_equal(carry2[1], carry[1]) and carry2[2] == carry[2]
        # scoring the forced steps instead changes neither
        scored = [(SC.SCORE if kind == SC.FOLLOW else kind, m) for kind, m in mine]
        r3 = SC.score_reference(hp, var, scored, clip, noise, dtype)
        assert np.array_equal(r3[3], out) and np.array_equal(r3[2], pred) and np.array_equal(r3[4][0], carry[0]) and r3[0].shape == (n, 8)


@pytest.mark.parametrize("D,n,segments", [(20, 1, (1, 3)), (8, 3, (63, 1, 1, 65)), (32, 4, (64, 64, 65)), (48, 3, (65, 1, 99)),
                                          (128, 2, (33, 37)), (48, 2, (70, 66)), (32, 3, (100, 100))])
def test_total_over_a_clip_is_psi_loss_per_clip(D, n, segments):
    """The float32 total of a clip scored from k0 = 0 equals O.psi_loss_per_clip bit for bit, on the inputs of the GPU cases, and these
    inputs keep every assertion of tests/test_gpu_stream_score.py non-vacuous."""
    nll32, total32, _ = SC.case_reference(D, n, segments, "f32")
    nll64, total64, _ = SC.case_reference(D, n, segments, "f64")
    clip = SC.case_clip(D, n, sum(segments) + 1)
    want = O.psi_loss_per_clip(PR.case_hparams(D, n), PR.case_variables(D, n), clip, "f32")
    assert total32.dtype == np.float32 and np.array_equal(total32, want)
    assert np.all(np.isfinite(nll32)) and 1e-3 < float(np.max(np.abs(nll32))) < 2e-2
    assert 0.0 < float(np.max(np.abs(nll32 - nll64))) < 1e-6 and float(np.max(np.abs(total32 - total64))) < 1e-5


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
    assert "cmps_psi_stream_score" in _capi.SYMBOLS and hasattr(lib, "cmps_psi_stream_score")
    assert re.search(r"^int cmps_psi_stream_score\(cmps_handle_t h, const void\* state_in_dev, void\* state_out_dev, int k0,", header, flags=re.M)
    for word in ("k_sample_wave_score", "k_sample_wide_score", "k_sample_block_score", "model.py:276-282", "1 + z <= 0"):
        assert word in header, word
    assert lib.cmps_version() == 500


def test_call_order_without_a_device():
    lib = _cdll()
    assert lib.cmps_psi_stream_score(None, None, None, 0, None, 1, 1, 1, None, None, None, None) == _capi.CMPS_ERR_BAD_ARG
    for D in (8, 48):
        h = ctypes.c_void_p()
        assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
        try:
            before = lib.cmps_psi_stream_state_bytes(h, 3)
            # a fresh handle: CMPS_ERR_STATE before any pointer or count is looked at
            assert lib.cmps_psi_stream_score(h, None, None, 0, None, 1, 0, 0, None, None, None, None) == _capi.CMPS_ERR_STATE
            assert b"cmps_psi_stream_score" in lib.cmps_last_error(h) and b"cmps_set_params" in lib.cmps_last_error(h)
            assert lib.cmps_psi_stream_state_bytes(h, 3) == before         # the record is cmps_psi_stream's
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
    want_loss = O.psi_loss_per_clip(*be._oracle_model(n), clips, "f32")     # (the numpy oracle: the composition's own primitives)
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
    with pytest.raises(ValueError):
        st.score(clips[:, :1])                                              # one step past max_steps
    assert st.position == T - 1 and np.array_equal(st.total_nll, want_loss)
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
    hp, var = be._oracle_model(n)
    plan = [(SC.SCORE, 40), (SC.SAMPLE, 30), (SC.FOLLOW, 9, True), (SC.SCORE, 70, True)]
    whole = np.concatenate([clip[:51], clip[50:]])
    nll, total, pred, out, _ = SC.score_reference(hp, var, plan, whole, noise, "f32")
    assert np.array_equal(np.concatenate([a, b], 1), nll) and np.array_equal(st.total_nll, total)
    assert np.array_equal(np.concatenate([pa, f, st.last_pred], 1), pred)
    for bad in (clip[None, None], np.zeros((n + 1, 4), np.float32)):
        with pytest.raises(ValueError):
            st.score(bad)


def test_score_on_a_rho_stream_says_psi_only():
    from _util import OracleBackend

    class RhoBackend(OracleBackend):
        def rho_stream_state(self, n):
            return {}

        def rho_stream(self, *a, **k):
            raise AssertionError("not reached")

    m = RhoCMPS(HParams(minibatch_size=2, bond_dim=4, initial_rank=2), seed=0, backend=RhoBackend(4))
    st = m.open_stream(2, 10)
    with pytest.raises(ValueError, match="PsiCMPS-only"):
        st.score(np.zeros(5, np.float32))
    assert st.position == 0 and st.last is None


# ---------------------------------------------------------------------------------------------------
# python -m audio_mps_amd.sample --score
# ---------------------------------------------------------------------------------------------------
def _checkpoint(tmp_path, D=4):
    from audio_mps_amd.train import Trainer
    from _util import OracleBackend
    hp = HParams(minibatch_size=4, bond_dim=D)
    m = PsiCMPS(hp, data_iterator=make_audio(4, 32, hp.delta_t, 1), seed=0, backend=OracleBackend(D))
    tr = Trainer(m, hp)
    tr.step()
    ckdir = os.path.join(tmp_path, "run")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    return hp, ckdir


def _loaded(ckdir, D):
    """The model sample.main builds from the checkpoint, on a ScoreBackend."""
    import math
    hp = HParams(delta_t=1.0 / 16000, h_reg=200.0 / (math.pi * 16000) ** 2)
    hp.bond_dim = D
    m = PsiCMPS(hp, seed=0, backend=ScoreBackend(D))
    for k, v in S.load_variables(ckdir).items():
        m.variables[k] = v
    return m


def test_sample_main_score(tmp_path, capsys):
    D, Tp = 4, 130
    hp, ckdir = _checkpoint(tmp_path, D)
    clip = 0.5 * O.damped_sine(1, Tp, hp.delta_t, seed=3)[0]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, clip, 16000)
    o1, o2, o3 = (os.path.join(tmp_path, d) for d in "abc")
    be = ScoreBackend(D)
    one = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", o1], backend=be)
    said = capsys.readouterr().out
    assert one.dtype == np.float32 and one.shape == (1, Tp - 1) and be.prepared[-1] == (1, Tp, False) and len(be.scored) == 1
    assert sorted(os.listdir(o1)) == ["nll.npy", "pred.npy"]
    assert np.array_equal(np.load(os.path.join(o1, "nll.npy")), one) and np.load(os.path.join(o1, "pred.npy")).shape == (1, Tp - 1)
    total = float(np.sum(one, dtype=np.float64))
    assert "total nll" in said and "mean per sample" in said and f"{total:.3g}"[:4] in said
    be = ScoreBackend(D)
    seg = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", o2, "--segment", "50"], backend=be)
    assert np.array_equal(seg, one) and [s[:2] for s in be.scored] == [(0, 50), (50, 50), (100, 29)]
    assert np.array_equal(np.load(os.path.join(o2, "pred.npy")), np.load(os.path.join(o1, "pred.npy")))
    # a .npy batch: one path per row
    npy = os.path.join(tmp_path, "clips.npy")
    np.save(npy, np.stack([clip, 0.5 * clip]))
    two = S.main(["--modeldir", ckdir, "--score", npy, "--out_dir", o3, "--segment", "64"], backend=ScoreBackend(D))
    assert two.shape == (2, Tp - 1) and np.all(np.isfinite(two)) and not np.array_equal(two[0], two[1])
    assert np.array_equal(two, PsiCMPS.nll_per_step(_loaded(ckdir, D), np.load(npy)))
    for bad in (["--segment", "0"], ["--prime", wav]):
        with pytest.raises(ValueError):
            S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", o1] + bad, backend=ScoreBackend(D))
    short = os.path.join(tmp_path, "short.npy")
    np.save(short, np.zeros(1, np.float32))
    with pytest.raises(ValueError):
        S.main(["--modeldir", ckdir, "--score", short, "--out_dir", o1], backend=ScoreBackend(D))


def test_sample_main_score_refuses_a_rho_checkpoint(tmp_path):
    from _util import OracleBackend
    D = 4
    m = RhoCMPS(HParams(bond_dim=D, initial_rank=2), seed=0, backend=False)
    ckdir = os.path.join(tmp_path, "rho")
    os.makedirs(ckdir)
    np.savez(os.path.join(ckdir, S.CKPT_NAME), **{"model/" + k: np.asarray(v) for k, v in m.variables.items()})
    npy = os.path.join(tmp_path, "clip.npy")
    np.save(npy, np.zeros(9, np.float32))
    with pytest.raises(ValueError, match="PsiCMPS-only"):
        S.main(["--modeldir", ckdir, "--score", npy, "--out_dir", os.path.join(tmp_path, "o")], backend=OracleBackend(D))
    assert not os.path.exists(os.path.join(tmp_path, "o"))


@pytest.mark.parametrize("N,S", [(1, None), (1, 1), (5, 1), (5, 2), (5, 5), (5, 8)])
def test_segments_cut_a_clip_as_the_written_out_loops_did(N, S):
    from audio_mps_amd.stream import segments
    cols = np.arange(N + 1)
    step = N if S is None else S
    old = [cols[:step + 1]] + [cols[a:a + step] for a in range(step + 1, N + 1, step)]     # "the anchor and S steps", then S steps at a time
    cuts = list(segments(N, S))
    got = [cols[lo:hi] for lo, hi in cuts]
    assert len(got) == len(old) and all(np.array_equal(g, o) for g, o in zip(got, old))
    assert np.array_equal(np.concatenate(got), cols) and all(len(g) >= 1 for g in got)
    assert cuts[0][0] == 0 and len(got[0]) == min(step + 1, N + 1)
    assert all(lo == before[1] for before, (lo, _) in zip(cuts[:-1], cuts[1:]))
    for bad in (0, -3):
        with pytest.raises(ValueError):
            list(segments(N, bad))
