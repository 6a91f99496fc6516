"""Host layer of the resumable RhoCMPS sampler without a GPU: the two C symbols, RhoCMPS.open_stream / SampleStream (follow, generate,
fill_gaps, states, purity) and `python -m audio_mps_amd.sample --segment` on a rho_mps checkpoint, on a stand-in backend that answers
`rho_stream_state` / `rho_stream` from the oracle composition (tests/_rho_stream_ref.py), carrying (rho, running sum).  The kernels
themselves are tested in tests/test_gpu_rho_stream.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import OracleBackend, make_audio
import _rho_primed_ref as RR
import _rho_stream_ref as RS
import _stream_ref as SR
from test_rho_primed_host import RhoPrimedBackend
from test_stream_host import _model as _psi_model

from audio_mps_amd import HParams, PsiCMPS, RhoCMPS, _capi
from audio_mps_amd import sample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RhoStreamBackend(RhoPrimedBackend):
    """RhoPrimedBackend plus HipScan's two rho stream entries; a state is a dict holding the composition's carry, with cmps_rho_stream's
    checks: the tables' T is set_params's, the stash's capacity rho_set_state's."""

    def rho_set_state(self, phi, B, T, train=True):
        super().rho_set_state(phi, B, T, train)
        assert T <= self.T, "cmps_rho_set_state: T exceeds T of cmps_set_params"
        self.rho_B, self.rho_T = B, T
        self.launches = 0

    def rho_stream_state(self, n):
        return {"n": n, "carry": None}

    def rho_stream(self, state_in, state_out, k0, audio, noise, want_pred=False, n=None, save_states=False):
        assert (state_in is None) == (k0 == 0)
        forced = 0 if audio is None else np.shape(audio)[1] - 1
        length = 0 if noise is None else np.shape(noise)[0]
        assert forced + length >= 1 and k0 + forced + length <= self.T - 1, "cmps_rho_stream: T of set_params too small"
        n = n if noise is None else np.shape(noise)[1]
        assert not save_states or (self.train and n * (forced + length) <= self.rho_B * (self.rho_T - 1)), "CMPS_ERR_WORKSPACE"
        start = None
        if state_in is not None:
            start = state_in["carry"]
            assert start[2] == k0 and state_in["n"] == n
        out, pred, rhos, pur, carry = RS.rho_stream_reference(*self._model(n), [(forced, length)],
                                                              audio if forced else np.zeros((n, 1), np.float32),
                                                              noise if length else None, self.dtype, start=start, n=n)
        if state_out is not None:
            state_out["carry"] = carry
        self.states = (rhos, pur) if save_states else None
        self.launches += 1
        return out.astype(np.float32), (pred.astype(np.float32) if want_pred else None)


def _model(D=5, rank=2, n=3):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=0.1, initial_rank=rank, A=5.0)
    be = RhoStreamBackend(D)
    m = RhoCMPS(hp, seed=2, backend=be)
    m.variables["Rx"] *= np.float32(0.3)
    m.variables["Ry"] *= np.float32(0.3)
    return m, be


# ---------------------------------------------------------------------------------------------------
# the C ABI, no device touched
# ---------------------------------------------------------------------------------------------------
def _cdll():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    _capi._declare(lib)
    return lib


def test_symbols_declared_exported_and_in_the_header():
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    lib = _cdll()
    for name in ("cmps_rho_stream_state_bytes", "cmps_rho_stream"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
        assert re.search(r"^\w[\w \*]*\b%s\(" % name, header, flags=re.M), name
    assert lib.cmps_version() == 500


def test_state_bytes_and_call_order_without_a_device():
    lib = _cdll()
    assert lib.cmps_rho_stream_state_bytes(None, 1) == 0
    assert lib.cmps_rho_stream(None, None, None, 0, None, 1, 0, None, 1, 1, None, None, 0, None) == _capi.CMPS_ERR_BAD_ARG
    for D in (8, 32, 48, 128):
        h = ctypes.c_void_p()
        assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
        try:
            # the record belongs to the rank of cmps_rho_set_state: no size before it, whatever n
            assert [lib.cmps_rho_stream_state_bytes(h, n) for n in (1, 0, -3, 1000)] == [0, 0, 0, 0]
            # a fresh handle: CMPS_ERR_STATE before any pointer is looked at
            assert lib.cmps_rho_stream(h, None, None, 0, None, 1, 0, None, 1, 1, None, None, 0, None) == _capi.CMPS_ERR_STATE
            msg = lib.cmps_last_error(h)
            assert b"cmps_set_params" in msg and b"cmps_rho_set_state" in msg
        finally:
            lib.cmps_destroy(h)


# ---------------------------------------------------------------------------------------------------
# the oracle composition
# ---------------------------------------------------------------------------------------------------
def test_reference_does_not_depend_on_the_segmentation():
    D, rank, n = 5, 2, 2
    ohp, ov, Wx, Wy = RR.oracle_side(RR.case_model(D, rank))
    plan = ((5, 0), (0, 4), (3, 6))
    clip, noise = RS.case_inputs(D, rank, plan, n)
    for dtype in ("f32", "f64"):
        out, pred, rhos, pur, carry = RS.rho_stream_reference(ohp, ov, Wx, Wy, plan, clip, noise, dtype)
        assert out.shape == (n, 10) and pred.shape == (n, 8) and rhos.shape == (n, 18, D, D) and pur.shape == (n, 18)
        fine = SR.refine(plan)
        assert fine != list(plan) and len(fine) > len(plan)
        res2 = RS.rho_stream_reference(ohp, ov, Wx, Wy, fine, clip, noise, dtype)
        assert all(np.array_equal(a, b) for a, b in zip((out, pred, rhos, pur, carry[0], carry[1]), res2[:4] + res2[4][:2]))
        # ... and resuming from a carry continues the same run
        o1, p1, r1, u1, c1 = RS.rho_stream_reference(ohp, ov, Wx, Wy, plan[:2], clip[:, :6], noise[:4], dtype)
        o2, p2, r2, u2, c2 = RS.rho_stream_reference(ohp, ov, Wx, Wy, plan[2:], clip[:, 5:], noise[4:], dtype, start=c1)
        assert np.array_equal(np.concatenate([o1, o2], 1), out) and np.array_equal(np.concatenate([p1, p2], 1), pred)
        assert np.array_equal(np.concatenate([r1, r2], 1), rhos) and np.array_equal(np.concatenate([u1, u2], 1), pur)
        assert np.array_equal(c2[0], carry[0]) and np.array_equal(c2[1], carry[1]) and c2[2] == carry[2] == 18
        assert np.array_equal(carry[0], rhos[:, -1])
        # one primed run is the plan [(P, length)], bit for bit
        ref = RR.rho_primed_reference(ohp, ov, Wx, Wy, clip[:, :6], noise[:4], dtype)
        got = RS.rho_stream_reference(ohp, ov, Wx, Wy, [(5, 4)], clip[:, :6], noise[:4], dtype)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got[:4], ref))
    # a shared clip is its tiled copy; the path count of a forced-only plan comes from n
    a = RS.rho_stream_reference(ohp, ov, Wx, Wy, [(5, 0)], clip[1, :6], None, n=n)
    b = RS.rho_stream_reference(ohp, ov, Wx, Wy, [(5, 0)], np.tile(clip[1:2, :6], (n, 1)), None)
    assert a[0].shape == (n, 0) and all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize("D,rank,variant,rank1,n,plan", RS.GPU_CASES)
def test_gpu_case_references_are_finite_and_physical(D, rank, variant, rank1, n, plan):
    """The float32 composition of every GPU case: finite, unit trace, purity in [1/D, 1] (what the GPU bars are laid around)."""
    out, pred, rhos, pur = RS.case_reference(D, rank, plan, n, "f32")
    F, L = SR.plan_steps(plan)
    assert out.shape == (n, L) and pred.shape == (n, F) and rhos.shape == (n, F + L, D, D) and pur.shape == (n, F + L)
    assert all(np.all(np.isfinite(x)) for x in (out, pred, rhos, pur))
    assert np.max(np.abs(np.einsum('abcc->ab', rhos) - 1)) <= 1e-4
    assert np.all(pur <= 1 + 1e-4) and np.all(pur >= 1.0 / D - 1e-4)


# ---------------------------------------------------------------------------------------------------
# SampleStream on the stand-in backend: all bit-exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [1, 7, 64])
def test_follow_in_blocks_equals_predict_increments(blk):
    n, T = 3, 100
    m, be = _model(n=n)
    clips = make_audio(n, T, m.hparams.delta_t, 4)
    want = m.predict_increments(clips)
    st = m.open_stream(n, T - 1)
    assert be.prepared[-1] == (n, T, False) and (st.position, st.max_steps, st.last, st.keep_states) == (0, T - 1, None, 0)
    preds = [st.follow(clips[:, a:a + blk]) for a in range(0, T, blk)]
    assert preds[0].shape == (n, blk - 1)                                   # the anchor makes no step
    pred = np.concatenate(preds, axis=1)
    assert pred.dtype == np.float32 and np.array_equal(pred, want)
    assert st.position == T - 1 and np.array_equal(st.last, clips[:, -1])
    with pytest.raises(ValueError):
        st.follow(clips[:, :1])                                             # one step past max_steps
    assert st.position == T - 1
    st1 = m.open_stream(n, T - 1)                                           # one signal shared by every path
    p1 = np.concatenate([st1.follow(clips[1, a:a + blk]) for a in range(0, T, blk)], axis=1)
    assert p1.shape == (n, T - 1) and all(np.array_equal(p1[b], want[1]) for b in range(n))


def test_generate_in_pieces_equals_sample():
    n, length = 3, 130
    m, _ = _model(n=n)
    want = m.sample(n, length, temp=0.5, seed=11) / m.A
    st = m.open_stream(n, length, temp=0.5, seed=11)
    parts = [st.generate(k) for k in (1, 63, 1, 65)]
    assert np.array_equal(np.concatenate(parts, axis=1), want) and parts[0].dtype == np.float32
    assert st.position == length and np.array_equal(st.last, want[:, -1])
    with pytest.raises(ValueError):
        st.generate(1)
    with pytest.raises(ValueError):
        m.open_stream(n, 4).generate(5)


def test_follow_then_generate_equals_continue_clip():
    n, Tp, length = 2, 70, 66
    m, _ = _model(n=n)
    clips = make_audio(n, Tp, m.hparams.delta_t, 6)
    want = m.continue_clip(clips, n, length, temp=0.5, seed=3)
    st = m.open_stream(n, Tp - 1 + length, temp=0.5, seed=3)
    st.follow(clips[:, :40])
    st.follow(clips[:, 40:])
    got = np.concatenate([st.generate(2), st.generate(length - 2)], axis=1)
    assert np.array_equal(got, want)
    one = m.continue_clip(clips[1], n, length, temp=0.5, seed=3)              # a 1-D clip under every path
    st = m.open_stream(n, Tp - 1 + length, temp=0.5, seed=3)
    st.follow(clips[1])
    assert np.array_equal(st.generate(length), one)


def test_fill_gaps():
    n, T = 3, 120
    m, _ = _model(n=n)
    clip = make_audio(1, T, m.hparams.delta_t, 8)[0]
    known = np.ones(T, bool)
    known[50:80] = False
    st = m.open_stream(n, T, temp=0.5, seed=5)
    wave = st.fill_gaps(clip, known)
    assert wave.shape == (n, T) and wave.dtype == np.float32 and np.all(np.isfinite(wave))
    assert np.array_equal(wave[:, known], np.tile(clip[known], (n, 1)))
    assert not np.array_equal(wave[0, 50:80], wave[1, 50:80])
    assert st.position == 49 + 30 + 39 and np.array_equal(st.last, np.full(n, clip[-1], np.float32))
    ref = m.open_stream(n, T, temp=0.5, seed=5)                              # the gap is the continuation of the first run
    ref.follow(clip[:50])
    assert np.array_equal(ref.generate(30), wave[:, 50:80])
    with pytest.raises(ValueError):
        m.open_stream(n, 60).fill_gaps(clip, known)                         # needs 118 steps


def test_keep_states_returns_rho_and_purity_of_the_last_call():
    """A stream opened with keep_states=S prepares tables of max_steps + 1 rows and a train=True rho workspace of S + 1, and returns
    the lab-frame rho / purity of each call's steps: collected call by call they are the one-shot scan's."""
    n, Tp, length, S_ = 2, 41, 50, 25
    m, be = _model(n=n)
    D = m.bond_d
    clips = make_audio(n, Tp, m.hparams.delta_t, 6)
    noise = O.sample_noise(O.HParams(**m.hparams.values()), n, length, temp=0.5, seed=1)
    rhos_want = m.rho_evolve_with_sampling(n, length, noise=noise, prime=clips)
    pur_want = m.purity(n, length, noise=noise, prime=clips)
    st = m.open_stream(n, Tp - 1 + length, keep_states=S_)
    assert be.prepared[-1] == (n, S_ + 1, True) and be.T == Tp + length and st.keep_states == S_
    rhos, purs = [], []
    with pytest.raises(ValueError):
        st.states()                                                         # no call has made a step yet
    for a, b in ((0, 21), (21, 41)):
        st.follow(clips[:, a:b])
        rhos.append(st.states())
        purs.append(st.purity())
    assert rhos[0].shape == (n, 20, D, D) and purs[1].shape == (n, 20)
    for a in (0, 25):
        st.generate(25, noise=noise[a:a + 25])
        purs.append(st.purity())
        rhos.append(st.states())
    assert np.array_equal(np.concatenate(rhos, axis=1), rhos_want) and rhos[0].dtype == np.complex64
    assert np.array_equal(np.concatenate(purs, axis=1), pur_want) and purs[0].dtype == np.float32


def test_keep_states_value_errors():
    n = 2
    m, be = _model(n=n)
    clip = make_audio(1, 40, m.hparams.delta_t, 3)[0]
    st = m.open_stream(n, 100, keep_states=10)
    launches = be.launches
    with pytest.raises(ValueError):
        st.generate(11)                                                     # longer than keep_states: refused before any launch
    with pytest.raises(ValueError):
        st.follow(clip[:12])                                                # 11 steps
    assert st.position == 0 and be.launches == launches
    st.follow(clip[:11])                                                    # 10 steps fit
    assert st.position == 10 and st.purity().shape == (n, 10)
    plain = m.open_stream(n, 100)
    plain.generate(3)
    for f in (plain.states, plain.purity):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):
        m.open_stream(n, 100, keep_states=-1)
    with pytest.raises(TypeError):
        _psi_model()[0].open_stream(n, 100, keep_states=4)                  # PsiCMPS has no states to keep


# ---------------------------------------------------------------------------------------------------
# PsiCMPS through the moved open_stream
# ---------------------------------------------------------------------------------------------------
def test_psi_stream_still_works_through_the_shared_open_stream():
    import _primed_ref as PR
    assert PsiCMPS.open_stream is not RhoCMPS.open_stream and "open_stream" not in vars(PsiCMPS)
    n, Tp, length = 3, 30, 20
    m, be = _psi_model(n=n)
    clips = make_audio(n, Tp, m.hparams.delta_t, 6)
    noise = O.sample_noise(O.HParams(**m.hparams.values()), n, length, temp=0.5, seed=2)
    st = m.open_stream(n, Tp - 1 + length)
    assert be.prepared[-1] == (n, Tp + length, False)
    pred = np.concatenate([st.follow(clips[:, :11]), st.follow(clips[:, 11:])], axis=1)
    out = np.concatenate([st.generate(7, noise=noise[:7]), st.generate(13, noise=noise[7:])], axis=1)
    hp, var = be._oracle_model(n)
    ref_out, ref_pred, _ = SR.stream_reference(hp, var, [(Tp - 1, length)], clips, noise)
    assert np.array_equal(pred, ref_pred.astype(np.float32))
    assert np.array_equal(out, (clips[:, -1:] + ref_out.astype(np.float32) / m.A).astype(np.float32))
    for f in (st.states, st.purity):
        with pytest.raises(ValueError):
            f()


# ---------------------------------------------------------------------------------------------------
# python -m audio_mps_amd.sample --segment on a rho_mps checkpoint
# ---------------------------------------------------------------------------------------------------
def test_sample_main_segment_on_a_rho_checkpoint_equals_one_shot(tmp_path):
    from audio_mps_amd.train import Trainer
    D, rank, n, dur, Tp = 4, 3, 2, 90, 70
    hp = HParams(minibatch_size=4, bond_dim=D, initial_rank=rank)
    m = RhoCMPS(hp, data_iterator=make_audio(4, 32, hp.delta_t, 1), seed=0, backend=OracleBackend(D))
    tr = Trainer(m, hp)
    tr.step()
    ckdir = os.path.join(tmp_path, "run")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    common = ["--sample_duration", str(dur), "--num_samples", str(n), "--seed", "7", "--temp", "0.5", "--modeldir", ckdir]
    clip = 0.5 * O.damped_sine(1, Tp, hp.delta_t, seed=3)[0]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, clip, 16000)
    for extra in ([], ["--prime", wav]):
        o1, o2 = os.path.join(tmp_path, "a"), os.path.join(tmp_path, "b" + str(len(extra)))
        want = S.main(common + extra + ["--out_dir", o1], backend=RhoStreamBackend(D))
        be = RhoStreamBackend(D)
        got = S.main(common + extra + ["--out_dir", o2, "--segment", "40"], backend=be)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert be.prepared[-1] == (n, (Tp - 1 if extra else 0) + dur + 1, False) and be.phi.shape == (rank, D)
        assert be.launches == (2 if extra else 0) + 3
        assert sorted(os.listdir(o2)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
        assert np.array_equal(np.load(os.path.join(o2, "samples.npy")), want)
    with pytest.raises(ValueError):
        S.main(common + ["--out_dir", o1, "--segment", "0"], backend=RhoStreamBackend(D))
