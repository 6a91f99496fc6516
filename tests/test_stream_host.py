"""Host layer of the resumable sampler without a GPU: the two C symbols, PsiCMPS.open_stream / SampleStream (follow, generate, fill_gaps)
and `python -m audio_mps_amd.sample --segment`, on a stand-in backend that answers `stream_state` / `stream` from the oracle composition
(tests/_stream_ref.py), carrying (psi, running sum).  The kernels themselves are tested in tests/test_gpu_stream.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import make_audio
import _primed_ref as PR
import _stream_ref as SR
from test_primed_host import PrimedBackend

from audio_mps_amd import HParams, PsiCMPS, _capi
from audio_mps_amd import sample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StreamBackend(PrimedBackend):
    """PrimedBackend plus HipScan's two stream entries; a state is a dict holding the oracle's carry, with cmps_psi_stream's checks."""

    def stream_state(self, n):
        return {"n": n, "carry": None}

    def stream(self, state_in, state_out, k0, audio, noise, want_pred=False, n=None):
        assert (state_in is None) == (k0 == 0)
        forced = 0 if audio is None else np.shape(audio)[1] - 1
        length = 0 if noise is None else np.shape(noise)[0]
        assert forced + length >= 1 and k0 + forced + length <= self.T - 1, "cmps_psi_stream: T of set_params too small"
        n = n if noise is None else np.shape(noise)[1]
        hp, var = self._oracle_model(n)
        start = None
        if state_in is not None:
            start = state_in["carry"]
            assert start[2] == k0 and state_in["n"] == n
        out, pred, carry = SR.stream_reference(hp, var, [(forced, length)], audio if forced else np.zeros((n, 1), np.float32),
                                               noise if length else None, self.dtype, start=start, n=n)
        if state_out is not None:
            state_out["carry"] = carry
        return out.astype(np.float32), (pred.astype(np.float32) if want_pred else None)


def _model(D=5, n=3):
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    be = StreamBackend(D)
    m = PsiCMPS(hp, seed=2, backend=be)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
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
    for name in ("cmps_psi_stream_state_bytes", "cmps_psi_stream"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
        assert re.search(r"^\w[\w \*]*\b%s\(" % name, header, flags=re.M), name
    assert lib.cmps_version() == 500


def test_state_bytes_and_call_order_without_a_device():
    lib = _cdll()
    assert lib.cmps_psi_stream_state_bytes(None, 1) == 0
    assert lib.cmps_psi_stream(None, None, None, 0, None, 1, 0, None, 1, 1, None, None, None) == _capi.CMPS_ERR_BAD_ARG
    for D in (8, 32, 48, 128):
        h = ctypes.c_void_p()
        assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
        try:
            one = lib.cmps_psi_stream_state_bytes(h, 1)
            assert one > 0 and one % 16 == 0
            assert lib.cmps_psi_stream_state_bytes(h, 0) == 0 and lib.cmps_psi_stream_state_bytes(h, -3) == 0
            assert [lib.cmps_psi_stream_state_bytes(h, n) for n in (2, 3, 1000)] == [2 * one, 3 * one, 1000 * one]
            # the record holds the state vector at least, and belongs to the sampler family: the block kernel's differs from the wave's
            assert one >= 2 * D * 4
            assert lib.cmps_set_variant(h, 1) == _capi.CMPS_OK
            blk = lib.cmps_psi_stream_state_bytes(h, 1)
            assert blk > 0 and blk % 16 == 0 and blk >= (2 * D + 1) * 4
            assert lib.cmps_set_variant(h, 0) == _capi.CMPS_OK
            # a fresh handle: CMPS_ERR_STATE before any pointer is looked at
            assert lib.cmps_psi_stream(h, None, None, 0, None, 1, 0, None, 1, 1, None, None, None) == _capi.CMPS_ERR_STATE
            assert b"cmps_set_params" in lib.cmps_last_error(h)
        finally:
            lib.cmps_destroy(h)


# ---------------------------------------------------------------------------------------------------
# the oracle composition
# ---------------------------------------------------------------------------------------------------
def test_reference_does_not_depend_on_the_segmentation():
    D, n = 5, 2
    hp, var = PR.case_hparams(D, n), PR.case_variables(D, n)
    plan = ((5, 0), (0, 4), (3, 6))
    clip, noise = SR.case_inputs(D, plan, n)
    for dtype in ("f32", "f64"):
        out, pred, carry = SR.stream_reference(hp, var, plan, clip, noise, dtype)
        fine = SR.refine(plan)
        assert fine != list(plan) and len(fine) > len(plan)
        out2, pred2, carry2 = SR.stream_reference(hp, var, fine, clip, noise, dtype)
        assert np.array_equal(out, out2) and np.array_equal(pred, pred2) and np.array_equal(carry[0], carry2[0])
        # ... and resuming from a carry continues the same run
        o1, p1, c1 = SR.stream_reference(hp, var, plan[:2], clip[:, :6], noise[:4], dtype)
        o2, p2, c2 = SR.stream_reference(hp, var, plan[2:], clip[:, 5:], noise[4:], dtype, start=c1)
        assert np.array_equal(np.concatenate([o1, o2], 1), out) and np.array_equal(np.concatenate([p1, p2], 1), pred)
        assert np.array_equal(c2[0], carry[0]) and np.array_equal(c2[1], carry[1]) and c2[2] == carry[2] == 18
    # one primed run is the plan [(P, length)]
    ref_out, ref_pred = PR.primed_reference(hp, var, clip[:, :6], noise[:4])
    o, p, _ = SR.stream_reference(hp, var, [(5, 4)], clip[:, :6], noise[:4])
    assert np.array_equal(o, ref_out) and np.array_equal(p, ref_pred)
    assert SR.refine([(1, 0), (0, 1), (4, 3)]) == [(1, 0), (0, 1), (2, 0), (2, 0), (0, 1), (0, 2)]


# ---------------------------------------------------------------------------------------------------
# SampleStream on the stand-in backend: all bit-exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [1, 7, 64])
def test_follow_in_blocks_equals_predict_increments(blk):
    n, T = 3, 150
    m, be = _model(n=n)
    clips = make_audio(n, T, m.hparams.delta_t, 4)
    want = m.predict_increments(clips)
    st = m.open_stream(n, T - 1)
    assert be.prepared[-1] == (n, T, False) and (st.position, st.max_steps, st.last) == (0, T - 1, None)
    preds = [st.follow(clips[:, a:a + blk]) for a in range(0, T, blk)]
    assert preds[0].shape == (n, blk - 1)                                   # the anchor makes no step
    pred = np.concatenate(preds, axis=1)
    assert pred.dtype == np.float32 and np.array_equal(pred, want)
    assert st.position == T - 1 and np.array_equal(st.last, clips[:, -1])
    with pytest.raises(ValueError):
        st.follow(clips[:, :1])                                             # one step past max_steps
    assert st.position == T - 1
    # one signal shared by every path
    st1 = m.open_stream(n, T - 1)
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
    # noise handed in, as model.sample takes it
    noise = O.sample_noise(O.HParams(**m.hparams.values()), n, length, temp=0.5, seed=1)
    st = m.open_stream(n, length)
    got = np.concatenate([st.generate(100, noise=noise[:100]), st.generate(30, noise=noise[100:])], axis=1)
    assert np.array_equal(got, m.sample(n, length, noise=noise) / m.A)


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
    for bad in (clips[:, :0], clips[None], np.zeros((n + 1, 4), np.float32)):
        with pytest.raises(ValueError):
            st.follow(bad)


def test_fill_gaps():
    n, T = 3, 120
    m, _ = _model(n=n)
    clip = make_audio(1, T, m.hparams.delta_t, 8)[0]
    assert np.array_equal(m.open_stream(n, T).fill_gaps(clip, np.ones(T, bool)), np.tile(clip, (n, 1)))
    known = np.ones(T, bool)
    known[50:80] = False
    st = m.open_stream(n, T, temp=0.5, seed=5)
    wave = st.fill_gaps(clip, known)
    assert wave.shape == (n, T) and wave.dtype == np.float32 and np.all(np.isfinite(wave))
    assert np.array_equal(wave[:, known], np.tile(clip[known], (n, 1)))
    assert not np.array_equal(wave[0, 50:80], wave[1, 50:80])
    # 49 followed steps, 30 generated, the run behind the gap re-anchored: 39 steps from its first sample
    assert st.position == 49 + 30 + 39 and np.array_equal(st.last, np.full(n, clip[-1], np.float32))
    # the gap is the continuation of the first run, from its last sample
    ref = m.open_stream(n, T, temp=0.5, seed=5)
    ref.follow(clip[:50])
    assert np.array_equal(ref.generate(30), wave[:, 50:80])
    per_path = make_audio(n, T, m.hparams.delta_t, 9)
    w2 = m.open_stream(n, T, seed=1).fill_gaps(per_path, known)
    assert np.array_equal(w2[:, known], per_path[:, known])
    with pytest.raises(ValueError):
        m.open_stream(n, T).fill_gaps(clip, known[:-1])
    with pytest.raises(ValueError):
        m.open_stream(n, 60).fill_gaps(clip, known)                         # needs 118 steps


def test_sample_main_segment_equals_one_shot(tmp_path):
    from audio_mps_amd.train import Trainer
    from _util import OracleBackend
    D, n, dur, Tp = 4, 2, 120, 130
    hp = HParams(minibatch_size=4, bond_dim=D)
    m = PsiCMPS(hp, data_iterator=make_audio(4, 32, hp.delta_t, 1), seed=0, backend=OracleBackend(D))
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
        want = S.main(common + extra + ["--out_dir", o1], backend=StreamBackend(D))
        be = StreamBackend(D)
        got = S.main(common + extra + ["--out_dir", o2, "--segment", "50"], backend=be)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert be.prepared[-1] == (n, (Tp - 1 if extra else 0) + dur + 1, False)
        assert sorted(os.listdir(o2)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
        assert np.array_equal(np.load(os.path.join(o2, "samples.npy")), want)
    with pytest.raises(ValueError):
        S.main(common + ["--out_dir", o1, "--segment", "0"], backend=StreamBackend(D))
