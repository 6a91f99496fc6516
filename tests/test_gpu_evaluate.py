"""Held-out evaluation end to end on a real MI355X (audio_mps_amd/evaluate.py): 21 clips of 16-bit PCM in a TFRecord file the test writes,
minibatch 8 (so the last batch is short), through ResidentDataset.ordered, the model's forward scan and cmps_loss_stats.

  * the per-clip losses equal model.loss_per_clip on the same batches handed over as host arrays, bit for bit and batch by batch;
  * they lie within the project's loss bar of the float64 oracle: |l - l64| <= 1e-5 * max(|l64|, 1) (README; tests/_util.py);
  * the statistics agree with numpy float64 on those losses (the sums to 1e-12: double accumulation of 21 values);
  * int16 storage gives the bits of float32 storage in every field, and feeds a Trainer the same bits;
  * a Trainer evaluated after steps 1 and 3 of 4 ends with the variables and both Adam slots of one never evaluated, bit for bit, with
    the device-resident step and with the host optimiser.
These tests do not exercise clips the scan kernels turn non-finite: that is tested on cmps_loss_stats directly
(tests/test_gpu_loss_stats.py) and on fabricated losses (tests/test_eval_host.py)."""
import os

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import c_oracle_run, make_audio

pytestmark = pytest.mark.gpu

N, MB = 21, 8
LOSS_RTOL = 1e-5
# (kind, D, rank, T)
MODELS = [("psi", 8, None, 256), ("psi", 20, None, 256), ("psi", 40, None, 64), ("rho", 8, 3, 256)]


def _pcm(B, T, seed):
    """Damped sines with a little noise, on the 16-bit grid: x = i / 32768."""
    x = make_audio(B, T, 1.0 / 16000, seed) * 0.5
    return (np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15))


@pytest.fixture(scope="module")
def held_out(tmp_path_factory):
    """{T: (path of the TFRecord file, its clips [21, T])}: written once, shared, never written to."""
    from audio_mps_amd import tfrecord as tfr
    d = tmp_path_factory.mktemp("held_out")
    out = {}
    for T in (256, 64):
        clips = _pcm(N, T, 40 + T)
        clips.setflags(write=False)
        path = os.path.join(d, f"held_{T}.tfrecords")
        tfr.write_audio_tfrecord(path, clips)
        out[T] = (path, clips)
    return out


def _model(kind, D, rank, B=MB, seed=3):
    from audio_mps_amd import HParams, PsiCMPS, RhoCMPS
    hp = HParams(minibatch_size=B, bond_dim=D, delta_t=1.0 / 16000, initial_rank=rank)
    return (RhoCMPS if kind == "rho" else PsiCMPS)(hp, seed=seed)


def _oracle64(kind, m, clips):
    if kind == "psi":
        return c_oracle_run(m, clips, "f64", want_grad=False, nthreads=8)["loss_per_clip"]
    ohp = O.HParams(**m.hparams.values())
    D = m.bond_d
    ov = O.Variables(np.asarray(m.variables["A"], dtype=np.float32), m.variables["Rx"].copy(), m.variables["Ry"].copy(),
                     m.variables["freqs"].copy(), np.zeros(D, np.float32), np.zeros(D, np.float32),
                     scaled_R=float(m._c_r) != 1.0, scaled_freqs=float(m._c_h) != 1.0)
    return O.rho_loss_per_clip(ohp, ov.astype(np.float64), m.variables["Wx"].astype(np.float64), m.variables["Wy"].astype(np.float64),
                               clips, "f64")


@pytest.mark.parametrize("kind,D,rank,T", MODELS)
def test_evaluate_equals_loss_per_clip_the_oracle_and_numpy(held_out, kind, D, rank, T):
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.evaluate import evaluate
    path, clips = held_out[T]
    m = _model(kind, D, rank)
    be = m._get_backend()
    results = {}
    for storage in ("float32", "int16"):
        ds = ResidentDataset.from_tfrecord(path, T, be, storage=storage)
        assert ds.storage == storage and ds.nbytes == N * T * (4 if storage == "float32" else 2)
        results[storage] = evaluate(m, ds, MB, keep_losses=True)
    res = results["float32"]
    want = np.concatenate([m.loss_per_clip(clips[i:i + MB]) for i in range(0, N, MB)])
    assert res.losses.shape == (N,) and res.losses.dtype == np.float32
    assert np.array_equal(res.losses.view(np.uint32), want.view(np.uint32)), np.flatnonzero(res.losses != want)
    l64 = np.asarray(_oracle64(kind, m, clips), dtype=np.float64)
    err = float(np.max(np.abs(res.losses.astype(np.float64) - l64) / np.maximum(np.abs(l64), 1.0)))
    print(f"{kind} D={D} T={T}: max |l - l64| / max(|l64|, 1) = {err:.3e} (bar {LOSS_RTOL:.0e}); mean {res.mean:.6f}")
    assert np.all(np.isfinite(res.losses)) and err <= LOSS_RTOL
    f = res.losses.astype(np.float64)
    assert (res.n_clips, res.n_nonfinite, res.first_nonfinite, res.T) == (N, 0, -1, T)
    assert res.mean == pytest.approx(f.mean(), rel=1e-12, abs=1e-12) and res.per_sample == pytest.approx(f.mean() / (T - 1), rel=1e-12, abs=1e-12)
    assert res.std == pytest.approx(f.std(ddof=1), rel=1e-6) and res.sem == pytest.approx(f.std(ddof=1) / np.sqrt(N), rel=1e-6)
    assert (res.min, res.max, res.argmin, res.argmax) == (float(f.min()), float(f.max()), int(f.argmin()), int(f.argmax()))
    # int16 storage: the same bits in every field
    r16 = results["int16"]
    assert np.array_equal(r16.losses.view(np.uint32), res.losses.view(np.uint32)) and r16.scalars() == res.scalars()
    # without keep_losses, and T < L: the first samples of every clip
    short = evaluate(m, ResidentDataset(clips, be, storage="auto"), 5, T=33)
    w33 = np.concatenate([m.loss_per_clip(clips[i:i + 5, :33]) for i in range(0, N, 5)]).astype(np.float64)
    assert short.losses is None and short.T == 33 and short.n_clips == N and short.mean == pytest.approx(w33.mean(), rel=1e-12, abs=1e-12)


def _train(kind, rank, device_step, eval_after, held, feed):
    """4 steps at D = 8, T = 256, B = 8 on `feed(step)`; evaluate after the steps in `eval_after`.  Returns (variables, Adam m, Adam v,
    [EvalResult ...])."""
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.train import Trainer
    m = _model(kind, 8, rank, B=8)
    tr = Trainer(m, m.hparams, device_step=device_step)
    ds = ResidentDataset(held, m._get_backend()) if eval_after else None
    evals = []
    for step in range(4):
        tr.step(feed(step, m._get_backend()), sync=False if device_step else True)
        if step + 1 in eval_after:
            evals.append(tr.evaluate(ds, MB))
    tr.sync_to_host()
    return ({k: v.copy() for k, v in m.variables.items()}, {k: v.copy() for k, v in tr.opt.m.items()},
            {k: v.copy() for k, v in tr.opt.v.items()}, evals)


@pytest.mark.parametrize("device_step", [True, False])
@pytest.mark.parametrize("kind,rank", [("psi", None), ("rho", 3)])
def test_trainer_evaluate_leaves_training_untouched(held_out, kind, rank, device_step):
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.evaluate import evaluate
    _, held = held_out[256]
    batches = [_pcm(8, 256, 70 + s) for s in range(4)]
    plain = _train(kind, rank, device_step, (), held, lambda s, be: batches[s])
    run = _train(kind, rank, device_step, (1, 3), held, lambda s, be: batches[s])
    for a, b, what in zip(plain[:3], run[:3], ("variables", "Adam m", "Adam v")):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)
    # the evaluations saw the parameters of their step: different means, each finite, 21 clips
    e1, e3 = run[3]
    assert e1.n_clips == e3.n_clips == N and e1.n_nonfinite == e3.n_nonfinite == 0 and e1.mean != e3.mean
    # ... and the last one's are those of a model holding the variables after step 3: trained 3 steps, evaluated on its own
    m3 = _model(kind, 8, rank, B=8)
    from audio_mps_amd.train import Trainer
    t3 = Trainer(m3, m3.hparams, device_step=device_step)
    for s in range(3):
        t3.step(batches[s])
    t3.sync_to_host()
    alone = evaluate(m3, ResidentDataset(held, m3._get_backend()), MB)
    assert alone.mean == pytest.approx(e3.mean, rel=1e-6)                              # (host and device chain rule differ in rounding)
    if not device_step:
        assert alone.scalars() == e3.scalars()


def test_two_training_steps_from_int16_storage_equal_two_from_float32(held_out):
    from audio_mps_amd.device_data import ResidentDataset
    _, held = held_out[256]
    runs = []
    for storage in ("float32", "int16"):
        streams = {}

        def feed(step, be, storage=storage, streams=streams):
            if "s" not in streams:
                ds = ResidentDataset(held, be, storage=storage)
                assert ds.storage == storage
                streams["s"] = ds.batches(8, seed=2, crop=200, crop_seed=4)
            return streams["s"]()
        from audio_mps_amd.train import Trainer
        m = _model("psi", 8, None, B=8)
        tr = Trainer(m, m.hparams, device_step=True)
        for step in range(2):
            tr.step(feed(step, m._get_backend()), sync=False)
        tr.sync_to_host()
        runs.append(({k: v.copy() for k, v in m.variables.items()}, dict(tr.opt.m), dict(tr.opt.v)))
    for a, b in zip(*runs):
        for k in a:
            assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), k
