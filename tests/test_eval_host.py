"""The host side of held-out evaluation (audio_mps_amd/evaluate.py, ResidentDataset.ordered and its storages, Trainer.evaluate, the
--eval_* flags of train.main, Estimator.evaluate) without a GPU: a stand-in backend whose `loss_stats`, `read_stats` and `gather_batch` ARE
the numpy reference (tests/_eval_ref.py) and count their calls.  The kernels are tied to the same reference in tests/test_gpu_loss_stats.py
and tests/test_gpu_gather_i16.py, the whole pass to the float64 oracle in tests/test_gpu_evaluate.py."""
import json
import os

import numpy as np
import pytest
import torch

import _data_ref as DR
import _eval_ref as ER
from _util import OracleBackend, make_audio


class EvalBackend(ER.EvalMethods, OracleBackend):
    def __init__(self, D=4):
        super().__init__(D)
        self._eval_init()
        self.fills, self.forwards = [], 0

    def damped_sine(self, seed, first_clip, B, T, delta_t):
        self.fills.append((seed, first_clip, B, T, delta_t))
        return torch.from_numpy(DR.damped_sine(seed, first_clip, B, T, delta_t, np.float32))

    def forward(self, audio, save_for_bwd=False):
        self.forwards += 1
        return super().forward(audio, save_for_bwd)


N, L, MB = 10, 16, 4


def pcm_clips(n=N, length=L, seed=1):
    """Clips on the 16-bit grid, both ends of the range included."""
    rng = np.random.default_rng(seed)
    i = rng.integers(-32768, 32768, size=(n, length)).astype(np.int16)
    i[0, 0], i[-1, -1] = -32768, 32767
    return i.astype(np.float32) * np.float32(2.0 ** -15), i


def quiet_pcm(n, length):
    """Clips on the grid at a quarter of the range (losses stay finite at any parameters)."""
    return (pcm_clips(n, length)[1] // 4).astype(np.float32) * np.float32(2.0 ** -15)


class NoStatsBackend(OracleBackend):
    """A backend that can gather but cannot reduce."""

    def gather_batch(self, data, index, offset=None, T=None):
        return torch.from_numpy(DR.gather(data.numpy(), index.numpy(), None if offset is None else offset.numpy(), data.shape[1] if T is None else T))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------
# the dataset
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float32", "int16", "auto"])
def test_ordered_visits_every_clip_once_in_order(storage):
    from audio_mps_amd.device_data import ResidentDataset
    clips, i16 = pcm_clips()
    be = EvalBackend()
    ds = ResidentDataset(clips, be, storage=storage)
    assert ds.storage == ("float32" if storage == "float32" else "int16") and ds.nbytes == N * L * (4 if storage == "float32" else 2)
    if ds.storage == "int16":
        assert ds.clips.dtype == torch.int16 and np.array_equal(ds.clips.numpy(), i16)
    got = list(ds.ordered(MB))
    assert [f for f, _ in got] == [0, 4, 8] and [tuple(b.shape) for _, b in got] == [(4, L), (4, L), (2, L)]
    assert np.array_equal(bits(np.concatenate([b.numpy() for _, b in got])), bits(clips))
    assert [list(idx) for idx, _, _, _ in be.gathers] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert all(off is None for _, off, _, _ in be.gathers)
    for T in (1, 5, L):
        cut = list(ds.ordered(3, T))
        assert [f for f, _ in cut] == [0, 3, 6, 9] and np.array_equal(bits(np.concatenate([b.numpy() for _, b in cut])), bits(clips[:, :T]))
    assert [tuple(b.shape) for _, b in ds.ordered(N + 5)] == [(N, L)]                 # one short batch
    for bad in (0, L + 1):
        with pytest.raises(ValueError, match="T must lie"):
            list(ds.ordered(MB, bad))
    with pytest.raises(ValueError, match="minibatch_size"):
        list(ds.ordered(0))
    # batches(...) works on either storage and is the float32 dataset's stream bit for bit, crops included
    a = ResidentDataset(clips, EvalBackend(), storage="float32").batches(MB, seed=3, crop=7, crop_seed=5)
    b = ds.batches(MB, seed=3, crop=7, crop_seed=5)
    for _ in range(7):
        assert np.array_equal(bits(a().numpy()), bits(b().numpy()))


def test_storage_rules():
    """Lossless data goes to int16; a sample off the grid, a 1.0 (i = 32768) and a -0.0 each fall back under "auto" and raise under "int16",
    naming clip and sample; the default holds float32 whatever the data."""
    from audio_mps_amd.device_data import ResidentDataset
    clips, i16 = pcm_clips()
    assert ResidentDataset(clips, EvalBackend()).storage == "float32"
    assert ResidentDataset(clips, EvalBackend(), storage="auto").storage == "int16"
    zero = clips.copy()
    zero[3, 4] = 0.0                                                                   # +0.0 is on the grid
    assert ResidentDataset(zero, EvalBackend(), storage="int16").storage == "int16"
    for value, (c, s) in ((np.float32(2.0 ** -16), (2, 5)), (np.float32(1.0), (7, 0)), (np.float32(-0.0), (9, 15)),
                          (np.float32(0.1), (0, 0)), (np.float32("nan"), (4, 4)), (np.float32(-1.0 - 2.0 ** -15), (5, 1))):
        other = clips.copy()
        other[c, s] = value
        ds = ResidentDataset(other, EvalBackend(), storage="auto")
        assert ds.storage == "float32" and ds.clips.dtype == torch.float32 and np.array_equal(bits(ds.clips.numpy()), bits(other))
        with pytest.raises(ValueError, match=rf"clip {c}, sample {s}\b"):
            ResidentDataset(other, EvalBackend(), storage="int16")
    two = clips.copy()
    two[6, 3], two[2, 9] = 0.3, 0.7                                                    # the FIRST offender is named
    with pytest.raises(ValueError, match=r"clip 2, sample 9\b"):
        ResidentDataset(two, EvalBackend(), storage="int16")
    with pytest.raises(ValueError, match="storage"):
        ResidentDataset(clips, EvalBackend(), storage="int8")
    assert ResidentDataset(i16, EvalBackend(), storage="int16").storage == "int16"     # an int16 array is PCM as it is
    assert np.array_equal(bits(ResidentDataset(i16, EvalBackend()).clips.numpy()), bits(clips))


def test_from_tfrecord_decides_per_chunk(tmp_path, monkeypatch):
    """Three chunks of two clips: all on the grid -> int16; an offender in the LAST chunk -> "auto" converts the two stored chunks back and
    the dataset holds the file's bits, "int16" names the clip by its position in the file."""
    from audio_mps_amd import device_data, tfrecord as tfr
    clips, i16 = pcm_clips(6, L)
    monkeypatch.setattr(device_data, "UPLOAD_CLIPS_BYTES", 2 * 4 * L)
    path = os.path.join(tmp_path, "pcm.tfrecords")
    tfr.write_audio_tfrecord(path, clips)
    for storage, want in (("float32", "float32"), ("auto", "int16"), ("int16", "int16")):
        ds = device_data.ResidentDataset.from_tfrecord(path, L, EvalBackend(), storage=storage)
        assert ds.storage == want and ds.n_clips == 6
        assert np.array_equal(bits(np.concatenate([b.numpy() for _, b in ds.ordered(4)])), bits(clips))
    off = clips.copy()
    off[5, 2] = 0.3
    path2 = os.path.join(tmp_path, "mixed.tfrecords")
    tfr.write_audio_tfrecord(path2, off)
    ds = device_data.ResidentDataset.from_tfrecord(path2, L, EvalBackend(), storage="auto")
    assert ds.storage == "float32" and np.array_equal(bits(ds.clips.numpy()), bits(off))
    with pytest.raises(ValueError, match=r"clip 5, sample 2\b"):
        device_data.ResidentDataset.from_tfrecord(path2, L, EvalBackend(), storage="int16")


# ---------------------------------------------------------------------------------------------------
# evaluate
# ---------------------------------------------------------------------------------------------------
def _psi(be, D=4, B=MB):
    from audio_mps_amd import HParams, PsiCMPS
    return PsiCMPS(HParams(minibatch_size=B, bond_dim=D, delta_t=1.0 / 16000), seed=3, backend=be)


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_evaluate_makes_one_download_and_equals_loss_per_clip(kind):
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.evaluate import evaluate
    clips = (make_audio(N, L, 1.0 / 16000, 5) * 0.2).astype(np.float32)
    be = EvalBackend()
    m = _psi(be) if kind == "psi" else RhoCMPS(HParams(minibatch_size=MB, bond_dim=4, delta_t=1.0 / 16000, initial_rank=2), seed=3, backend=be)
    ds = ResidentDataset(clips, be)
    res = evaluate(m, ds, MB, keep_losses=True)
    assert be.downloads == 1 and be.stats_calls == [(0, 4, True), (4, 4, False), (8, 2, False)]
    want = np.concatenate([m.loss_per_clip(clips[i:i + MB]) for i in range(0, N, MB)])
    assert res.losses.dtype == np.float32 and np.array_equal(bits(res.losses), bits(want))
    w64 = want.astype(np.float64)
    assert res.n_clips == N and res.n_nonfinite == 0 and res.first_nonfinite == -1 and res.T == L
    assert res.mean == pytest.approx(w64.mean(), rel=1e-14) and res.per_sample == pytest.approx(w64.mean() / (L - 1), rel=1e-14)
    assert res.std == pytest.approx(w64.std(ddof=1), rel=1e-9) and res.sem == pytest.approx(w64.std(ddof=1) / np.sqrt(N), rel=1e-9)
    assert (res.min, res.max, res.argmin, res.argmax) == (float(want.min()), float(want.max()), int(want.argmin()), int(want.argmax()))
    # without keep_losses nothing else comes back; T < L scores the first T samples
    be.downloads = 0
    short = evaluate(m, ds, 3, T=9)
    assert short.losses is None and be.downloads == 1 and short.T == 9 and short.n_clips == N
    assert short.mean == pytest.approx(np.concatenate([m.loss_per_clip(clips[i:i + 3, :9]) for i in range(0, N, 3)]).astype(np.float64).mean(),
                                       rel=1e-14)
    with pytest.raises(ValueError, match="T >= 2"):
        evaluate(m, ds, MB, T=1)


def test_a_backend_without_loss_stats_is_a_value_error():
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.evaluate import evaluate
    be = NoStatsBackend(4)
    with pytest.raises(ValueError, match="loss_stats") as e:
        evaluate(_psi(be), ResidentDataset(pcm_clips()[0], be), MB)
    assert "NoStatsBackend" in str(e.value)


def test_eval_result_arithmetic_on_fabricated_losses():
    """Losses that include NaN, +Inf and -Inf through run_pass on the stand-in: every field against numpy float64 on the finite ones."""
    from audio_mps_amd.evaluate import EvalResult, run_pass
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(23) * 10.0 ** rng.integers(-3, 4, 23)).astype(np.float32)
    x[[2, 9, 22]] = [np.nan, np.inf, -np.inf]
    x[5] = x[17] = x[np.isfinite(x)].max() + np.float32(1)                             # a tie for the maximum: the lowest id
    be = EvalBackend()
    batches = [(i, torch.from_numpy(x[i:i + 8].copy())) for i in range(0, 23, 8)]
    res = run_pass(batches, lambda b: b, be, T=101, keep_losses=True)
    assert be.downloads == 1 and np.array_equal(bits(res.losses), bits(x))
    f = x[np.isfinite(x)].astype(np.float64)
    assert res.n_clips == 23 and res.n_nonfinite == 3 and res.first_nonfinite == 2 and res.T == 101
    assert res.mean == pytest.approx(f.mean(), rel=1e-14) and res.per_sample == pytest.approx(f.mean() / 100.0, rel=1e-14)
    assert res.std == pytest.approx(f.std(ddof=1), rel=1e-10) and res.sem == pytest.approx(f.std(ddof=1) / np.sqrt(20.0), rel=1e-10)
    assert res.max == float(x[5]) and res.argmax == 5 and res.min == float(f.min()) and res.argmin == int(np.flatnonzero(x == np.float32(f.min()))[0])
    assert set(res.scalars()) == {"mean", "per_sample", "std", "sem", "n_clips", "n_nonfinite", "first_nonfinite", "min", "max", "argmin",
                                  "argmax", "T"}
    # the edges: equal losses (the variance is clamped at 0), one clip, none finite
    same = EvalResult.from_stats({"sum": 3 * 0.1, "sumsq": 3 * 0.1 * 0.1 - 1e-18, "n_finite": 3, "n_nonfinite": 0, "argmin": 0, "argmax": 0,
                                  "first_nonfinite": -1, "min": 0.1, "max": 0.1}, 11)
    assert same.std == 0.0 and same.sem == 0.0 and same.mean == pytest.approx(0.1)
    one = run_pass([(4, torch.tensor([2.5]))], lambda b: b, EvalBackend(), T=3)
    assert (one.mean, one.per_sample, one.std, one.n_clips, one.argmin, one.argmax) == (2.5, 1.25, 0.0, 1, 4, 4)
    none = run_pass([(0, torch.tensor([np.nan, np.inf]))], lambda b: b, EvalBackend(), T=3)
    assert np.isnan(none.mean) and none.n_nonfinite == 2 and none.n_clips == 2 and none.argmin == -1 and none.min == float("inf")
    with pytest.raises(ValueError, match="no batch"):
        run_pass([], lambda b: b, EvalBackend(), T=3)


# ---------------------------------------------------------------------------------------------------
# the trainer, the estimator, the command line
# ---------------------------------------------------------------------------------------------------
def _argv(tmp, name, steps, extra=()):
    return ["--dataset", "damped_sine", "--datadir", str(tmp), "--sample_duration", "24", "--max_steps", str(steps), "--seed", "5",
            "--hparams", "bond_dim=4,minibatch_size=4", "--logdir", os.path.join(tmp, name)] + list(extra)


def test_train_main_with_eval_every_writes_its_files_and_leaves_training_alone(tmp_path, capsys):
    from audio_mps_amd import train
    be0, be1 = EvalBackend(), EvalBackend()
    plain = train.main(_argv(tmp_path, "plain", 5), backend=be0)
    capsys.readouterr()
    flags = ["--eval_dataset", "damped_sine", "--eval_every", "2", "--eval_clips", "6", "--eval_minibatch", "4"]
    run = train.main(_argv(tmp_path, "eval", 5, flags), backend=be1)
    out = capsys.readouterr().out
    assert [h["model_loss"] for h in run.history] == [h["model_loss"] for h in plain.history] and len(run.history) == 5
    assert [h["total_loss"] for h in run.history] == [h["total_loss"] for h in plain.history]
    for k in plain.model.variables:
        assert np.array_equal(run.model.variables[k], plain.model.variables[k]), k
    logdir = os.path.join(tmp_path, "eval", "damped_sine", "4_6.25e-05_4")
    with open(os.path.join(logdir, "eval.jsonl")) as f:
        recs = [json.loads(line) for line in f]
    assert [r["global_step"] for r in recs] == [2, 4, 5] and all(r["n_clips"] == 6 and r["n_nonfinite"] == 0 and r["T"] == 24 for r in recs)
    lines = [ln for ln in out.splitlines() if ln.startswith("eval ")]
    assert len(lines) == 3 and all(all(k in ln for k in ("step=", "loss=", "per_sample=", "clips=6", "nonfinite=0")) for ln in lines)
    assert be1.fills == [(6, 0, 6, 24, 1.0 / 16000)] and be0.fills == []               # seed + 1, clips [0, 6), generated once
    assert be1.downloads == 3 and be1.stats_calls == [(0, 4, True), (4, 2, False)] * 3
    assert not os.path.exists(os.path.join(tmp_path, "plain", "damped_sine", "4_6.25e-05_4", "eval.jsonl"))
    # model.best.ckpt.npz holds the variables of the best evaluation: re-evaluating it gives that record's mean
    best = min(recs, key=lambda r: r["mean"])
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.evaluate import evaluate
    from audio_mps_amd.sample import build_model, load_variables
    with np.load(os.path.join(logdir, "model.best.ckpt.npz")) as z:
        assert int(z["global_step"]) == best["global_step"]
    m = build_model(load_variables(os.path.join(logdir, "model.best.ckpt.npz")), 16000, backend=EvalBackend())
    held = DR.damped_sine(6, 0, 6, 24, 1.0 / 16000, np.float32)
    assert evaluate(m, ResidentDataset(held, m._get_backend()), 4).mean == best["mean"]


def test_train_main_evaluates_a_tfrecord_file(tmp_path):
    from audio_mps_amd import tfrecord as tfr, train
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "held.tfrecords"), quiet_pcm(5, 24))
    be = EvalBackend()
    tr = train.main(_argv(tmp_path, "rec", 2, ["--eval_dataset", "held", "--eval_storage", "auto"]), backend=be)
    assert tr.global_step == 2 and be.downloads == 1                                   # --eval_every 0: after the last step only
    assert [g[3] for g in be.gathers] == ["torch.int16", "torch.int16"] and be.stats_calls == [(0, 4, True), (4, 1, False)]
    with pytest.raises(FileNotFoundError):
        train.main(_argv(tmp_path, "none", 1, ["--eval_dataset", "absent"]), backend=EvalBackend())


def test_estimator_evaluate():
    from audio_mps_amd import training_estimators as TE
    be = EvalBackend()
    est = TE.Estimator({"bond_d": 4, "dt": 1.0 / 16000, "batch_size": MB, "discr": False}, model_kw={"seed": 0, "backend": be})
    data = (make_audio(3 * MB, L, 1.0 / 16000, 9) * 0.2).astype(np.float32)
    state = {"i": 0}

    def input_fn():
        state["i"] += 1
        return data[(state["i"] - 1) * MB:state["i"] * MB]
    before = {k: v.copy() for k, v in est.model.variables.items()}
    out = est.evaluate(input_fn, steps=3)
    want = np.concatenate([est.model.loss_per_clip(data[i:i + MB]) for i in range(0, 3 * MB, MB)]).astype(np.float64)
    assert set(out) == {"loss", "global_step"} and out["global_step"] == 0 and out["loss"] == pytest.approx(want.mean(), rel=1e-14)
    assert out["loss"] == pytest.approx(np.mean([want[i:i + MB].mean() for i in range(0, 3 * MB, MB)]), rel=1e-14)   # tf.metrics.mean
    assert be.downloads == 1 and be.stats_calls == [(0, MB, True), (MB, MB, False), (2 * MB, MB, False)]
    assert all(np.array_equal(est.model.variables[k], before[k]) for k in before) and est.opt.t == 0
    with pytest.raises(ValueError, match="steps"):
        est.evaluate(input_fn, steps=0)


def test_the_command_line(tmp_path, capsys):
    from audio_mps_amd import evaluate as EV, tfrecord as tfr, train
    p = EV.build_parser()
    a = p.parse_args(["--dataset", "held"])
    assert (a.storage, a.minibatch_size, a.per_clip, a.json, a.kernel_variant, a.hparams) == ("auto", 64, None, False, 0, "")
    a = p.parse_args(["--modeldir", "m", "--datadir", "d", "--dataset", "x", "--sample_duration", "100", "--minibatch_size", "8",
                      "--storage", "int16", "--per_clip", "o.npy", "--hparams", "sigma=2", "--kernel_variant", "2", "--json"])
    assert (a.modeldir, a.datadir, a.dataset, a.sample_duration, a.minibatch_size, a.storage, a.per_clip, a.hparams, a.kernel_variant,
            a.json) == ("m", "d", "x", 100, 8, "int16", "o.npy", "sigma=2", 2, True)
    with pytest.raises(SystemExit):
        p.parse_args(["--dataset", "x", "--storage", "int8"])
    t = train.build_parser().parse_args([])
    assert (t.eval_dataset, t.eval_every, t.eval_clips, t.eval_minibatch) == (None, 0, 256, None)
    # end to end on the stand-in: a checkpoint of either model, one line, one JSON line, the per-clip file
    clips = quiet_pcm(5, 24)
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "held.tfrecords"), clips)
    for model, extra in (("psi_mps", []), ("rho_mps", ["--hparams", "bond_dim=4,minibatch_size=4,initial_rank=2"])):
        tr = train.main(_argv(tmp_path, model, 1, ["--mps_model", model] + extra), backend=EvalBackend())
        logdir = os.path.join(tmp_path, model, "damped_sine", "4_6.25e-05_4")
        capsys.readouterr()
        per_clip = os.path.join(tmp_path, model + ".npy")
        be = EvalBackend()
        res = EV.main(["--modeldir", logdir, "--datadir", str(tmp_path), "--dataset", "held", "--sample_duration", "24",
                       "--minibatch_size", "2", "--per_clip", per_clip, "--json"], backend=be)
        lines = capsys.readouterr().out.strip().splitlines()
        assert len(lines) == 2 and lines[0].startswith("eval held: loss=") and "storage=int16" in lines[0]
        rec = json.loads(lines[1])
        assert rec["n_clips"] == 5 and rec["storage"] == "int16" and rec["mean"] == res.mean and rec["T"] == 24
        want = np.concatenate([tr.model.loss_per_clip(clips[i:i + 2]) for i in range(0, 5, 2)])
        assert np.array_equal(bits(np.load(per_clip)), bits(want)) and be.downloads == 1
    with pytest.raises(FileNotFoundError):
        EV.main(["--modeldir", logdir, "--datadir", str(tmp_path), "--dataset", "absent"], backend=EvalBackend())
