"""The host side of the device-resident training input (audio_mps_amd/device_data.py, --device_data) without a GPU: a stand-in backend
whose `gather_batch` and `damped_sine` ARE the numpy reference (tests/_data_ref.py) and record their calls.  Index plans against
tfrecord.audio_batches bit for bit, shards, crops, the definition's delays, and the flag on a backend that cannot serve it.  The kernels
are tied to the same reference in tests/test_gpu_device_data.py."""
import os

import numpy as np
import pytest
import torch

import _data_ref as DR
from _util import OracleBackend, make_audio


class DataBackend(OracleBackend):
    """`gather_batch` / `damped_sine` from the reference on host tensors, recording what they were asked for."""

    def __init__(self, D=4):
        super().__init__(D)
        self.gathers, self.fills, self.seen = [], [], []

    def gather_batch(self, data, index, offset=None, T=None):
        assert data.dtype == torch.float32 and index.dtype == torch.int32 and (offset is None or offset.dtype == torch.int32)
        T = data.shape[1] if T is None else T
        idx, off = index.numpy().copy(), None if offset is None else offset.numpy().copy()
        self.gathers.append((idx, off, T))
        return torch.from_numpy(DR.gather(data.numpy(), idx, off, T))

    def damped_sine(self, seed, first_clip, B, T, delta_t):
        self.fills.append((seed, first_clip, B, T, delta_t))
        return torch.from_numpy(DR.damped_sine(seed, first_clip, B, T, delta_t, np.float32))

    def loss_and_grad_sums(self, audio, check=False):
        self.seen.append(np.asarray(audio).copy())
        return super().loss_and_grad_sums(audio)


N, L, MB = 10, 16, 4


@pytest.fixture(scope="module")
def record_file(tmp_path_factory):
    from audio_mps_amd import tfrecord as tfr
    clips = make_audio(N, L, 1 / 16000, 3)
    clips.setflags(write=False)
    path = os.path.join(tmp_path_factory.mktemp("data"), "organ.tfrecords")
    tfr.write_audio_tfrecord(path, clips)
    return path, clips


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("order", ["data", "estimator"])
@pytest.mark.parametrize("shuffle_buffer", [24, 2])
def test_plans_equal_the_host_pipeline(record_file, shuffle_buffer, order, seed):
    """The first 9 batches (three epochs of "data": 4, 4, 2 clips each) equal tfrecord.audio_batches' bit for bit, shapes included; the
    file is read once, and a step uploads nothing: one plan tensor per epoch, sliced."""
    from audio_mps_amd import tfrecord as tfr
    from audio_mps_amd.device_data import ResidentDataset
    path, clips = record_file
    be = DataBackend()
    ds = ResidentDataset.from_tfrecord(path, L, be)
    assert ds.n_clips == N and ds.clip_len == L and np.array_equal(ds.clips.numpy(), clips)
    want = tfr.audio_batches(path, MB, L, seed=seed, shuffle_buffer=shuffle_buffer, order=order)
    got = ds.batches(MB, seed=seed, order=order, shuffle_buffer=shuffle_buffer)
    sizes = []
    for k in range(9):
        w, n = want(), got.next_size
        g = got()
        assert isinstance(g, torch.Tensor) and g.dtype == torch.float32
        assert g.shape == w.shape == (n, L) and np.array_equal(g.numpy().view(np.uint32), w.view(np.uint32)), (k, order)
        sizes.append(n)
    assert sizes == [4] * 9 if order == "estimator" else all(sorted(sizes[3 * e:3 * e + 3]) == [2, 4, 4] for e in range(3)), sizes
    assert all(off is None and T == L for _, off, T in be.gathers) and len(be.gathers) == 9
    if order == "data":                                         # every epoch is a permutation of the batches 0-3, 4-7, 8-9
        for e in range(3):
            rows = sorted(tuple(idx) for idx, _, _ in be.gathers[3 * e:3 * e + 3])
            assert rows == [(0, 1, 2, 3), (4, 5, 6, 7), (8, 9)]
    else:                                                       # ... of the clips, batches crossing the epoch boundaries
        flat = np.concatenate([idx for idx, _, _ in be.gathers])
        assert all(sorted(flat[N * e:N * e + N]) == list(range(N)) for e in range(3))


def test_shards_tile_every_batch():
    """For every (start, count) the sharded batch equals the slice of the whole one -- over a run of batches that includes the short ones,
    the streams staying in step (a shard consumes the whole batch's plan)."""
    from audio_mps_amd.device_data import ResidentDataset
    clips = make_audio(N, L, 1 / 16000, 4)
    for order in ("data", "estimator"):
        for start, count in [(0, 4), (0, 2), (2, 2), (1, 3), (3, 1), (0, 0), (4, 0), (1, 1), (3, 5), (5, 2)]:
            be = DataBackend()
            whole = ResidentDataset(clips, DataBackend()).batches(MB, seed=3, order=order)
            part = ResidentDataset(clips, be).batches(MB, seed=3, order=order)
            for k in range(7):
                assert part.next_size == whole.next_size
                full, got = whole().numpy(), part(shard=(start, count))
                assert got.shape[1] == L and np.array_equal(got.numpy(), full[start:start + count]), (order, start, count, k)
            assert all(len(idx) <= max(count, 0) for idx, _, _ in be.gathers)       # only the shard's rows are gathered


def test_crops_stay_inside_the_clip_and_leave_the_order_alone():
    from audio_mps_amd.device_data import ResidentDataset
    clips = make_audio(N, L, 1 / 16000, 5)
    T = 5
    for order in ("data", "estimator"):
        plain_be, crop_be, crop2_be = DataBackend(), DataBackend(), DataBackend()
        plain = ResidentDataset(clips, plain_be).batches(MB, seed=1, order=order)
        crop = ResidentDataset(clips, crop_be).batches(MB, seed=1, order=order, crop=T, crop_seed=9)
        crop2 = ResidentDataset(clips, crop2_be).batches(MB, seed=1, order=order, crop=T, crop_seed=10)
        for _ in range(40):
            p, c = plain().numpy(), crop().numpy()
            crop2()
            assert c.shape == (p.shape[0], T)
            idx, off, t = crop_be.gathers[-1]
            assert t == T and off is not None and off.min() >= 0 and off.max() <= L - T
            assert np.array_equal(idx, plain_be.gathers[-1][0])                      # the order stream is undisturbed
            assert all(np.array_equal(c[b], p[b, off[b]:off[b] + T]) for b in range(len(idx)))
        offs = np.concatenate([g[1] for g in crop_be.gathers])
        assert set(offs.tolist()) == set(range(L - T + 1))                           # every start occurs, both ends included
        assert not np.array_equal(offs, np.concatenate([g[1] for g in crop2_be.gathers]))
    # crop = L is no crop; a crop beyond the clip is refused
    be = DataBackend()
    ResidentDataset(clips, be).batches(MB, crop=L)()
    assert be.gathers[-1][1] is None
    for bad in (0, L + 1, -3):
        with pytest.raises(ValueError, match="crop"):
            ResidentDataset(clips, be).batches(MB, crop=bad)


def test_the_definitions_delays_are_gamma_2():
    """Gamma(2, theta) with theta = T / 200: mean 2 theta = T / 100, variance 2 theta^2, so the standard error of the mean of 4096 draws is
    theta sqrt(2) / 64; the mean lies within 5 of them, for several seeds and a range of clips across the 32-bit counter word."""
    T, n = 16000, 4096
    theta = T / 200.0
    se = theta * np.sqrt(2.0) / 64.0
    for seed, first in [(0, 0), (1, 0), (2 ** 64 - 1, 5), (20261019, 2 ** 32 - 2048)]:
        d = DR.delays(seed, first, n, T, np.float64)
        assert d.shape == (n,) and d.min() > 0.0 and d.max() <= theta * 2 * 24 * np.log(2.0) * (1 + 1e-12)
        assert abs(d.mean() - T / 100.0) <= 5.0 * se, (seed, first, d.mean())
        assert abs(d.var() - 2.0 * theta ** 2) <= 0.25 * 2.0 * theta ** 2           # (a Gamma(1) or Gamma(3) would miss by a factor)
        d32 = DR.delays(seed, first, n, T, np.float32)
        assert d32.dtype == np.float32 and np.max(np.abs(d32 - d)) <= 4e-6 * d.max()
    # a clip is a function of its own number: any window of the sequence holds the same delays
    assert np.array_equal(DR.delays(3, 100, 50, T), DR.delays(3, 0, 4096, T)[100:150])
    assert not np.array_equal(DR.delays(3, 0, 50, T), DR.delays(4, 0, 50, T))


def test_the_reference_waveform_is_the_host_generators_formula():
    """tests/_data_ref.damped_sine in float32 against audio_mps_amd.data.damped_sine's expression for the same delays: the same bits (the
    two differ in where the delays come from, not in the waveform)."""
    T, dt = 300, 1.0 / 16000
    d = DR.delays(5, 0, 3, T, np.float32)
    times = (np.arange(T, dtype=np.float32)[None, :] - d[:, None]) * np.float32(dt)
    want = (np.float32(0.5) * (np.sign(times) + np.float32(1)) * np.sin(np.float32(2 * np.pi * 261.6) * times)
            * np.exp(-times / np.float32(0.1))).astype(np.float32)
    got = DR.damped_sine(5, 0, 3, T, dt, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.all(np.isfinite(got)) and np.any(got != 0)
    assert np.all(got[np.arange(T)[None, :] < d[:, None]] == 0)                       # silent before the onset


def test_damped_sine_source_follows_the_step_and_the_shard():
    from audio_mps_amd.device_data import DampedSineSource
    be = DataBackend()
    src = DampedSineSource(be, 6, 40, 1e-3, seed=11)
    whole = src.next(3).numpy()
    assert whole.shape == (6, 40) and be.fills[-1] == (11, 18, 6, 40, 1e-3)
    for start, count in [(0, 6), (2, 3), (5, 1), (0, 1)]:
        assert np.array_equal(src.next(3, shard=(start, count)).numpy(), whole[start:start + count])
        assert be.fills[-1] == (11, 18 + start, count, 40, 1e-3)
    calls = len(be.fills)
    assert src.next(3, shard=(4, 0)).shape == (0, 40) and len(be.fills) == calls      # an empty shard generates nothing
    assert not np.array_equal(src.next(4).numpy(), whole)


# ---------------------------------------------------------------------------------------------------
# the flag
# ---------------------------------------------------------------------------------------------------
def _argv(tmp, dataset, T, steps, extra=()):
    return ["--dataset", dataset, "--datadir", str(tmp), "--sample_duration", str(T), "--max_steps", str(steps),
            "--hparams", "bond_dim=4,minibatch_size=4", "--logdir", os.path.join(tmp, "log")] + list(extra)


def test_device_data_on_a_backend_without_the_methods_is_a_value_error(tmp_path, record_file):
    from audio_mps_amd import tfrecord as tfr
    from audio_mps_amd import train
    from audio_mps_amd.device_data import DampedSineSource, ResidentDataset
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "organ.tfrecords"), record_file[1])
    for dataset, method in (("damped_sine", "damped_sine"), ("organ", "gather_batch")):
        with pytest.raises(ValueError, match="--device_data") as e:
            train.main(_argv(tmp_path, dataset, L, 2, ["--device_data"]), backend=OracleBackend(4))
        assert method in str(e.value) and "OracleBackend" in str(e.value)
    with pytest.raises(ValueError, match="gather_batch"):
        ResidentDataset(record_file[1], OracleBackend(4))
    with pytest.raises(ValueError, match="damped_sine"):
        DampedSineSource(OracleBackend(4), 4, L, 1e-3)
    # --crop_duration is accepted only together with --device_data, and for a dataset that has clips to cut
    with pytest.raises(ValueError, match="--crop_duration"):
        train.main(_argv(tmp_path, "organ", L, 2, ["--crop_duration", "8"]), backend=DataBackend())
    with pytest.raises(ValueError, match="--crop_duration"):
        train.main(_argv(tmp_path, "damped_sine", L, 2, ["--crop_duration", "8", "--device_data"]), backend=DataBackend())


def test_train_main_with_device_data_sees_the_batches_of_the_host_pipeline(tmp_path, record_file):
    """train.main over two epoch boundaries (batches of 4, 4, 2 clips), with and without --device_data on the same stand-in scan: the scan
    is handed the same batches bit for bit and the checkpoints hold the same variables; with --crop_duration every batch is 8 samples long;
    damped_sine draws the clips of the step it is at."""
    from audio_mps_amd import tfrecord as tfr
    from audio_mps_amd import train
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "organ.tfrecords"), record_file[1])
    runs = {}
    for name, extra in (("host", []), ("dev", ["--device_data"])):
        be = DataBackend()
        argv = _argv(tmp_path, "organ", L, 7, extra)
        argv[argv.index("--logdir") + 1] = os.path.join(tmp_path, name)
        runs[name] = (train.main(argv, backend=be), be)
    (t_host, b_host), (t_dev, b_dev) = runs["host"], runs["dev"]
    assert len(b_host.gathers) == 0 and len(b_dev.gathers) == 7
    assert [s.shape for s in b_dev.seen] == [s.shape for s in b_host.seen] and sorted(s.shape[0] for s in b_host.seen[:3]) == [2, 4, 4]
    assert all(np.array_equal(a, b) for a, b in zip(b_dev.seen, b_host.seen))
    assert [h["global_batch"] for h in t_dev.history] == [h["global_batch"] for h in t_host.history]
    for k in t_host.model.variables:
        assert np.array_equal(t_dev.model.variables[k], t_host.model.variables[k]), k
    be = DataBackend()
    train.main(_argv(tmp_path, "organ", L, 3, ["--device_data", "--crop_duration", "8", "--logdir", os.path.join(tmp_path, "crop")]), backend=be)
    assert all(s.shape[1] == 8 for s in be.seen) and all(T == 8 for _, _, T in be.gathers)
    be = DataBackend()
    tr = train.main(_argv(tmp_path, "damped_sine", 24, 3, ["--device_data", "--seed", "5", "--logdir", os.path.join(tmp_path, "sine")]), backend=be)
    assert [f[:4] for f in be.fills] == [(5, 0, 4, 24), (5, 4, 4, 24), (5, 8, 4, 24)] and tr.global_step == 3
    assert all(np.isfinite(h["model_loss"]) for h in tr.history)


def test_estimator_with_device_data_sees_the_batches_of_the_host_pipeline(record_file):
    """training_estimators' loop fed by build_device_input_fns (shuffle -> repeat -> batch on indices; the callable is handed the rank's
    shard) against the same loop fed by build_input_fns: the scan sees the same batches bit for bit, the variables end up the same.  Without
    a dataset the synthetic clips continue from the step the run is at."""
    from audio_mps_amd import training_estimators as TE
    path, _ = record_file
    params = {"bond_d": 4, "dt": 1.0 / 16000, "batch_size": MB, "discr": False}
    runs = []
    for device in (False, True):
        be = DataBackend()
        est = TE.Estimator(params, model_kw={"seed": 0, "backend": be})
        fn = TE.build_device_input_fns(be, path, MB, L, params["dt"], seed=5) if device else TE.build_input_fns(path, MB, L, seed=5)
        assert getattr(fn, "takes_shard", False) == device
        est.train(fn, steps=6)                                  # 24 clips: across two epoch boundaries of the 10-clip file
        runs.append((est, be))
    (e_host, b_host), (e_dev, b_dev) = runs
    assert len(b_dev.gathers) == 6 and len(b_host.gathers) == 0 and len(b_host.seen) == len(b_dev.seen) == 6
    assert all(a.shape == (MB, L) and np.array_equal(a, b) for a, b in zip(b_dev.seen, b_host.seen))
    assert e_dev.global_step == 6 and e_dev.last_loss == e_host.last_loss
    for k in e_host.model.variables:
        assert np.array_equal(e_dev.model.variables[k], e_host.model.variables[k]), k
    be = DataBackend()
    fn = TE.build_device_input_fns(be, "", MB, 24, params["dt"], seed=2, first_step=3)
    TE.Estimator(params, model_kw={"seed": 0, "backend": be}).train(fn, steps=2)
    assert [f[:4] for f in be.fills] == [(2, 3 * MB, MB, 24), (2, 4 * MB, MB, 24)]
