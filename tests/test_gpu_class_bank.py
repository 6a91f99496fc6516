"""A class bank end to end on a real MI355X: D = 4, T = 64, B = 4, three classes of 3, 5 and 9 clips on the 16-bit grid, a PsiBank and a
RhoBank (rank 3).
  (a) ten ClassBatches steps are, member by member and bit for bit, the plain BatchStream of the filtered dataset -- in both storages;
  (b) ten BankTrainer steps fed by them leave every member's variables bit for bit those of a trainer fed the stacked plain batches;
  (c) evaluate_classifier on a 17-clip held-out set (minibatch 8: the last batch is short) is tests/_classify_ref.py applied to the losses
      BankTrainer.evaluate(keep_losses=True) brings back: every count, the matrix and `best` exactly, the two means within the bound
      include/cmps.h states for the sums, divided by their counts (plus one rounding of the division);
  (d) the steps after an evaluation are bit for bit those of a run without it."""
import numpy as np
import pytest
import torch

import _classify_ref as CR

pytestmark = pytest.mark.gpu

D, T, B, RANK = 4, 64, 4, 3
CLASSES = [62, 60, 67]                                                                 # (member order is not label order)
SIZES = {60: 3, 62: 5, 67: 9}
SEED = 11


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pcm(n, length, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64)
    f = rng.uniform(0.02, 0.2, (n, 1))
    x = 0.2 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6, (n, 1))) + 0.01 * rng.standard_normal((n, length))
    return np.round(x * 32768.0).astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15)


def training_set():
    rng = np.random.default_rng(3)
    labels = np.array([c for c, n in SIZES.items() for _ in range(n)], dtype=np.int64)
    return pcm(labels.size, T + 9, 4), labels[rng.permutation(labels.size)]            # clips longer than T: (a) also runs with crops


def held_out():
    rng = np.random.default_rng(5)
    labels = rng.choice(np.array([60, 62, 67, 71], np.int64), 17)                      # 71: a label the bank has no member for
    return pcm(17, T, 6), labels


def make_trainer(kind):
    from audio_mps_amd import HParams
    from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D, delta_t=1.0 / 16000, initial_rank=RANK if kind == "rho" else None)
    bank = (RhoBank if kind == "rho" else PsiBank)(hp, [{"seed": 20 + m} for m in range(3)], backend=HipScan(D), classes=CLASSES,
                                                   label_key="pitch")
    return BankTrainer(bank)


def plain_streams(clips, labels, be, storage, crop):
    from audio_mps_amd.device_data import ResidentDataset
    return [ResidentDataset(clips[labels == c], be, storage=storage).batches(B, seed=SEED + m, order="estimator", crop=crop, crop_seed=SEED + m)
            for m, c in enumerate(CLASSES)]


@pytest.mark.parametrize("storage", ["float32", "int16"])
@pytest.mark.parametrize("crop", [None, T])
def test_class_batches_are_the_plain_streams_of_the_filtered_datasets(storage, crop):
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    clips, labels = training_set()
    ds = ResidentDataset(clips, be, storage=storage, labels=labels)
    assert ds.storage == storage
    stream = ds.class_batches(CLASSES, B, seed=SEED, crop=crop)
    plain = plain_streams(clips, labels, be, storage, crop)
    be.kernel_events(True)
    got = [stream() for _ in range(10)]
    times = be.kernel_times()
    be.kernel_events(False)
    name = "k_batch_gather_i16" if storage == "int16" else "k_batch_gather"
    assert list(times) == [name] and times[name][1] == 10 and stream.uploads == 1      # one launch per step, one upload for all ten
    for step, g in enumerate(got):
        assert tuple(g.shape) == (3, B, clips.shape[1] if crop is None else crop) and g.is_cuda and g.is_contiguous()
        for m in range(3):
            assert np.array_equal(bits(g[m]), bits(plain[m]())), (step, m)
    with pytest.raises(ValueError, match="61"):
        ds.class_batches([60, 61], B)


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_training_evaluation_and_the_steps_after_it(kind):
    from audio_mps_amd.device_data import ResidentDataset
    clips, labels = training_set()
    fed, stacked, judged = make_trainer(kind), make_trainer(kind), make_trainer(kind)
    assert fed.native
    held, held_labels = held_out()

    def class_stream(tr):
        return ResidentDataset(clips, tr.bank.backend, storage="int16", labels=labels).class_batches(CLASSES, B, seed=SEED, crop=T)

    s_fed, s_judged = class_stream(fed), class_stream(judged)
    plain = plain_streams(clips, labels, stacked.bank.backend, "float32", T)
    ds = ResidentDataset(held, judged.bank.backend, storage="int16", labels=held_labels)
    res = None
    for step in range(10):
        fed.step(s_fed(), sync=False)
        stacked.step(torch.stack([p() for p in plain]), sync=False)
        judged.step(s_judged(), sync=False)
        if step == 4:
            res = judged.evaluate_classifier(ds, 8, keep_best=True)                    # (c), in the middle of the run
            per_member = judged.evaluate(ds, 8, keep_losses=True)
    for m in range(3):
        for k, v in stacked.member(m).variables.items():
            assert np.array_equal(bits(fed.member(m).variables[k]), bits(v)), ("(b)", m, k)
            assert np.array_equal(bits(judged.member(m).variables[k]), bits(v)), ("(d)", m, k)
    # (c)
    loss = np.stack([r.losses for r in per_member])
    assert loss.shape == (3, 17) and np.isfinite(loss).all()
    ref = CR.Record(3).add(loss, ds.class_positions(CLASSES), 0)
    want = ref.record()
    assert np.array_equal(res.best, want["best"]) and res.best.dtype == np.int32
    assert np.array_equal(res.confusion, want["confusion"]) and np.array_equal(res.unlabelled_best, want["unlabelled_best"])
    n_lab = int((held_labels != 71).sum())
    assert (res.n_clips, res.n_undecided, res.first_undecided, res.n_labelled, res.n_unlabelled) == (17, 0, -1, n_lab, 17 - n_lab)
    assert (res.n_correct, res.n_xent, res.n_margin) == (want["n_correct"], n_lab, 17) and res.accuracy == want["n_correct"] / n_lab
    bar_x, bar_m = ref.bounds()
    e_x, e_m = abs(res.cross_entropy - want["sum_xent"] / n_lab), abs(res.mean_margin - want["sum_margin"] / 17)
    print(f"{kind}: accuracy {res.accuracy:.3f}  |xent - exact| {e_x:.3e} (bar {bar_x / n_lab:.3e})  |margin - exact| {e_m:.3e} "
          f"(bar {bar_m / 17:.3e})")
    assert e_x <= bar_x / n_lab + 2.0 ** -52 * abs(res.cross_entropy) and e_m <= bar_m / 17 + 2.0 ** -52 * abs(res.mean_margin)
    rows = want["confusion"].sum(axis=1)
    assert np.array_equal(res.recall[rows > 0], (np.diagonal(want["confusion"]) / np.maximum(rows, 1))[rows > 0])
