"""The host side of class banks without a GPU: the numpy reference of cmps_bank_classify_stats (tests/_classify_ref.py) against hand-worked
cases, labelled TFRecords (tfrecord.labelled_records, the extended make_example), the ClassBatches plan against plain BatchStream plans over
the filtered subsets, bank.json of a class bank, BankTrainer.evaluate_classifier and the command lines -- on the stand-in backends of the
other host tests, whose `classify_stats` IS the reference and counts its calls.  The kernel is tied to the same reference in
tests/test_gpu_classify_stats.py, the whole loop to plain streams and trainers in tests/test_gpu_class_bank.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _classify_ref as CR
import _eval_ref as ER
from _util import OracleBackend

NAN, INF = float("nan"), float("inf")


class Backend(CR.ClassifyMethods, ER.EvalMethods, OracleBackend):
    def __init__(self, D=4):
        super().__init__(D)
        self._eval_init()
        self._classify_init()


class NoClassifyBackend(ER.EvalMethods, OracleBackend):
    def __init__(self, D=4):
        super().__init__(D)
        self._eval_init()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------
# the reference, by hand
# ---------------------------------------------------------------------------------------------------
def test_the_reference_on_hand_worked_clips():
    ln = math.log
    #            clip 0      1 (tie)  2 (NaN member)  3 (nobody)  4 (unlabelled)  5 (own member absent)  6 (one present)
    loss = np.array([[1.0,   2.0,     NAN,            NAN,        5.0,            INF,                   NAN],
                     [3.0,   2.0,     4.0,            -INF,       1.0,            2.0,                   NAN],
                     [2.0,   7.0,     6.0,            INF,        3.0,            2.5,                   0.5]], np.float32)
    labels = [0, 1, 2, 0, 9, 0, 2]
    j = CR.judge(loss, labels)
    assert list(j["best"]) == [0, 0, 1, -1, 1, 1, 2]                                   # clip 1: the lowest member keeps the tie
    want_margin = [1.0, 0.0, 2.0, NAN, 2.0, 0.5, NAN]                                  # clip 6: one present member has no margin
    assert np.array_equal(np.isnan(j["margin"]), np.isnan(want_margin))
    assert np.allclose(j["margin"].astype(float)[[0, 1, 2, 4, 5]], [1.0, 0.0, 2.0, 2.0, 0.5], rtol=0, atol=0)
    want_xent = [ln(1 + math.exp(-2) + math.exp(-1)),                                  # label 0 is the best: log of the sum alone
                 ln(2 + math.exp(-5)),                                                 # label 1 ties for the best
                 2.0 + ln(1 + math.exp(-2)),                                           # label 2 loses by 2; member 0 is absent
                 NAN, NAN, NAN,                                                        # undecided; unlabelled; own member absent
                 0.0]                                                                  # the only present member: p = 1
    got = j["xent"].astype(float)
    assert np.array_equal(np.isnan(got), np.isnan(want_xent))
    ok = ~np.isnan(got)
    assert np.allclose(got[ok], np.array(want_xent)[ok], rtol=1e-15, atol=1e-16)
    rec = CR.Record(3).add(loss, labels, 100).record()
    assert (rec["n_decided"], rec["n_undecided"], rec["n_unlabelled"], rec["n_correct"], rec["n_xent"], rec["n_margin"]) == (6, 1, 1, 2, 4, 5)
    assert rec["first_undecided"] == 103
    assert rec["confusion"].tolist() == [[1, 1, 0], [1, 0, 0], [0, 1, 1]] and rec["unlabelled_best"].tolist() == [0, 1, 0]
    assert rec["sum_margin"] == 5.5 and rec["sum_xent"] == pytest.approx(sum(np.array(want_xent)[ok]), rel=1e-15)
    # continued: a second call adds to the first, a reset forgets it; no labels: every decided clip is unlabelled
    r = CR.Record(3).add(loss, labels, 100).add(loss[:, :2], None, 0)
    two = r.record()
    assert (two["n_decided"], two["n_unlabelled"], two["n_xent"], two["first_undecided"]) == (8, 3, 4, 103)
    assert two["unlabelled_best"].tolist() == [2, 1, 0]
    assert r.add(loss[:, 3:4], [0], 7, reset=True).record()["first_undecided"] == 7


def test_the_reference_with_one_member():
    loss = np.array([[2.5, NAN, -1.0]], np.float32)
    rec = CR.Record(1).add(loss, [0, 0, 1], 0).record()
    assert (rec["n_decided"], rec["n_undecided"], rec["n_unlabelled"], rec["n_correct"], rec["n_xent"], rec["n_margin"]) == (2, 1, 1, 1, 1, 0)
    assert rec["sum_xent"] == 0.0 and rec["sum_margin"] == 0.0 and rec["confusion"].tolist() == [[1]] and rec["best"].tolist() == [0, -1, 0]
    bar_x, bar_m = CR.Record(1).add(loss, [0, 0, 1], 0).bounds()
    assert bar_x == 2.0 ** -52 * 1 * (1 + 40 + 2 * 2.5) and bar_m == 0.0


# ---------------------------------------------------------------------------------------------------
# labelled records
# ---------------------------------------------------------------------------------------------------
def test_labelled_records_and_the_extended_writer(tmp_path):
    from audio_mps_amd import tfrecord as tfr
    rng = np.random.default_rng(0)
    clips = rng.standard_normal((5, 12)).astype(np.float32)
    pitch, family = [60, 62, -3, 2 ** 40, 60], ["guitar", "organ", "", "bäss", "guitar"]
    path = os.path.join(tmp_path, "lab.tfrecords")
    tfr.write_audio_tfrecord(path, clips, int64_features={"pitch": pitch}, bytes_features={"instrument_family_str": family})
    ex = tfr.parse_example(next(tfr.read_records(path, verify=True)))
    assert set(ex) == {"audio", "pitch", "instrument_family_str"} and ex["pitch"].tolist() == [60] and ex["instrument_family_str"] == [b"guitar"]
    got = list(tfr.labelled_records(path, 12, "pitch", verify=True))
    assert [lab for _, lab in got] == pitch and all(type(lab) is int for _, lab in got)
    assert np.array_equal(bits(np.stack([a for a, _ in got])), bits(clips))
    got = list(tfr.labelled_records(path, 12, "instrument_family_str"))
    assert [lab for _, lab in got] == family and all(type(lab) is str for _, lab in got)
    assert np.array_equal(bits(np.stack(list(tfr._audio_records(path, 12, False)))), bits(clips))     # the plain reader skips the extras
    with pytest.raises(ValueError, match=r"record 0\b.*'velocity'"):
        list(tfr.labelled_records(path, 12, "velocity"))
    with pytest.raises(ValueError, match="FixedLenFeature"):
        list(tfr.labelled_records(path, 11, "pitch"))
    # a record with two values, and one without the key, named by their position in the file
    tfr.write_records(os.path.join(tmp_path, "two.tfrecords"),
                      [tfr.make_example(clips[0], {"pitch": 60}), tfr.make_example(clips[1], {"pitch": [60, 61]})])
    with pytest.raises(ValueError, match=r"record 1\b.*2 values"):
        list(tfr.labelled_records(os.path.join(tmp_path, "two.tfrecords"), 12, "pitch"))
    tfr.write_records(os.path.join(tmp_path, "gap.tfrecords"),
                      [tfr.make_example(clips[0], None, {"f": b"x"}), tfr.make_example(clips[1], None, {"f": "y"}), tfr.make_example(clips[2])])
    with pytest.raises(ValueError, match=r"record 2\b.*'f'"):
        list(tfr.labelled_records(os.path.join(tmp_path, "gap.tfrecords"), 12, "f"))
    with pytest.raises(ValueError, match=r"record 0\b.*12 values"):
        list(tfr.labelled_records(path, 12, "audio"))
    with pytest.raises(ValueError, match="FloatList"):                                 # one float is one value, but no label
        tfr.write_audio_tfrecord(os.path.join(tmp_path, "one.tfrecords"), clips[:, :1])
        list(tfr.labelled_records(os.path.join(tmp_path, "one.tfrecords"), 1, "audio"))


def test_the_default_writer_writes_the_bytes_it_always_wrote(tmp_path):
    """make_example without extras against the encoding spelled out by hand, and the file against the committed golden record."""
    from audio_mps_amd import tfrecord as tfr
    a = np.array([0.5, -1.25, 3.0], np.float32)
    floats = a.tobytes()
    feature = b"\x12" + bytes([2 + len(floats)]) + b"\x0a" + bytes([len(floats)]) + floats          # Feature{2: FloatList{1: packed}}
    entry = b"\x0a\x05audio" + b"\x12" + bytes([len(feature)]) + feature
    features = b"\x0a" + bytes([len(entry)]) + entry
    want = b"\x0a" + bytes([len(features)]) + features
    assert tfr.make_example(a) == want == tfr.make_example(a, None, None) == tfr.make_example(a, {}, {})
    p1, p2 = os.path.join(tmp_path, "a.tfrecords"), os.path.join(tmp_path, "b.tfrecords")
    tfr.write_audio_tfrecord(p1, [a, 2 * a])
    tfr.write_records(p2, [want, tfr.make_example(2 * a)])
    with open(p1, "rb") as f1, open(p2, "rb") as f2:
        data = f1.read()
        assert data == f2.read()
    head = (len(want)).to_bytes(8, "little")
    assert data.startswith(head) and data[12:12 + len(want)] == want


# ---------------------------------------------------------------------------------------------------
# the dataset's labels and the class plan
# ---------------------------------------------------------------------------------------------------
SIZES = {"a": 1, "b": 5, "c": 11}
L, MB = 16, 4


def labelled_clips(seed=1):
    """17 clips on the 16-bit grid, classes interleaved in file order."""
    rng = np.random.default_rng(seed)
    labels = np.array([c for c, n in SIZES.items() for _ in range(n)], dtype=object)
    labels = labels[rng.permutation(labels.size)]
    i = rng.integers(-8000, 8000, size=(labels.size, L)).astype(np.int16)
    return i.astype(np.float32) * np.float32(2.0 ** -15), labels


def test_dataset_labels_and_class_index(tmp_path):
    from audio_mps_amd import tfrecord as tfr
    from audio_mps_amd.device_data import ResidentDataset
    clips, labels = labelled_clips()
    be = Backend()
    plain = ResidentDataset(clips, be)
    assert plain.labels is None
    with pytest.raises(ValueError, match="labels"):
        plain.class_index(["a"])
    with pytest.raises(ValueError, match="labels"):
        plain.class_batches(["a"], MB)
    ds = ResidentDataset(clips, be, labels=labels)
    assert ds.labels.dtype == object and ds.labels.tolist() == labels.tolist()
    idx = ds.class_index(["c", "a"])
    assert idx.dtype == torch.int32 and idx.tolist() == [{"c": 0, "a": 1}.get(x, -1) for x in labels]
    with pytest.raises(ValueError, match="one label per clip"):
        ResidentDataset(clips, be, labels=labels[:-1])
    with pytest.raises(ValueError, match="distinct"):
        ds.class_index(["a", "a"])
    ints = ResidentDataset(clips, be, labels=np.arange(17) % 3 + 60)
    assert ints.labels.dtype == np.int64 and ints.class_index([62, 60]).tolist() == [{62: 0, 60: 1}.get(x, -1) for x in ints.labels]
    # through a file, with either kind of label, in either storage
    path = os.path.join(tmp_path, "lab.tfrecords")
    tfr.write_audio_tfrecord(path, clips, {"pitch": list(ints.labels)}, {"family": list(labels)})
    for storage in ("float32", "int16"):
        a = ResidentDataset.from_tfrecord(path, L, be, storage=storage, label_key="family")
        b = ResidentDataset.from_tfrecord(path, L, be, storage=storage, label_key="pitch")
        assert a.labels.tolist() == labels.tolist() and b.labels.tolist() == ints.labels.tolist() and a.storage == storage
        assert ResidentDataset.from_tfrecord(path, L, be, storage=storage).labels is None


@pytest.mark.parametrize("crop", [None, 7])
def test_class_batches_plan_is_the_plain_plan_of_every_filtered_subset(crop):
    from audio_mps_amd.device_data import ClassBatches, ResidentDataset
    clips, labels = labelled_clips()
    classes, seed = ["a", "b", "c"], 5
    be = Backend()
    ds = ResidentDataset(clips, be, labels=labels)
    stream = ds.class_batches(classes, MB, seed=seed, shuffle_buffer=3, crop=crop)
    assert isinstance(stream, ClassBatches) and len(stream) == 3
    ids = [np.flatnonzero(labels == c) for c in classes]
    assert [i.size for i in ids] == [1, 5, 11]
    plain_be = [Backend() for _ in classes]
    plain = [ResidentDataset(clips[ids[m]], plain_be[m]).batches(MB, seed=seed + m, order="estimator", shuffle_buffer=3, crop=crop,
                                                                 crop_seed=seed + m) for m in range(3)]
    stream.PLAN_STEPS = 16                                                             # 40 steps: three blocks
    for step in range(40):
        got = stream()
        assert tuple(got.shape) == (3, MB, L if crop is None else crop)
        idx, off, T, _ = be.gathers[-1]                                                # ONE gather of M B rows per step
        assert len(be.gathers) == step + 1 and idx.shape == (3 * MB,) and (off is None) == (crop is None)
        for m in range(3):
            want = plain[m]()
            pidx, poff, pT, _ = plain_be[m].gathers[-1]
            assert np.array_equal(idx[m * MB:(m + 1) * MB], ids[m][pidx]) and pT == T, (step, m)
            if crop is not None:
                assert np.array_equal(off[m * MB:(m + 1) * MB], poff), (step, m)
            assert np.array_equal(bits(got[m].numpy()), bits(want.numpy())), (step, m)
    assert stream.uploads == 3
    # the same stream on int16 storage holds the same bits
    other = ResidentDataset(clips, Backend(), storage="int16", labels=labels).class_batches(classes, MB, seed=seed, shuffle_buffer=3, crop=crop)
    again = ds.class_batches(classes, MB, seed=seed, shuffle_buffer=3, crop=crop)
    for _ in range(5):
        assert np.array_equal(bits(other().numpy()), bits(again().numpy()))
    with pytest.raises(ValueError, match="'d'"):
        ds.class_batches(["a", "d"], MB)
    with pytest.raises(ValueError, match="at least one class"):
        ds.class_batches([], MB)


# ---------------------------------------------------------------------------------------------------
# the bank
# ---------------------------------------------------------------------------------------------------
D, T = 4, 24


def hparams(B=MB):
    from audio_mps_amd import HParams
    return HParams(minibatch_size=B, bond_dim=D, delta_t=1.0 / 16000)


def class_bank(classes=("a", "b", "c"), be=None, key="family"):
    from audio_mps_amd.bank import PsiBank
    return PsiBank(hparams(), [{"seed": 3 + m} for m in range(len(classes))], backend=be or Backend(), classes=list(classes), label_key=key)


def quiet(n, length, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3000, 3000, size=(n, length)).astype(np.int16)).astype(np.float32) * np.float32(2.0 ** -15)


def test_bank_json_round_trip_and_refusals(tmp_path):
    from audio_mps_amd.bank import BankTrainer, PsiBank
    from audio_mps_amd.sample import load_bank
    bt = BankTrainer(class_bank())
    assert bt.bank.member_of("b") == 1 and bt.bank.classes == ["a", "b", "c"]
    with pytest.raises(ValueError, match="'z'"):
        bt.bank.member_of("z")
    d = str(tmp_path / "bank")
    bt.save(d)
    with open(os.path.join(d, "bank.json")) as f:
        meta = json.load(f)
    assert meta["classes"] == ["a", "b", "c"] and meta["label_key"] == "family"
    assert BankTrainer(class_bank()).restore(d)
    with pytest.raises(ValueError, match="classes"):
        BankTrainer(class_bank(("a", "c", "b"))).restore(d)
    plain = PsiBank(hparams(), [{"seed": 3 + m} for m in range(3)], backend=Backend())
    with pytest.raises(ValueError, match="classes"):
        BankTrainer(plain).restore(d)
    with pytest.raises(ValueError, match="no classes"):
        plain.member_of("a")
    loaded = load_bank(d, 16000, backend=Backend())
    assert loaded.classes == ["a", "b", "c"] and loaded.label_key == "family"
    # a bank without classes writes the file it always wrote, and a class bank does not restore from it
    d2 = str(tmp_path / "plain")
    BankTrainer(plain).save(d2)
    with open(os.path.join(d2, "bank.json")) as f:
        assert set(json.load(f)) == {"members", "adam_step", "global_step"}
    assert BankTrainer(plain).restore(d2)
    with pytest.raises(ValueError, match="classes"):
        BankTrainer(class_bank()).restore(d2)
    ints = class_bank((60, 62, 64), key="pitch")
    assert ints.member_of(62) == 1 and ints.member_of(np.int64(64)) == 2
    for bad in (["a", "b"], ["a", "a", "b"]):                                          # one class short; a class twice
        with pytest.raises(ValueError, match="one distinct class per member"):
            PsiBank(hparams(), [{"seed": 1}] * 3, backend=Backend(), classes=bad)


def test_evaluate_classifier_is_the_reference_on_the_members_losses():
    from audio_mps_amd.bank import BankTrainer, PsiBank
    from audio_mps_amd.device_data import ResidentDataset
    be = Backend()
    bt = BankTrainer(class_bank(be=be))
    clips = quiet(10, T)
    labels = np.array(list("abcabczabc"), dtype=object)                                # clip 6 carries a label the bank has no member for
    ds = ResidentDataset(clips, be, labels=labels)
    res = bt.evaluate_classifier(ds, 4, keep_best=True)
    assert be.classify_downloads == 1 and be.classify_calls == [(0, (3, 4), True), (4, (3, 4), False), (8, (3, 2), False)]
    loss = np.stack([np.concatenate([m.loss_per_clip(clips[i:i + 4]) for i in range(0, 10, 4)]) for m in bt.bank.models])
    want = CR.Record(3).add(loss, ds.class_positions(["a", "b", "c"]), 0).record()
    assert np.array_equal(res.best, want["best"]) and np.array_equal(res.confusion, want["confusion"])
    assert (res.n_clips, res.n_labelled, res.n_unlabelled, res.n_undecided, res.first_undecided) == (10, 9, 1, 0, -1)
    assert res.n_correct == want["n_correct"] and res.accuracy == want["n_correct"] / 9
    assert res.cross_entropy == want["sum_xent"] / 9 and res.mean_margin == want["sum_margin"] / 10 and res.T == T
    assert np.array_equal(res.recall, np.diagonal(want["confusion"]) / want["confusion"].sum(axis=1))
    s = res.scalars()
    json.dumps(s)
    assert {"accuracy", "cross_entropy", "mean_margin", "n_clips", "n_undecided", "n_unlabelled", "first_undecided", "recall",
            "classes"} <= set(s) and "confusion" not in s and "best" not in s
    assert bt.evaluate_classifier(ResidentDataset(clips, be), 4).n_unlabelled == 10    # a dataset without labels: nothing to be right about
    nb = NoClassifyBackend()
    with pytest.raises(ValueError, match="classify_stats") as e:
        BankTrainer(class_bank(be=nb)).evaluate_classifier(ResidentDataset(clips, nb, labels=labels), 4)
    assert "NoClassifyBackend" in str(e.value)
    with pytest.raises(ValueError, match="class bank"):
        BankTrainer(PsiBank(hparams(), [{"seed": 1}], backend=be)).evaluate_classifier(ds, 4)


# ---------------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------------
def _files(tmp):
    from audio_mps_amd import tfrecord as tfr
    labels = ["x", "y", "y", "x", "y", "x", "y"]
    tfr.write_audio_tfrecord(os.path.join(tmp, "guitar.tfrecords"), quiet(7, T, 3), {"pitch": [60 + (c == "y") for c in labels]}, {"fam": labels})
    held = ["y", "x", "x", "y", "q"]
    tfr.write_audio_tfrecord(os.path.join(tmp, "organ.tfrecords"), quiet(5, T, 4), {"pitch": [60, 61, 61, 60, 99]}, {"fam": held})


def _argv(tmp, extra=()):
    return ["--dataset", "guitar", "--datadir", str(tmp), "--sample_duration", str(T), "--max_steps", "3", "--seed", "5",
            "--hparams", f"bond_dim={D},minibatch_size=2", "--logdir", os.path.join(tmp, "log"), "--device_data"] + list(extra)


def test_train_bank_by_and_evaluate_bankdir(tmp_path, capsys):
    from audio_mps_amd import evaluate as EV, sample, train
    from audio_mps_amd.bank import BankTrainer
    _files(tmp_path)
    be = Backend()
    tr = train.main(_argv(tmp_path, ["--bank_by", "fam", "--eval_dataset", "organ", "--eval_every", "2", "--eval_minibatch", "4"]), backend=be)
    out = capsys.readouterr().out
    assert isinstance(tr, BankTrainer) and tr.bank.classes == ["x", "y"] and tr.bank.seeds == [5, 6] and tr.global_step == 3
    assert [g[0].shape for g in be.gathers[:3]] == [(4,)] * 3                          # one gather of M B rows per training step
    lines = [ln for ln in out.splitlines() if ln.startswith("eval ")]
    assert len(lines) == 2 and all(all(k in ln for k in ("step=", "accuracy=", "xent=", "margin=", "clips=5", "undecided=0")) for ln in lines)
    logdir = os.path.join(tmp_path, "log", "guitar", f"{D}_{1.0 / 16000}_2")
    with open(os.path.join(logdir, "eval.jsonl")) as f:
        recs = [json.loads(line) for line in f]
    assert [r["global_step"] for r in recs] == [2, 3] and all(r["n_clips"] == 5 and r["n_unlabelled"] == 1 for r in recs)
    assert be.classify_downloads == 2
    # ints as classes, named on the command line, in the order given
    tr2 = train.main(_argv(tmp_path, ["--bank_by", "pitch", "--bank_classes", "61,60", "--logdir", os.path.join(tmp_path, "log2"),
                                      "--crop_duration", "10"]), backend=Backend())
    assert tr2.bank.classes == [61, 60] and tr2.bank.label_key == "pitch"
    # the saved bank judged from its directory: the figures of the last evaluation of the run
    capsys.readouterr()
    conf, per = os.path.join(tmp_path, "conf.npy"), os.path.join(tmp_path, "best.npy")
    res = EV.main(["--bankdir", logdir, "--datadir", str(tmp_path), "--dataset", "organ", "--sample_duration", str(T), "--minibatch_size", "4",
                   "--confusion", conf, "--per_clip", per, "--json"], backend=Backend())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("eval organ: accuracy=") and "classes=2" in lines[0]
    rec = json.loads(lines[1])
    assert rec["accuracy"] == recs[-1]["accuracy"] and rec["cross_entropy"] == recs[-1]["cross_entropy"] and rec["classes"] == ["x", "y"]
    assert np.array_equal(np.load(conf), res.confusion) and np.load(conf).shape == (2, 2) and np.load(conf).sum() == 4
    assert np.load(per).dtype == np.int32 and np.load(per).shape == (5,)
    # sample --score names the class of every member
    np.save(os.path.join(tmp_path, "clip.npy"), quiet(1, T, 9)[0])
    if hasattr(sample, "_bank_main"):
        bank = sample.load_bank(logdir, 16000, backend=Backend())
        assert bank.classes == ["x", "y"] and bank.member_of("y") == 1


def test_sample_score_names_the_class_of_every_member(tmp_path, capsys):
    from test_score_host import ScoreBackend
    from _util import make_audio
    from audio_mps_amd import HParams, sample as S
    from audio_mps_amd.bank import BankTrainer, PsiBank
    hp = HParams(delta_t=1.0 / 16000, h_reg=200.0 / (np.pi * 16000) ** 2, minibatch_size=2, bond_dim=D)      # what sample.main assumes
    members = [{"seed": 3}, {"seed": 4}, {"seed": 5}]
    d, out = str(tmp_path / "bank"), str(tmp_path / "out")
    BankTrainer(PsiBank(hp, members, backend=ScoreBackend(D), classes=["bass", "flute", "organ"], label_key="fam")).save(d)
    clip = str(tmp_path / "clip.npy")
    np.save(clip, make_audio(1, 15, hp.delta_t, seed=4)[0])
    nll = S.main(["--bankdir", d, "--out_dir", out, "--score", clip], backend=ScoreBackend(D))
    lines = capsys.readouterr().out.strip().splitlines()
    names = ["bass", "flute", "organ"]
    assert len(lines) == 4 and all(lines[m].startswith(f"member {m} (class '{names[m]}'): total nll") for m in range(3))
    best = int(np.argmin(nll.astype(np.float64).sum(axis=1)))
    assert lines[-1].startswith(f"best member {best} (class '{names[best]}') of 3")


@pytest.mark.parametrize("extra, match", [
    (["--bank_by", "fam", "--bank", "2"], "--bank N"), (["--bank_by", "fam", "--bank_hparams", "r_reg=0.1,1"], "--bank_hparams"),
    (["--bank_by", "fam", "--host_optimizer"], "--host_optimizer"), (["--bank_by", "fam", "--eval_dataset", "damped_sine"], "no labels"),
    (["--bank_by", "fam", "--eval_every", "2"], "--eval_dataset"), (["--bank_classes", "x"], "--bank_by"),
    (["--bank_by", "fam", "--bank_classes", "x,nobody"], "'nobody'"), (["--bank_by", "velocity"], "'velocity'"),
    (["--bank", "2", "--eval_dataset", "organ"], "--eval_dataset")])
def test_train_refusals(tmp_path, extra, match):
    from audio_mps_amd import train
    _files(tmp_path)
    with pytest.raises(ValueError, match=match):
        train.main(_argv(tmp_path, extra), backend=Backend())
    assert not os.path.exists(os.path.join(tmp_path, "log"))


def test_bank_by_needs_device_data_and_a_file(tmp_path):
    from audio_mps_amd import evaluate as EV, train
    _files(tmp_path)
    argv = _argv(tmp_path, ["--bank_by", "fam"])
    argv.remove("--device_data")
    with pytest.raises(ValueError, match="--device_data"):
        train.main(argv, backend=Backend())
    sine = [a if a != "guitar" else "damped_sine" for a in _argv(tmp_path, ["--bank_by", "fam"])]
    with pytest.raises(ValueError, match="damped_sine has no labels"):
        train.main(sine, backend=Backend())
    with pytest.raises(ValueError, match="--bankdir"):
        EV.main(["--modeldir", str(tmp_path), "--dataset", "organ", "--confusion", "c.npy"], backend=Backend())
