"""The host side of discriminative class-bank training without a GPU: the numpy reference of cmps_bank_classify_weights
(tests/_disc_ref.py) against central differences of the objective it differentiates, its skip rules by hand, its cross-entropy against
tests/_classify_ref.py, ResidentDataset.labelled_batches against the plain stream it is built from, and train.py's flag errors.  The kernel
is tied to the same reference in tests/test_gpu_classify_weights.py, the step to its five backend calls in tests/test_gpu_disc_step.py."""
import math
import os

import numpy as np
import pytest
import torch

import _classify_ref as CR
import _disc_ref as DR
from test_classify_host import Backend, _argv, _files, bits, class_bank, labelled_clips, quiet

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa,alpha,beta", [(1.0, 0.0, 1.0), (0.25, 0.5, 2.0), (3.0, 1.0, 0.0)])
def test_reference_weights_are_the_central_differences_of_the_objective(kappa, alpha, beta):
    rng = np.random.default_rng(11)
    M, B = 4, 6
    loss = (rng.standard_normal((M, B)) * 1.5 + 5.0).astype(np.float32)
    loss[2, 1], loss[0, 4] = NAN, INF                                                  # another member absent in clips 1 and 4
    labels = np.array([0, 1, 3, 2, 1, 9])                                              # clip 5 unlabelled
    got = DR.weights(loss, labels, kappa, alpha, beta)
    x = loss.astype(np.float64)
    h = 1e-5
    # J is smooth in every present l_m with third derivatives of order beta kappa^3: the central difference is within
    # h^2 beta kappa^3 of the derivative, and rounding adds |J| 2^-52 / h
    tol = h * h * (beta * kappa ** 3 + 1.0) + 200.0 * 2.0 ** -52 / h
    for m in range(M):
        for b in range(B):
            if not np.isfinite(x[m, b]):
                assert got["w64"][m, b] == 0.0
                continue
            up, dn = x.copy(), x.copy()
            up[m, b] += h
            dn[m, b] -= h
            fd = (DR.objective(up, labels, kappa, alpha, beta) - DR.objective(dn, labels, kappa, alpha, beta)) / (2 * h)
            assert abs(fd - got["w64"][m, b]) <= tol, (m, b, fd, got["w64"][m, b])
    assert np.array_equal(got["w"], got["w64"].astype(np.float32))
    # every used clip's discriminative part sums to zero over the members: sum_m (delta - p) = 0
    used = got["state"] == 0
    assert np.all(np.abs(got["w64"][:, used].sum(axis=0) - alpha) <= 1e-15 * (alpha + beta * kappa) * M)


def test_reference_skip_rules_by_hand():
    #            clip 0 used   1 unlabelled  2 own absent  3 another absent  4 all absent  5 label -1
    loss = np.array([[1.0,     2.0,          NAN,          NAN,              NAN,          1.0],
                     [3.0,     2.0,          4.0,          4.0,              INF,          2.0],
                     [2.0,     7.0,          6.0,          6.0,              -INF,         3.0]], np.float32)
    labels = [0, 3, 0, 2, 1, -1]
    got = DR.weights(loss, labels, 1.0, 0.0, 1.0)
    assert got["state"].tolist() == [0, 1, 2, 0, 2, 1]
    w = got["w"]
    assert np.array_equal(bits(w[:, [1, 2, 4, 5]]), np.zeros((3, 4), np.uint32))       # skipped clips: +0, bit for bit
    assert bits(w[0:1, 3:4])[0, 0] == 0                                                # the absent member of a used clip: +0
    e = np.exp(-np.array([0.0, 2.0, 1.0]))
    assert np.allclose(got["w64"][:, 0], np.array([1.0, 0.0, 0.0]) - e / e.sum(), rtol=1e-15, atol=0)
    e3 = np.exp(-np.array([0.0, 2.0]))                                                 # clip 3: members 1 and 2, label 2 loses by 2
    assert np.allclose(got["w64"][1:, 3], np.array([0.0, 1.0]) - e3 / e3.sum(), rtol=1e-15, atol=0)
    assert got["xent"][3] == pytest.approx(2.0 + math.log(1 + math.exp(-2)), rel=1e-15)
    rec = DR.record([got])
    assert (rec["n_used"], rec["n_unlabelled"], rec["n_own_absent"]) == (2, 2, 2) and rec["sum_own_loss"] == 1.0 + 6.0
    # gen_weight alone: the own member's weight is exactly alpha, every other exactly +0
    gen = DR.weights(loss, labels, 2.0, 1.0, 0.0)["w"]
    assert np.array_equal(bits(gen[:, 0]), bits([1.0, 0.0, 0.0])) and np.array_equal(bits(gen[:, 3]), bits([0.0, 0.0, 1.0]))
    # M = 1: p = 1, the discriminative weight vanishes, xent = 0
    one = DR.weights(np.array([[2.5, NAN, -1.0]], np.float32), [0, 0, 1], 0.5, 0.25, 3.0)
    assert one["state"].tolist() == [0, 2, 1] and one["w"].tolist() == [[0.25, 0.0, 0.0]] and one["xent"][0] == 0.0
    # a far member: p underflows to exactly 0 and its weight is +0; the own member's p is 1
    far = DR.weights(np.array([[1.0], [2000.0]], np.float32), [0], 1.0, 0.0, 1.0)
    assert np.array_equal(bits(far["w"]), np.zeros((2, 1), np.uint32)) and far["xent"][0] == 0.0


def test_reference_cross_entropy_at_unit_temperature_is_classify_stats():
    rng = np.random.default_rng(3)
    M, B = 5, 40
    loss = (rng.standard_normal((M, B)) * 3.0 + 10.0).astype(np.float32)
    loss[rng.random((M, B)) < 0.1] = NAN
    labels = rng.integers(-1, M + 1, size=B)
    got = DR.record([DR.weights(loss, labels, 1.0, 0.3, 0.7)])
    ref = CR.Record(M).add(loss, labels, 0)
    want = ref.record()
    assert got["n_used"] == want["n_xent"] > 10
    fin = loss[np.isfinite(loss)]
    bar = DR.record_bounds(got, M, 1.0, float(np.abs(fin).max()), 0.0)[0] + ref.bounds()[0]
    assert abs(got["sum_xent"] - want["sum_xent"]) <= bar
    # a clip without a present member is undecided there and "own member absent" (or unlabelled) here; the two records count it differently
    assert got["n_used"] + got["n_unlabelled"] + got["n_own_absent"] == B


# ---------------------------------------------------------------------------------------------------
# labelled batches
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,crop", [("data", None), ("estimator", 7)])
def test_labelled_batches_are_the_plain_batches_with_their_rows_labels(order, crop):
    from audio_mps_amd.device_data import ResidentDataset
    clips, labels = labelled_clips()
    classes = ["c", "a"]                                                               # "b" is not among them: -1
    kw = dict(seed=5, order=order, shuffle_buffer=3, crop=crop, crop_seed=9)
    be, be2 = Backend(), Backend()
    stream = ResidentDataset(clips, be, labels=labels).labelled_batches(classes, 4, **kw)
    plain = ResidentDataset(clips, be2, labels=labels).batches(4, **kw)
    where = {"c": 0, "a": 1}
    for step in range(23):                                                             # several epochs of 17 clips, short batches included
        assert stream.next_size == plain.next_size
        got, lab = stream()
        want = plain()
        assert np.array_equal(bits(got.numpy()), bits(want.numpy())), step
        idx = be.gathers[-1][0]
        assert np.array_equal(idx, be2.gathers[-1][0]) and np.array_equal(plain.last_index.numpy(), idx)
        assert lab.dtype == torch.int32 and lab.tolist() == [where.get(labels[i], -1) for i in idx], step
    with pytest.raises(ValueError, match="labels"):
        ResidentDataset(clips, Backend()).labelled_batches(classes, 4)


def test_batch_stream_output_is_unchanged_by_last_index():
    """The same stream read with and without anyone looking at last_index, whole and in shards: the same rows, and last_index names them."""
    from audio_mps_amd.device_data import ResidentDataset
    clips, _ = labelled_clips()
    be_a, be_b = Backend(), Backend()
    a = ResidentDataset(clips, be_a).batches(4, seed=2, shuffle_buffer=5)
    b = ResidentDataset(clips, be_b).batches(4, seed=2, shuffle_buffer=5)
    assert a.last_index is None
    rng = np.random.default_rng(2)                                                     # the plan a stream of this seed draws, restated
    from audio_mps_amd import tfrecord
    rows = [list(range(i, min(i + 4, 17))) for i in range(0, 17, 4)]
    planned = [r for _ in range(3) for r in tfrecord._shuffle(iter(rows), 5, rng)]     # (three epochs of five batches)
    for step in range(12):
        n = a.next_size
        shard = (1, 2) if step % 3 == 1 else None
        x, y = a(shard=shard), b(shard=shard)
        _ = a.last_index.tolist()                                                      # only one of the two is looked at
        assert np.array_equal(bits(x.numpy()), bits(y.numpy())) and np.array_equal(be_a.gathers[-1][0], be_b.gathers[-1][0])
        lo, hi = (0, n) if shard is None else (1, min(3, n))
        assert np.array_equal(a.last_index.numpy(), be_a.gathers[-1][0]) and len(a.last_index) == hi - lo
        assert a.last_index.tolist() == planned[step][lo:hi], step
        assert np.array_equal(bits(x.numpy()), bits(clips[a.last_index.numpy()]))


# ---------------------------------------------------------------------------------------------------
# the trainer and the command line
# ---------------------------------------------------------------------------------------------------
def test_step_classifier_refusals():
    from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
    from test_classify_host import hparams
    be = Backend()
    data, labels = quiet(4, 24), np.array([0, 1, 2, 0], np.int32)
    with pytest.raises(ValueError, match="class bank"):
        BankTrainer(PsiBank(hparams(), [{"seed": 1}], backend=be)).step_classifier(data, labels[:4])
    with pytest.raises(ValueError, match="native path") as e:                          # the stand-in has no bank entries: no silent loop
        BankTrainer(class_bank(be=be)).step_classifier(data, labels)
    assert "Backend" in str(e.value)
    rho = RhoBank(hparams(), [{"seed": 3 + m} for m in range(3)], backend=be, classes=["a", "b", "c"], label_key="family")
    with pytest.raises(ValueError, match="RhoBank"):
        BankTrainer(rho).step_classifier(data, labels)


@pytest.mark.parametrize("extra, match", [
    (["--bank_objective", "discriminative"], "--bank_by"),
    (["--bank", "2", "--bank_objective", "discriminative"], "--bank_by"),
    (["--bank_by", "fam", "--disc_temperature", "5"], "--bank_objective discriminative"),
    (["--bank_by", "fam", "--gen_weight", "1"], "--bank_objective discriminative"),
    (["--disc_weight", "2"], "--bank_objective discriminative"),
    (["--bank_by", "fam", "--bank_objective", "discriminative", "--mps_model", "rho_mps"], "no --mps_model rho_mps"),
    (["--bank_by", "fam", "--bank_objective", "discriminative", "--disc_temperature", "0"], "--disc_temperature > 0"),
    (["--bank_by", "fam", "--bank_objective", "discriminative", "--disc_temperature", "inf"], "finite"),
    (["--bank_by", "fam", "--bank_objective", "discriminative", "--disc_weight", "-1"], "--disc_weight >= 0"),
    (["--bank_by", "fam", "--bank_objective", "discriminative", "--gen_weight", "nan"], "--gen_weight >= 0"),
    (["--bank_by", "fam", "--bank_objective", "discriminative"], "cmps_bank_classify_weights")])      # (the stand-in backend has none)
def test_train_flag_errors(tmp_path, extra, match):
    from audio_mps_amd import train
    _files(tmp_path)
    with pytest.raises(ValueError, match=match):
        train.main(_argv(tmp_path, extra), backend=Backend())
    assert not os.path.exists(os.path.join(tmp_path, "log"))


def test_train_flags_default_to_the_generative_path_and_explain_the_temperature(tmp_path):
    from audio_mps_amd import train
    p = train.build_parser()
    a = p.parse_args(["--bank_by", "fam"])
    assert (a.bank_objective, a.disc_weight, a.gen_weight, a.disc_temperature) == ("generative", 1.0, 0.0, 1.0)
    with pytest.raises(SystemExit):
        p.parse_args(["--bank_objective", "both"])
    text = " ".join(p.format_help().split())
    assert "sample_duration - 1 samples" in text and "saturating" in text
    # the generative run writes the bank.json it always wrote
    import json
    _files(tmp_path)
    tr = train.main(_argv(tmp_path, ["--bank_by", "fam"]), backend=Backend())
    assert tr.objective is None
    with open(os.path.join(tmp_path, "log", "guitar", f"4_{1.0 / 16000}_2", "bank.json")) as f:
        assert "objective" not in json.load(f)
    # ... and a trainer told its objective records it
    tr.objective = {"name": "discriminative", "disc_weight": 1.0, "gen_weight": 0.0, "temperature": 24.0}
    d = str(tmp_path / "disc")
    tr.save(d)
    with open(os.path.join(d, "bank.json")) as f:
        assert json.load(f)["objective"] == tr.objective
