"""BankTrainer.calibrate / cross_entropy and the command lines on the GPU, for a PsiCMPS and a RhoCMPS class bank: D = 4, M = 3, B = 4,
T = 24, twelve labelled held-out clips (rank 3 for the RhoCMPS members).  The kernels themselves are tested in tests/test_gpu_calibrate.py."""
import json
import os

import numpy as np
import pytest
import torch

import _calib_ref as R
import _classify_ref as CR

pytestmark = pytest.mark.gpu

D, T, B, RANK = 4, 24, 4, 3
CLASSES = [62, 60, 67]                                                                 # (member order is not label order)
HELD = np.array([60, 62, 67, 62, 60, 67, 71, 60, 62, 67, 62, 60], dtype=np.int64)      # 71: a label the bank has no member for


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pcm(n, length, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64)
    f = rng.uniform(0.02, 0.2, (n, 1))
    x = 0.2 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6, (n, 1))) + 0.01 * rng.standard_normal((n, length))
    return np.round(x * 32768.0).astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15)


def make_trainer(kind):
    from audio_mps_amd import HParams
    from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D, delta_t=1.0 / 16000, initial_rank=RANK if kind == "rho" else None)
    bank = (RhoBank if kind == "rho" else PsiBank)(hp, [{"seed": 20 + m} for m in range(3)], backend=HipScan(D), classes=CLASSES,
                                                   label_key="pitch")
    return BankTrainer(bank)


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_calibrate_is_bank_calibrate_on_the_forward_losses_and_leaves_training_alone(kind):
    from audio_mps_amd.device_data import ResidentDataset
    cal, twin, fwd = make_trainer(kind), make_trainer(kind), make_trainer(kind)
    assert cal.native
    train_clips, train_labels = pcm(18, T, 4), np.array(CLASSES * 6, dtype=np.int64)
    streams = [ResidentDataset(train_clips, tr.bank.backend, labels=train_labels).class_batches(CLASSES, B, seed=11) for tr in (cal, twin, fwd)]
    for tr, s in zip((cal, twin, fwd), streams):
        tr.step(s(), sync=False)
    held = pcm(12, T, 6)
    ds = ResidentDataset(held, cal.bank.backend, labels=HELD)
    res = cal.calibrate(ds, fit="both", max_iter=60)
    x_uniform = cal.cross_entropy(ds, 1.0, None)
    plain = cal.evaluate_classifier(ds)
    # (a) the same call on the losses of bank_forward over the same ordered batches, bit for bit
    be = fwd.bank.backend
    ds2 = ResidentDataset(held, be, labels=HELD)
    fwd._configure(fwd._device_state(), B, T, False)
    loss = torch.cat([fwd._forward(batch, save_for_bwd=False).clone() for _, batch in ds2.ordered(B, T)], dim=1)
    labels = ds2.class_index(CLASSES)
    theta, rec = be.read_calibrate_record(be.bank_calibrate(loss, labels, 3, 1.0, None, 1e-9, 60, 1e-6, 1e6))
    assert loss.shape == (3, 12) and bits64(1.0 / theta[0]) == bits64(res.temperature) and np.array_equal(bits64(theta[1:]), bits64(res.log_prior))
    assert (rec["xent_start"], rec["xent_end"], rec["passes"], rec["n_used"], rec["n_unlabelled"]) == \
        (res.xent_before, res.xent_after, res.passes, res.n_used, res.n_unlabelled) and res.n_used == 11 and res.n_unlabelled == 1
    assert res.xent_after <= res.xent_before and res.T == T and res.unfitted == [] and cal.calibration == res.meta()
    # (b) cross_entropy at temperature 1 and the uniform prior is evaluate_classifier's, within the two entries' bounds
    l, y = loss.cpu().numpy(), labels.cpu().numpy()
    ref = R.evaluate(l, y, 1.0, np.zeros(3), np.longdouble)
    bar_stats = CR.Record(3).add(l, y, 0).bounds()[0] / ref.n + 2.0 ** -52 * abs(plain.cross_entropy)
    bar_calib = ref.bounds()[0]
    print(f"{kind}: xent {x_uniform} (calibrate) {plain.cross_entropy} (classify_stats) {float(ref.J)} (long double); bars {bar_calib:.2e} "
          f"{bar_stats:.2e}; fitted temperature {res.temperature} prior {res.prior} xent {res.xent_before} -> {res.xent_after}")
    assert bits64(x_uniform) == bits64(res.xent_before)
    assert abs(x_uniform - float(ref.J)) <= bar_calib and abs(x_uniform - plain.cross_entropy) <= bar_calib + bar_stats
    # (c) three training steps after it are those of the twin that never calibrated
    for _ in range(3):
        for tr, s in zip((cal, twin), streams[:2]):
            tr.step(s(), sync=False)
    for m in range(3):
        for k, v in twin.member(m).variables.items():
            assert np.array_equal(bits32(cal.member(m).variables[k]), bits32(v)), (m, k)


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_command_lines(kind, tmp_path, capsys):
    from audio_mps_amd import evaluate as EV, sample as S, tfrecord as tfr
    from audio_mps_amd.bank import normalised_prior
    d, out1, out2 = str(tmp_path / "bank"), str(tmp_path / "o1"), str(tmp_path / "o2")
    make_trainer(kind).save(d)
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "held.tfrecords"), pcm(12, T, 6), {"pitch": [int(v) for v in HELD]})
    common = ["--bankdir", d, "--datadir", str(tmp_path), "--dataset", "held", "--sample_duration", str(T), "--minibatch_size", str(B)]
    EV.main(common + ["--calibrate", "both", "--save_calibration"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[1].startswith("calibration temperature=") and sum(ln.startswith("class ") for ln in lines) == 3
    with open(os.path.join(d, "bank.json")) as f:
        saved = json.load(f)["calibration"]
    assert (saved["fit"], saved["dataset"], saved["clips"], saved["T"]) == ("both", "held", 11, T) and saved["xent_after"] <= saved["xent_before"]
    EV.main(common + ["--calibrated", "--json"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(kind, saved, rec["xent_calibrated"])
    # (the saved temperature is 1 / kappa and the zero-iteration call forms kappa = 1 / temperature again: one rounding of kappa apart)
    assert abs(rec["xent_calibrated"] - saved["xent_after"]) <= 1e-12 * max(1.0, saved["xent_after"])
    clip = str(tmp_path / "clip.npy")
    np.save(clip, pcm(1, T, 9)[0])
    score = ["--bankdir", d, "--score", clip, "--posterior"]
    S.main(score + ["--out_dir", out1, "--calibrated"])
    prior = normalised_prior(saved["log_prior"])
    S.main(score + ["--out_dir", out2, "--temperature", repr(float(saved["temperature"])), "--prior", ",".join(repr(float(p)) for p in prior)])
    a, b = np.load(os.path.join(out1, "posterior.npy")), np.load(os.path.join(out2, "posterior.npy"))
    assert a.shape == (3, T - 1) and np.array_equal(bits32(a), bits32(b))
    uniform = str(tmp_path / "o3")
    S.main(score + ["--out_dir", uniform])
    assert not np.array_equal(bits32(a), bits32(np.load(os.path.join(uniform, "posterior.npy"))))


class MemberLoopScan:
    """A HipScan that shows no bank entries: a BankTrainer on it loops over its members' plain forward scans."""
    HIDDEN = ("bank_set_params_dev", "bank_forward", "bank_backward", "bank_apply_step", "rho_bank_set_state_dev", "rho_bank_forward",
              "rho_bank_backward", "rho_bank_apply_step")

    def __init__(self, D):
        from audio_mps_amd.scan import HipScan
        self._be = HipScan(D)

    def __getattr__(self, name):
        if name in MemberLoopScan.HIDDEN:
            raise AttributeError(name)
        return getattr(self._be, name)


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_the_member_loop_gives_what_the_bank_entries_give(kind):
    """`calibrate` on a backend without the bank entries scores the batches member by member: the same losses, so the same fit, bit for bit."""
    from audio_mps_amd import HParams
    from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
    from audio_mps_amd.device_data import ResidentDataset
    native = make_trainer(kind)
    hp = HParams(minibatch_size=B, bond_dim=D, delta_t=1.0 / 16000, initial_rank=RANK if kind == "rho" else None)
    loop = BankTrainer((RhoBank if kind == "rho" else PsiBank)(hp, [{"seed": 20 + m} for m in range(3)], backend=MemberLoopScan(D),
                                                               classes=CLASSES, label_key="pitch"))
    assert native.native and not loop.native
    held = pcm(12, T, 6)
    got = [tr.calibrate(ResidentDataset(held, tr.bank.backend, labels=HELD), fit="both", max_iter=40) for tr in (native, loop)]
    a, b = got
    assert bits64(a.temperature) == bits64(b.temperature) and np.array_equal(bits64(a.log_prior), bits64(b.log_prior))
    assert (a.xent_before, a.xent_after, a.passes, a.n_used, a.unfitted) == (b.xent_before, b.xent_after, b.passes, b.n_used, b.unfitted)
    x = [tr.cross_entropy(ResidentDataset(held, tr.bank.backend, labels=HELD), 3.0, [0.2, 0.3, 0.5]) for tr in (native, loop)]
    assert bits64(x[0]) == bits64(x[1])
