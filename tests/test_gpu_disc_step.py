"""BankTrainer.step_classifier on a real MI355X: a two-class bank (damped sines of two pitches; D = 4, T = 256, B = 8, M = 2) trained
against itself.

  * one step_classifier is, bit for bit, the five backend calls chained by hand -- cmps_bank_set_params_dev, cmps_bank_loss_fwd,
    cmps_bank_classify_weights, cmps_bank_loss_bwd_weighted, cmps_bank_apply_step: variables, Adam slots, effective parameters, losses_dev;
  * the steps after a step_classifier are bit for bit those of a bank restored from its checkpoint;
  * gen_weight = 1, disc_weight = 0 on a batch whose clips all belong to one class leaves the other member to its regularisers: its
    weights are exactly 0, so its gradient row is exactly 0, and the Adam update of A and psi_0 from zero slots is 0 -- those variables
    keep their bits.  Rx, Ry and freqs still take the step of the regularisers (the optimiser step always runs with them, and r_reg = 0 or
    h_reg = 0 is not a model: the variables are scaled by 1 / sqrt of them), which does not depend on the batch: a different batch of that
    class leaves the other member with the same bits.
What the objective learns is recorded by scripts/time_disc_bank.py, not asserted here."""
import math

import numpy as np
import pytest
import torch

import _disc_ref as DR

pytestmark = pytest.mark.gpu

D, T, B, M = 4, 256, 8, 2
PITCH = (220.0, 440.0)


def clips(n, seed):
    """n damped sines, pitch PITCH[label], random onset and a little noise -> (float32 [n, T], labels [n])."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, M, n)
    t = np.arange(T) / 16000.0
    out = np.zeros((n, T), np.float32)
    for i, y in enumerate(labels):
        s = t - rng.uniform(0.0, 0.004)
        out[i] = (0.5 * (s > 0) * np.sin(2 * np.pi * PITCH[y] * s) * np.exp(-np.maximum(s, 0) / 0.01) + 0.01 * rng.standard_normal(T)).astype(np.float32)
    return out, labels.astype(np.int32)


def trainer(hp=None, **member):
    from audio_mps_amd import HParams
    from audio_mps_amd.bank import BankTrainer, PsiBank
    from audio_mps_amd.scan import HipScan
    hp = HParams(minibatch_size=B, bond_dim=D) if hp is None else hp
    bank = PsiBank(hp, [{"seed": 3 + m, **member} for m in range(M)], backend=HipScan(D), classes=[0, 1], label_key="pitch")
    return BankTrainer(bank)


def state(bt):
    torch.cuda.synchronize()
    return {k: bt._dev[k].cpu().numpy().copy() for k in ("vars", "m", "v", "params", "losses")}


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a) and a.keys() == b.keys()


KW = dict(gen_weight=0.25, disc_weight=1.0, temperature=float(T))


def test_step_classifier_is_the_five_backend_calls():
    data, labels = clips(B, 1)
    bt = trainer()
    out = bt.step_classifier(data, labels, **KW)
    got = state(bt)
    assert out["global_step"] == 1 and out["used"] == B and out["unlabelled"] == 0 and out["own_absent"] == 0
    assert [tr.opt.t for tr in bt.trainers] == [1] * M and [tr.global_step for tr in bt.trainers] == [1] * M

    by_hand = trainer()
    st = by_hand._device_state()                                                        # the members' variables, zero slots, hyper
    start = state(by_hand)
    be, m0, o = by_hand.bank.backend, by_hand.bank.models[0], by_hand.trainers[0].opt
    audio = torch.from_numpy(data).to(be.device)
    lab = torch.from_numpy(labels).to(be.device)
    be.bank_set_params_dev(st["params"], m0.sigma, m0.delta_t, B, T, train=True)
    loss = be.bank_forward(audio, save_for_bwd=True)
    w, rec = be.classify_weights(loss, lab, 1.0 / KW["temperature"], KW["gen_weight"], KW["disc_weight"])
    flat = be.bank_backward(weights=w)
    be.bank_apply_step(st["vars"], st["m"], st["v"], flat, B, math.sqrt(1.0 - o.b2), 1.0 - o.b1, o.b1, o.b2, o.eps, st["hyper"], True,
                       st["params"], st["losses"])
    want = state(by_hand)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(out["model_loss"], want["losses"][:, 0]) and np.array_equal(out["total_loss"], want["losses"][:, 1])
    # the record it reports, against the numpy reference on the very losses of that forward
    x = loss.cpu().numpy()
    ref = DR.weights(x, labels, 1.0 / KW["temperature"], KW["gen_weight"], KW["disc_weight"])
    r = DR.record([ref])
    bar = 2 * DR.record_bounds(r, M, 1.0 / KW["temperature"], float(np.abs(x).max()), 0.0)[0]
    assert abs(out["xent"] * B - r["sum_xent"]) <= bar + 2.0 ** -52 * r["sum_xent"]
    assert np.all(np.abs(w.cpu().numpy().astype(np.float64) - ref["w64"])
                  <= 2 * DR.weight_bound(ref["w64"], M, 1.0 / KW["temperature"], KW["gen_weight"], KW["disc_weight"]))
    # model_loss is the member's weighted loss sum / B
    # (a double sum of exact products, rounded to float32 in grad_dev and once more after the division: 2^-23 of sum |w l| / B covers both)
    wx = w.cpu().numpy().astype(np.float64) * x.astype(np.float64)
    assert np.all(np.abs(out["model_loss"] - wx.sum(axis=1) / B) <= 2.0 ** -23 * np.abs(wx).sum(axis=1) / B)
    assert not np.array_equal(got["vars"], start["vars"])                                # (it moved)


def test_steps_after_a_classifier_step_equal_a_restored_bank(tmp_path):
    data, labels = clips(B, 2)
    more, more_labels = clips(B, 3)
    a = trainer()
    a.step_classifier(data, labels, **KW)
    a.save(str(tmp_path))
    b = trainer()
    assert b.restore(str(tmp_path)) and b.global_step == 1 and b.trainers[0].opt.t == 1
    for bt in (a, b):
        bt.step_classifier(more, more_labels, **KW)
        bt.step(data)                                                                   # a generative step on a shared batch
        bt.step_classifier(data, labels, gen_weight=1.0, disc_weight=0.5, temperature=64.0, sync=False)
    sa, sb = state(a), state(b)
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k
    assert a.global_step == b.global_step == 4


def test_generative_weights_on_one_class_leave_the_other_member_alone():
    data, labels = clips(4 * B, 4)
    from audio_mps_amd import layout
    own, other = data[labels == 1][:B], data[labels == 1][B:2 * B]
    assert own.shape == other.shape == (B, T) and not np.array_equal(own, other)
    kw = dict(gen_weight=1.0, disc_weight=0.0, temperature=3.0)
    bt = trainer()
    bt._device_state()
    before = state(bt)
    out = bt.step_classifier(own, np.ones(B, np.int32), **kw)
    after = state(bt)
    fields = layout.var_fields(D)
    b0, a0 = ({k: layout.unpack(fields, s[k][0]) for k in ("vars", "m", "v")} for s in (before, after))
    for f in ("A", "psi_x", "psi_y"):                  # no regulariser acts on these: untouched, and their slots stay zero
        assert np.array_equal(np.asarray(a0["vars"][f]).view(np.uint32), np.asarray(b0["vars"][f]).view(np.uint32)), f
        assert np.all(np.asarray(a0["m"][f]) == 0.0) and np.all(np.asarray(a0["v"][f]) == 0.0), f
    # Rx, Ry and freqs do move -- by the regularisers, whose gradient (2 Rx, 2 Ry, 2 freqs on the scaled variables) does not depend on the
    # batch: another batch of class 1 leaves member 0 with the same bits, and member 1 with other ones
    bt2 = trainer()
    bt2.step_classifier(other, np.ones(B, np.int32), **kw)
    after2 = state(bt2)
    for k in ("vars", "m", "v", "params"):
        assert np.array_equal(after[k][0].view(np.uint32), after2[k][0].view(np.uint32)), k
        assert not np.array_equal(after[k][1].view(np.uint32), after2[k][1].view(np.uint32)), k
    assert not np.array_equal(after["vars"][1], before["vars"][1]) and np.any(after["m"][1] != 0)   # member 1: trained
    assert out["model_loss"][0] == 0.0 and out["used"] == B
    # the same forward by hand: member 0's weights and its whole gradient row are exactly zero, member 1's weights exactly 1
    be = bt.bank.backend
    loss = be.bank_forward(torch.from_numpy(own).to(be.device), save_for_bwd=True)
    w, _ = be.classify_weights(loss, torch.ones(B, dtype=torch.int32, device=be.device), 1.0 / 3.0, 1.0, 0.0)
    flat = be.bank_backward(weights=w).cpu().numpy()
    wn = w.cpu().numpy()
    assert np.all(wn[0].view(np.uint32) == 0) and np.all(wn[1] == 1.0)
    assert np.all(flat[0] == 0.0) and np.all(np.isfinite(flat[1])) and np.any(flat[1] != 0.0)
    # ... which is the plain reverse pass for member 1, bit for bit
    be.bank_forward(torch.from_numpy(own).to(be.device), save_for_bwd=True)
    plain = be.bank_backward().cpu().numpy()
    assert np.array_equal(flat[1].view(np.uint32), plain[1].view(np.uint32))


def test_train_command_line_discriminative(tmp_path, capsys):
    """train.py --bank_by pitch --bank_objective discriminative on two small TFRecord files: the loop is step_classifier on labelled_batches
    (the same bits as the calls made by hand), it logs xent, judges the held-out file, and bank.json records the objective."""
    import json
    import os
    from audio_mps_amd import tfrecord as tfr, train
    from audio_mps_amd.bank import BankTrainer
    from audio_mps_amd.device_data import ResidentDataset
    data, labels = clips(24, 6)
    held, held_labels = clips(10, 7)
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "guitar.tfrecords"), data, {"pitch": [int(x) for x in labels]})
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "organ.tfrecords"), held, {"pitch": [int(x) for x in held_labels]})
    argv = ["--dataset", "guitar", "--datadir", str(tmp_path), "--sample_duration", str(T), "--max_steps", "3", "--seed", "3", "--device_data",
            "--hparams", f"bond_dim={D},minibatch_size={B}", "--logdir", os.path.join(tmp_path, "log"), "--bank_by", "pitch",
            "--bank_objective", "discriminative", "--gen_weight", "0.25", "--disc_temperature", "4", "--eval_dataset", "organ"]
    tr = train.main(argv)
    out = capsys.readouterr().out
    assert isinstance(tr, BankTrainer) and tr.global_step == 3 and tr.bank.classes == [0, 1]
    steps = [ln for ln in out.splitlines() if ln.startswith("step ")]
    assert len(steps) == 3 and all("xent=" in ln and f"used={B}" in ln for ln in steps), out
    assert sum(ln.startswith("eval step=3 ") for ln in out.splitlines()) == 1
    logdir = os.path.join(tmp_path, "log", "guitar", f"{D}_{1.0 / 16000}_{B}")
    with open(os.path.join(logdir, "bank.json")) as f:
        meta = json.load(f)
    assert meta["objective"] == {"name": "discriminative", "disc_weight": 1.0, "gen_weight": 0.25, "temperature": 4.0}
    # the same three steps by hand (the hyper-parameters train.py sets: train.py:41-43)
    from audio_mps_amd import HParams
    bt = trainer(HParams(delta_t=1.0 / 16000, h_reg=200.0 / (math.pi * 16000) ** 2, minibatch_size=B, bond_dim=D))
    stream = ResidentDataset(data, bt.bank.backend, labels=labels).labelled_batches([0, 1], B, seed=3, order="estimator", crop_seed=3)
    for _ in range(3):
        batch, lab = stream()
        bt.step_classifier(batch, lab, gen_weight=0.25, disc_weight=1.0, temperature=4.0, sync=False)
    a, b = state(tr), state(bt)
    for k in ("vars", "m", "v"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_refusals_on_the_device():
    from audio_mps_amd import HParams
    from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
    from audio_mps_amd.scan import HipScan
    data, labels = clips(B, 5)
    hp = HParams(minibatch_size=B, bond_dim=D)
    with pytest.raises(ValueError, match="class bank"):
        BankTrainer(PsiBank(hp, [{"seed": 1}, {"seed": 2}], backend=HipScan(D))).step_classifier(data, labels)
    rho = RhoBank(HParams(minibatch_size=B, bond_dim=D, initial_rank=3), [{"seed": 1}, {"seed": 2}], backend=HipScan(D), classes=[0, 1])
    rho_bt = BankTrainer(rho)
    with pytest.raises(ValueError, match="RhoBank"):
        rho_bt.step_classifier(data, labels)
    # ... and at the C ABI: a handle that holds a RhoCMPS bank (one generative step has configured it) answers CMPS_ERR_STATE with a message
    from audio_mps_amd import _capi
    rho_bt.step(data)
    be = rho.backend
    audio = torch.from_numpy(data).to(be.device)
    w = torch.ones((M, B), dtype=torch.float32, device=be.device)
    grad = torch.empty((M, 2 * D * D + 3 * D + 2 + 2 * 3 * D), dtype=torch.float32, device=be.device)
    code = be._lib.cmps_bank_loss_bwd_weighted(be._h, audio.data_ptr(), 1, B, T, w.data_ptr(), B, grad.data_ptr(), None)
    msg = be._lib.cmps_last_error(be._h).decode()
    assert code == _capi.CMPS_ERR_STATE and msg.startswith("cmps_bank_loss_bwd_weighted:") and "RhoCMPS" in msg, (code, msg)
    with pytest.raises(RuntimeError, match="bank_forward"):
        be.bank_backward(weights=w)
    bt = trainer()
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        bt.step_classifier(np.stack([data, data]), labels)
    with pytest.raises(ValueError, match="labels"):
        bt.step_classifier(data, labels[:3])
    with pytest.raises(ValueError, match="temperature"):
        bt.step_classifier(data, labels, temperature=0.0)
    assert bt.global_step == 0
