"""The host side of a RhoCMPS bank (audio_mps_amd/bank.py::RhoBank) without a GPU: on a backend without the rho_bank_* entries
BankTrainer loops over plain steps of its members, which by the bank's contract give the numbers of M plain Trainers; checkpoints."""
import json
import os

import numpy as np
import pytest

from audio_mps_amd import HParams, RhoCMPS
from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
from audio_mps_amd.train import Trainer

from _util import OracleBackend, make_audio

D, RANK, B, T = 4, 3, 2, 24
MEMBERS = [{"seed": 3, "learning_rate": 1e-3, "h_reg": 2e-7, "r_reg": 0.1},
           {"seed": 4, "learning_rate": 3e-3},
           {"seed": 5, "r_reg": 1.0}]


def hparams(rank=RANK):
    return HParams(minibatch_size=B, bond_dim=D, initial_rank=rank)


def make_bank():
    return RhoBank(hparams(), MEMBERS, backend=OracleBackend(D))


def test_members_are_plain_rho_models_of_their_seed_and_overrides():
    bank = make_bank()
    assert len(bank) == 3 and bank.seeds == [3, 4, 5] and bank.rank == RANK and bank.MODEL_NAME == "rho_mps"
    for m, ov in enumerate(MEMBERS):
        hp = bank.member_hparams[m]
        ref = RhoCMPS(hp, seed=ov["seed"], backend=OracleBackend(D))
        assert isinstance(bank.models[m], RhoCMPS) and bank.models[m].rank_rho_0 == RANK
        assert hp.learning_rate == ov.get("learning_rate", hparams().learning_rate) and hp.r_reg == ov.get("r_reg", hparams().r_reg)
        assert set(ref.variables) == {"A", "Rx", "Ry", "freqs", "Wx", "Wy"}
        for k, v in ref.variables.items():
            assert np.array_equal(bank.models[m].variables[k], v), (m, k)
    assert RhoBank(hparams(rank=None), MEMBERS[:1], backend=OracleBackend(D)).rank == D          # initial_rank None: bond_dim


@pytest.mark.parametrize("key", ["bond_dim", "initial_rank", "sigma", "minibatch_size"])
def test_unknown_member_keys_raise_naming_the_key(key):
    with pytest.raises(ValueError, match=key):
        RhoBank(hparams(), [{"seed": 1}, {key: 3}], backend=OracleBackend(D))
    with pytest.raises(ValueError):
        RhoBank(hparams(), [], backend=OracleBackend(D))


@pytest.mark.parametrize("shared", [True, False])
def test_two_steps_equal_M_plain_trainers(shared):
    bank = make_bank()
    bt = BankTrainer(bank)
    assert not bt.native and bt.rank == RANK               # the stand-in has no rho_bank entries: plain steps of the members
    plain = [Trainer(RhoCMPS(hp, seed=s, backend=OracleBackend(D)), hp) for hp, s in zip(bank.member_hparams, bank.seeds)]
    M = len(plain)
    for step in range(2):
        audio = np.stack([make_audio(B, T, hparams().delta_t, seed=20 + step * 7 + (0 if shared else m)) for m in range(M)])
        out = bt.step(audio[0] if shared else audio)
        assert out["global_step"] == step + 1 and out["model_loss"].shape == (M,)
        for m, tr in enumerate(plain):
            ref = tr.step(audio[m])
            assert np.float32(ref["model_loss"]) == out["model_loss"][m] and np.float32(ref["total_loss"]) == out["total_loss"][m]
            for k, v in tr.model.variables.items():
                assert np.array_equal(bt.member(m).variables[k], v), (step, m, k)
    assert bt.best() == int(np.argmin(bt.last["model_loss"]))
    assert isinstance(bt.member(bt.best()), RhoCMPS)


def test_save_restore_round_trip_and_the_other_kind_is_refused(tmp_path):
    bt = BankTrainer(make_bank())
    audio = make_audio(B, T, hparams().delta_t, seed=1)
    bt.step(audio)
    bt.step(audio)
    d = str(tmp_path / "bank")
    bt.save(d)
    assert sorted(os.listdir(d)) == ["bank.json", "model.0.ckpt.npz", "model.1.ckpt.npz", "model.2.ckpt.npz"]
    with open(os.path.join(d, "bank.json")) as f:
        meta = json.load(f)
    assert meta == {"members": MEMBERS, "adam_step": 2, "global_step": 2, "model": "rho_mps"}
    # a member's file is what Trainer.save writes for that RhoCMPS model
    with np.load(BankTrainer.member_path(d, 1)) as z:
        assert {"model/Wx", "model/Wy", "model/Rx", "global_step"} <= set(z.files) and "model/psi_x" not in z.files
        assert np.array_equal(z["model/Wx"], bt.member(1).variables["Wx"])
    fresh = BankTrainer(make_bank())
    assert fresh.restore(d) and fresh.global_step == 2
    for m in range(3):
        for k, v in bt.member(m).variables.items():
            assert np.array_equal(fresh.member(m).variables[k], v)
        assert fresh.trainers[m].opt.t == 2
    a, b = bt.step(audio), fresh.step(audio)
    assert np.array_equal(a["model_loss"], b["model_loss"]) and np.array_equal(a["total_loss"], b["total_loss"])
    # a directory of the other kind
    psi = BankTrainer(PsiBank(hparams(), MEMBERS, backend=OracleBackend(D)))
    with pytest.raises(ValueError, match="rho_mps"):
        psi.restore(d)
    psi.step(audio)
    dp = str(tmp_path / "psi")
    psi.save(dp)
    with open(os.path.join(dp, "bank.json")) as f:
        assert "model" not in json.load(f)                 # a PsiCMPS bank's file stays as it was
    with pytest.raises(ValueError, match="psi_mps"):
        BankTrainer(make_bank()).restore(dp)


def test_train_main_refuses_a_rho_bank_on_a_backend_without_the_entries(tmp_path):
    from audio_mps_amd.train import main
    argv = ["--dataset", "damped_sine", "--hparams", f"bond_dim={D},minibatch_size={B},initial_rank={RANK}", "--sample_duration", "32", "--max_steps", "1",
            "--logdir", str(tmp_path), "--bank", "2", "--mps_model", "rho_mps"]
    with pytest.raises(ValueError, match="cmps_rho_bank"):
        main(argv, backend=OracleBackend(D))
