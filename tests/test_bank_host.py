"""The host side of the model bank (audio_mps_amd/bank.py) without a GPU: on a backend without the bank entries BankTrainer loops over
plain steps of its members, which by the bank's contract give the numbers of M plain Trainers; checkpoints, the command line."""
import json
import os

import numpy as np
import pytest

from audio_mps_amd import HParams, PsiCMPS
from audio_mps_amd.bank import BankTrainer, PsiBank, bank_members, parse_bank_hparams
from audio_mps_amd.train import Trainer, bank_log_line, build_parser

from _util import OracleBackend, make_audio

D, B, T = 4, 2, 24
MEMBERS = [{"seed": 3, "learning_rate": 1e-3, "h_reg": 2e-7, "r_reg": 0.1},
           {"seed": 4, "learning_rate": 3e-3},
           {"seed": 5, "r_reg": 1.0}]


def hparams():
    return HParams(minibatch_size=B, bond_dim=D)


def make_bank():
    return PsiBank(hparams(), MEMBERS, backend=OracleBackend(D))


def test_members_are_plain_models_of_their_seed_and_overrides():
    bank = make_bank()
    assert len(bank) == 3 and bank.seeds == [3, 4, 5]
    for m, ov in enumerate(MEMBERS):
        hp = bank.member_hparams[m]
        ref = PsiCMPS(hp, seed=ov["seed"], backend=OracleBackend(D))
        assert hp.learning_rate == ov.get("learning_rate", hparams().learning_rate) and hp.r_reg == ov.get("r_reg", hparams().r_reg)
        for k, v in ref.variables.items():
            assert np.array_equal(bank.models[m].variables[k], v), (m, k)
        assert bank.models[m]._c_r == ref._c_r and bank.models[m]._c_h == ref._c_h


@pytest.mark.parametrize("key", ["bond_dim", "sigma", "minibatch_size", "delta_t", "A", "lr"])
def test_unknown_member_keys_raise_naming_the_key(key):
    with pytest.raises(ValueError, match=key):
        PsiBank(hparams(), [{"seed": 1}, {key: 3}], backend=OracleBackend(D))
    with pytest.raises(ValueError):
        PsiBank(hparams(), [], backend=OracleBackend(D))


def test_more_than_one_rank_is_refused():
    class TwoRanks:
        world_size = 2
    with pytest.raises(ValueError, match="world size"):
        BankTrainer(make_bank(), TwoRanks())


@pytest.mark.parametrize("shared", [True, False])
def test_three_steps_equal_M_plain_trainers(shared):
    bank = make_bank()
    bt = BankTrainer(bank)
    assert not bt.native                                   # the stand-in has no bank entries: plain steps of the members
    plain = [Trainer(PsiCMPS(hp, seed=s, backend=OracleBackend(D)), hp) for hp, s in zip(bank.member_hparams, bank.seeds)]
    M = len(plain)
    for step in range(3):
        audio = np.stack([make_audio(B, T, hparams().delta_t, seed=20 + step * 7 + (0 if shared else m)) for m in range(M)])
        out = bt.step(audio[0] if shared else audio)
        assert out["global_step"] == step + 1 and out["model_loss"].shape == (M,) and out["total_loss"].shape == (M,)
        for m, tr in enumerate(plain):
            ref = tr.step(audio[m])
            assert np.float32(ref["model_loss"]) == out["model_loss"][m] and np.float32(ref["total_loss"]) == out["total_loss"][m]
            for k, v in tr.model.variables.items():
                assert np.array_equal(bt.member(m).variables[k], v), (step, m, k)
    assert bt.best() == int(np.argmin(bt.last["model_loss"]))
    dev = bt.step(audio[0], sync=False)
    assert dev["losses_dev"].shape == (M, 2) and "model_loss" not in dev
    with pytest.raises(ValueError):
        bt.step(np.zeros((M + 1, B, T), np.float32))
    with pytest.raises(ValueError):
        bt.step(np.zeros(T, np.float32))


def test_best_skips_non_finite_members():
    bt = BankTrainer(make_bank())
    with pytest.raises(RuntimeError):
        bt.best()
    bt.last = {"model_loss": np.array([np.nan, 2.0, 1.5], np.float32)}
    assert bt.best() == 2
    bt.last = {"model_loss": np.array([np.nan, np.inf, np.nan], np.float32)}
    with pytest.raises(RuntimeError):
        bt.best()
    line = bank_log_line({"global_step": 7, "model_loss": np.array([np.nan, 2.0, 1.5, 3.0], np.float32)})
    assert line.startswith("step 7:") and "best 1.500000 (member 2)" in line and "median 2.000000" in line and "worst 3.000000" in line
    assert line.endswith("nonfinite 1")


def test_save_restore_member_and_the_sample_and_evaluate_loaders(tmp_path):
    from audio_mps_amd.sample import build_model, load_variables
    bt = BankTrainer(make_bank())
    audio = make_audio(B, T, hparams().delta_t, seed=1)
    bt.step(audio)
    bt.step(audio)
    d = str(tmp_path / "bank")
    bt.save(d)
    assert sorted(os.listdir(d)) == ["bank.json", "model.0.ckpt.npz", "model.1.ckpt.npz", "model.2.ckpt.npz"]
    with open(os.path.join(d, "bank.json")) as f:
        meta = json.load(f)
    assert meta["members"] == MEMBERS and meta["adam_step"] == 2 and meta["global_step"] == 2
    fresh = BankTrainer(make_bank())
    assert not fresh.restore(str(tmp_path / "nothing"))
    assert fresh.restore(d) and fresh.global_step == 2
    for m in range(3):
        for k, v in bt.member(m).variables.items():
            assert np.array_equal(fresh.member(m).variables[k], v)
        assert fresh.trainers[m].opt.t == 2
        for k, v in bt.trainers[m].opt.m.items():
            assert np.array_equal(fresh.trainers[m].opt.m[k], v)
        # one member's file is an ordinary checkpoint: what python -m audio_mps_amd.sample / .evaluate load
        variables = load_variables(BankTrainer.member_path(d, m))
        model = build_model(variables, 16000, "", 0, 0, OracleBackend(D))
        assert isinstance(model, PsiCMPS) and model.bond_d == D
        for k, v in bt.member(m).variables.items():
            assert np.array_equal(model.variables[k], v)
    # the restored bank goes on exactly as the saved one
    a, b = bt.step(audio), fresh.step(audio)
    assert np.array_equal(a["model_loss"], b["model_loss"]) and np.array_equal(a["total_loss"], b["total_loss"])
    other = BankTrainer(PsiBank(hparams(), MEMBERS[:2] + [{"seed": 9}], backend=OracleBackend(D)))
    with pytest.raises(ValueError, match="other members"):
        other.restore(d)


def test_bank_flags_parse_and_the_grid_order():
    args = build_parser().parse_args([])
    assert args.bank == 0 and args.bank_hparams == ""
    args = build_parser().parse_args(["--bank", "3", "--seed", "5", "--bank_hparams", "learning_rate=1e-3,3e-3;r_reg=0.1,1"])
    assert args.bank == 3 and args.bank_hparams == "learning_rate=1e-3,3e-3;r_reg=0.1,1"
    grid = parse_bank_hparams(args.bank_hparams)
    assert grid == [{"learning_rate": 1e-3, "r_reg": 0.1}, {"learning_rate": 1e-3, "r_reg": 1.0},
                    {"learning_rate": 3e-3, "r_reg": 0.1}, {"learning_rate": 3e-3, "r_reg": 1.0}]
    assert parse_bank_hparams("") == [{}] and parse_bank_hparams("h_reg=1e-7;") == [{"h_reg": 1e-7}]
    assert bank_members(5, 3, "") == [{"seed": 5}, {"seed": 6}, {"seed": 7}]
    assert bank_members(5, 0, "r_reg=0.1,1") == [{"r_reg": 0.1, "seed": 5}, {"r_reg": 1.0, "seed": 5}]
    both = bank_members(5, 2, "r_reg=0.1,1")
    assert both == [{"r_reg": 0.1, "seed": 5}, {"r_reg": 0.1, "seed": 6}, {"r_reg": 1.0, "seed": 5}, {"r_reg": 1.0, "seed": 6}]
    for bad in ("bond_dim=4,8", "seed=1,2", "sigma=1", "r_reg="):
        with pytest.raises(ValueError):
            parse_bank_hparams(bad)


def test_train_main_with_a_bank(tmp_path, capsys):
    from audio_mps_amd.train import main
    argv = ["--dataset", "damped_sine", "--sample_duration", str(T), "--hparams", f"bond_dim={D},minibatch_size={B}", "--max_steps", "2",
            "--logdir", str(tmp_path), "--bank", "2", "--bank_hparams", "learning_rate=1e-3,3e-3", "--seed", "1"]
    trainer = main(argv, backend=OracleBackend(D))
    assert isinstance(trainer, BankTrainer) and len(trainer) == 4 and trainer.global_step == 2
    assert trainer.bank.overrides == [{"learning_rate": 1e-3, "seed": 1}, {"learning_rate": 1e-3, "seed": 2},
                                      {"learning_rate": 3e-3, "seed": 1}, {"learning_rate": 3e-3, "seed": 2}]
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 2 and all("members 4 best" in ln and "median" in ln and "worst" in ln and ln.endswith("nonfinite 0") for ln in lines)
    logdir = next(p for p, _, files in os.walk(tmp_path) if "bank.json" in files)
    assert sorted(f for f in os.listdir(logdir) if f.startswith("model.")) == [f"model.{m}.ckpt.npz" for m in range(4)]
    again = main(argv, backend=OracleBackend(D))                 # restores and continues
    assert again.global_step == 4
    with pytest.raises(ValueError):
        main(argv + ["--mps_model", "rho_mps"], backend=OracleBackend(D))


@pytest.mark.parametrize("extra, match", [(["--eval_dataset", "damped_sine"], "--eval_dataset"), (["--eval_every", "5"], "--eval_every"),
                                          (["--eval_minibatch", "4"], "--eval_minibatch"), (["--host_optimizer"], "--host_optimizer")])
def test_train_main_refuses_what_a_bank_run_does_not_do(tmp_path, extra, match):
    """Flags the bank loop would ignore are refused before anything is built or written."""
    from audio_mps_amd.train import main
    argv = ["--dataset", "damped_sine", "--sample_duration", str(T), "--hparams", f"bond_dim={D},minibatch_size={B}", "--max_steps", "1",
            "--logdir", str(tmp_path), "--bank", "2"]
    with pytest.raises(ValueError, match=match):
        main(argv + extra, backend=OracleBackend(D))
    assert not os.listdir(tmp_path)


def test_a_negative_bank_is_refused_and_zero_means_one_seed_per_grid_point(tmp_path):
    from audio_mps_amd.train import main
    argv = ["--dataset", "damped_sine", "--sample_duration", str(T), "--hparams", f"bond_dim={D},minibatch_size={B}", "--max_steps", "1",
            "--logdir", str(tmp_path)]
    with pytest.raises(ValueError, match="negative"):
        main(argv + ["--bank", "-1"], backend=OracleBackend(D))
    trainer = main(argv + ["--bank", "0", "--bank_hparams", "r_reg=0.1,1"], backend=OracleBackend(D))
    assert len(trainer) == 2 and trainer.bank.seeds == [0, 0]
