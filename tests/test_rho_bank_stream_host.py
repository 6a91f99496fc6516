"""Host layer of a RhoCMPS bank's streams without a GPU: BankStream over a RhoBank (follow, score, generate, fill_gaps, ranking, best),
RhoBank.open_stream / sample / nll_per_step / classify, BankTrainer.open_stream and `python -m audio_mps_amd.sample --bankdir` on a bank of
rho_mps members, on the stand-in backends of tests/test_rho_stream_host.py and tests/test_rho_score_host.py (imported, not edited).  Two
stand-ins: the plain one, on which a BankStream loops over one plain backend per member (rho_stream / rho_stream_score), and one with
HipScan's rho_bank_* entries, answered per member from the same oracle composition (tests/_rho_stream_ref.py, tests/_rho_score_ref.py)
behind its own expansion of the shared rows to global paths.  The kernel is tested in tests/test_gpu_rho_bank_stream.py."""
import json
import os

import numpy as np
import pytest

from _util import make_audio
from test_rho_score_host import RhoScoreBackend
from test_rho_stream_host import RhoStreamBackend
from test_score_host import ScoreBackend

from audio_mps_amd import HParams
from audio_mps_amd import sample as S
from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
from audio_mps_amd.stream import BankStream

D, RANK, N_PATHS = 4, 3, 2
MEMBERS = [{"seed": 3, "h_reg": 2e-7, "r_reg": 0.1}, {"seed": 4}, {"seed": 5, "r_reg": 1.0}]


class RhoBankBackend(RhoScoreBackend):
    """RhoScoreBackend plus HipScan's rho_bank_set_state / rho_bank_stream_state / rho_bank_stream / rho_bank_stream_score.  Every array
    the members may share is first expanded to one row per global path g = m n + b, as the C ABI numbers them; member m then runs rows
    m n .. m n + n - 1."""

    def __init__(self, D, dtype="f32"):
        super().__init__(D, dtype)
        self.bank_calls = []

    def rho_bank_set_state(self, members, columns, B, T, train=False):
        assert len(members) == len(columns) and all(np.shape(c) == np.shape(columns[0]) for c in columns)
        self.member_be = [RhoScoreBackend(self.D, self.dtype) for _ in members]
        for be, p, phi in zip(self.member_be, members, columns):
            be.set_params(p, B, T, train=False)
            be.rho_set_state(phi, B, T, train=train)
        self.prepared.append(("rho_bank", len(members), B, T, train))

    def rho_bank_stream_state(self, n):
        return [be.rho_stream_state(n) for be in self.member_be]

    def _global(self, rows, n):
        """[1 | n | M n, ...] -> [M, n, ...]"""
        M = len(self.member_be)
        rows = np.asarray(rows, dtype=np.float32)
        assert rows.shape[0] in (1, n, M * n), rows.shape
        reps = M * n // rows.shape[0]
        return np.tile(rows, (reps,) + (1,) * (rows.ndim - 1)).reshape((M, n) + rows.shape[1:])

    def rho_bank_stream(self, state_in, state_out, k0, audio, noise, want_pred=False, n=None):
        self.bank_calls.append(("stream", k0, None if audio is None else np.shape(audio), None if noise is None else np.shape(noise)))
        M = len(self.member_be)
        a = None if audio is None else self._global(audio, n)
        z = None if noise is None else self._global(np.asarray(noise).T, n)          # [M, n, length]
        assert z is None or np.shape(noise)[1] in (n, M * n)
        outs, preds = [], []
        for m, be in enumerate(self.member_be):
            o, p = be.rho_stream(None if state_in is None else state_in[m], None if state_out is None else state_out[m], k0,
                                 None if a is None else a[m], None if z is None else z[m].T, want_pred, n=n)
            outs.append(o)
            preds.append(p)
        return np.stack(outs), (np.stack(preds) if want_pred else None)

    def rho_bank_stream_score(self, state_in, state_out, k0, audio, want_nll=True, want_pred=False, n=None, loss=None):
        self.bank_calls.append(("score", k0, np.shape(audio), None))
        a = self._global(audio, n)
        res = [be.rho_stream_score(None if state_in is None else state_in[m], None if state_out is None else state_out[m], k0, a[m], want_nll,
                                   want_pred, n=n, loss=None if loss is None else np.asarray(loss)[m]) for m, be in enumerate(self.member_be)]
        return (np.stack([r[0] for r in res]) if want_nll else None), np.stack([r[1] for r in res]), \
            (np.stack([r[2] for r in res]) if want_pred else None)


def make_bank(backend_cls=RhoScoreBackend, n=N_PATHS, members=MEMBERS, d=D, rank=RANK):
    bank = RhoBank(HParams(minibatch_size=n, bond_dim=d, sigma=0.1, initial_rank=rank, A=5.0), members, backend=backend_cls(d))
    for m, model in enumerate(bank.models):
        model.variables["Rx"] *= np.float32(0.3)
        model.variables["Ry"] *= np.float32(0.3)
        model.variables["A"] = np.asarray(np.float32(5.0 + m))                        # (trained members differ in A too)
    return bank


def _clip(n, T, seed):
    return make_audio(n, T, HParams().delta_t, seed=seed)


def _session(st, clip, M, n):
    """One of everything, with blocks of every shape: the results, in order."""
    per_member = np.stack([clip + np.float32(0.01 * m) for m in range(M)])            # [M, n, T]
    out = [st.follow(clip[0, :9]),                                                     # [m]: one signal for everybody
           st.score(clip[:, 9:20]),                                                    # [n, m]: shared by the members
           st.generate(7),
           st.generate(5),
           st.follow(per_member[:, :, 20:31], anchor=True),                            # [M, n, m]
           st.score(per_member[:, :, 31:40]),
           st.score(clip[:1, 40:46]),                                                  # [1, m] behind last samples that differ per member
           st.generate(6)]
    return out + [st.last_pred, st.total_nll.copy(), st.last.copy(), np.asarray(st.position)]


def test_open_stream_is_no_longer_refused_and_native_and_looped_agree_exactly():
    M, n, T = len(MEMBERS), N_PATHS, 46
    clip = _clip(n, T, seed=5)
    known = np.ones(30, dtype=bool)
    known[8:15] = known[22:26] = False
    res = {}
    for kind, cls in (("looped", RhoScoreBackend), ("native", RhoBankBackend)):
        bank = make_bank(cls)
        st = bank.open_stream(n, 80, temp=0.5, seed=11)
        assert isinstance(st, BankStream) and st.native == (kind == "native") and len(st) == M
        assert st.total_nll.shape == (M, n) and st.last is None and st.position == 0
        r = _session(st, clip, M, n)
        assert [x.shape for x in r[:8]] == [(M, n, 8), (M, n, 11), (M, n, 7), (M, n, 5), (M, n, 10), (M, n, 9), (M, n, 6), (M, n, 6)]
        assert st.position == 8 + 11 + 7 + 5 + 10 + 9 + 6 + 6 and st.last_pred.shape == (M, n, 6) and st.last.shape == (M, n)
        assert st.ranking().shape == (M, n) and np.array_equal(st.best(), np.argmin(st.total_nll, axis=0))
        gaps = bank.open_stream(n, 40, temp=0.5, seed=3).fill_gaps(clip[:, :30], known)
        assert gaps.shape == (M, n, 30) and np.array_equal(gaps[:, :, known], np.broadcast_to(clip[:, :30][:, known], (M, n, int(known.sum()))))
        res[kind] = r + [gaps, st.ranking(), st.best()]
        if kind == "native":                                                           # the sharing of a block reaches the entry as it is
            shapes = [c[2] for c in st._be.bank_calls if c[2] is not None]
            assert shapes[:2] == [(1, 9), (n, 12)] and (M * n, 11) in shapes and shapes[-1] == (M * n, 7)
            assert st._be.prepared[-1] == ("rho_bank", M, n, 81, False)
            assert all(be.phi.shape == (RANK, D) for be in st._be.member_be)            # every member's columns went with its parameters
        # the stream runs on a backend of its own and leaves the bank's alone
        assert st._be is not bank.backend and bank.backend.prepared == []
    for a, b in zip(res["looped"], res["native"]):
        assert np.array_equal(a, b)
    nll = res["native"][1]
    assert not np.array_equal(nll[0], nll[1]) and np.all(np.isfinite(res["native"][9])) and np.all(res["native"][9] != 0)


@pytest.mark.parametrize("cls", [RhoScoreBackend, RhoBankBackend])
def test_member_m_is_the_members_own_stream_of_the_same_seed(cls):
    M, n, T = len(MEMBERS), N_PATHS, 46
    clip = _clip(n, T, seed=6)
    known = np.ones(30, dtype=bool)
    known[10:17] = False
    bank = make_bank(cls)
    got = _session(bank.open_stream(n, 80, temp=0.5, seed=11), clip, M, n)
    gaps = bank.open_stream(n, 40, temp=0.5, seed=3).fill_gaps(clip[:, :30], known)
    for m in range(M):
        st = bank.models[m].open_stream(n, 80, temp=0.5, seed=11)
        c = clip + np.float32(0.01 * m)
        want = [st.follow(clip[0, :9]), st.score(clip[:, 9:20]), st.generate(7), st.generate(5), st.follow(c[:, 20:31], anchor=True),
                st.score(c[:, 31:40]), st.score(clip[:1, 40:46]), st.generate(6), st.last_pred, st.total_nll, st.last]
        for a, b in zip(got, want):
            assert np.array_equal(a[m], b), m
        assert np.array_equal(gaps[m], bank.models[m].open_stream(n, 40, temp=0.5, seed=3).fill_gaps(clip[:, :30], known)), m


@pytest.mark.parametrize("cls", [RhoScoreBackend, RhoBankBackend])
def test_independent_noise_numbers_the_paths_globally(cls):
    M, n, L, seed = len(MEMBERS), N_PATHS, 12, 21
    bank = make_bank(cls, members=[{"seed": 7}] * M)                                   # the same model three times: only the draw differs
    for model in bank.models:
        model.variables["A"] = np.asarray(np.float32(5.0))
    shared = bank.open_stream(n, L, temp=0.5, seed=seed).generate(L)
    own = bank.open_stream(n, L, temp=0.5, seed=seed, independent_noise=True).generate(L)
    assert np.array_equal(shared[0], shared[1]) and np.array_equal(shared[0], shared[2])
    assert not np.array_equal(own[0], own[1]) and not np.array_equal(own[1], own[2])
    m0 = bank.models[0]
    std = float(m0.sigma) * np.sqrt(0.5 * float(m0.delta_t))
    noise = (std * np.random.default_rng(seed).standard_normal((L, M * n))).astype(np.float32)   # one draw, column g = m n + b
    for m in range(M):
        want = bank.models[m].open_stream(n, L, temp=0.5, seed=0).generate(L, noise=noise[:, m * n:(m + 1) * n])
        assert np.array_equal(own[m], want), m
    st = bank.open_stream(n, L, independent_noise=True)
    with pytest.raises(ValueError, match=f"{M * n}"):
        st.generate(4, noise=np.zeros((4, n), np.float32))
    assert np.array_equal(st.generate(L, noise=noise), own)


@pytest.mark.parametrize("cls", [RhoScoreBackend, RhoBankBackend])
def test_sample_nll_per_step_and_classify(cls):
    M, n, L, T = len(MEMBERS), 3, 10, 17
    bank = make_bank(cls, n=n)
    out = bank.sample(n, L, temp=0.5, seed=4)
    assert out.shape == (M, n, L) and out.dtype == np.float32
    prime = _clip(1, 6, seed=2)[0]
    cont = bank.sample(n, L, temp=0.5, seed=4, prime=prime)
    assert cont.shape == (M, n, L)
    for m in range(M):                                                                 # the reference's convention, as RhoCMPS.sample
        assert np.array_equal(out[m], bank.models[m].sample(n, L, temp=0.5, seed=4))
        assert np.array_equal(cont[m], bank.models[m].sample(n, L, temp=0.5, seed=4, prime=prime))
    with pytest.raises(ValueError, match="prime must be"):
        bank.sample(n, L, prime=np.zeros((2, 6), np.float32))                          # RhoCMPS._prime's own rules
    clips = _clip(n, T, seed=3)
    nll = bank.nll_per_step(clips)
    assert nll.shape == (M, n, T - 1) and np.array_equal(nll, bank.nll_per_step(clips, segment=5))
    for m in range(M):
        assert np.array_equal(nll[m], bank.models[m].nll_per_step(clips))
    best, total = bank.classify(clips)
    assert best.shape == (n,) and total.shape == (M, n) and np.array_equal(best, np.argmin(total, axis=0))
    assert np.allclose(total, nll.astype(np.float64).sum(axis=-1), rtol=1e-5, atol=0)  # (float32 fold against a float64 sum of 16 terms)
    with pytest.raises(ValueError):
        bank.classify(np.zeros((n, 1), np.float32))


def test_refusals_come_before_anything_runs():
    bank = make_bank(RhoBankBackend)
    st = bank.open_stream(N_PATHS, 10, seed=0)
    be = st._be
    st.follow(_clip(N_PATHS, 8, seed=1))
    calls, pos = len(be.bank_calls), st.position
    with pytest.raises(ValueError, match="max_steps=10"):
        st.generate(4)
    with pytest.raises(ValueError, match="max_steps=10"):
        st.score(_clip(N_PATHS, 4, seed=2))
    for bad in (np.zeros((3, 5), np.float32), np.zeros((len(MEMBERS), 1, 5), np.float32), np.zeros((2, 2, 2, 2), np.float32)):
        with pytest.raises(ValueError, match="a block must be"):
            st.follow(bad)
    assert len(be.bank_calls) == calls and st.position == pos
    with pytest.raises(ValueError, match="draws noise on the device"):
        bank.open_stream(N_PATHS, 10, device_noise=True)
    # a backend that streams RhoCMPS but cannot score it: the loop follows and generates, and scoring says so before anything runs
    loop = make_bank(RhoStreamBackend)
    st = loop.open_stream(N_PATHS, 20, seed=0)
    assert not st.native and st.follow(_clip(N_PATHS, 6, seed=1)).shape == (len(MEMBERS), N_PATHS, 5)
    launches = [b.launches for b in st._be.backends]
    with pytest.raises(ValueError, match="rho_stream_score"):
        st.score(_clip(N_PATHS, 4, seed=2))
    assert [b.launches for b in st._be.backends] == launches and st.position == 5 and not st.total_nll.any()
    with pytest.raises(ValueError, match="PsiCMPS-only"):
        loop.nll_per_step(_clip(N_PATHS, 6, seed=1))
    # a backend with neither rho_bank_stream nor rho_stream
    psi_only = RhoBank(HParams(minibatch_size=2, bond_dim=D, initial_rank=RANK), [{"seed": 1}, {"seed": 2}], backend=ScoreBackend(D))
    for call in (lambda: psi_only.open_stream(2, 10), lambda: BankTrainer(psi_only).open_stream(2, 10), lambda: psi_only.sample(2, 5),
                 lambda: psi_only.classify(np.zeros((2, 5), np.float32))):
        with pytest.raises(ValueError, match="neither rho_bank_stream nor rho_stream"):
            call()
    assert psi_only.backend.prepared == []


def test_a_stream_keeps_the_parameters_it_was_opened_with_and_a_trainer_hands_over_its_own():
    n, T = N_PATHS, 24
    bank = make_bank(RhoScoreBackend)
    bt = BankTrainer(bank)
    audio = _clip(n, T, seed=9)
    bt.step(audio)
    st = bt.open_stream(n, 30, seed=1)
    want = [bt.member(m).open_stream(n, 30, seed=1).score(audio) for m in range(len(bank))]
    bt.step(audio)                                                                     # (the members move on; the stream does not)
    assert np.array_equal(st.score(audio), np.stack(want))
    assert not np.array_equal(bt.open_stream(n, 30, seed=1).score(audio), np.stack(want))


def test_the_command_line_on_a_saved_rho_bank(tmp_path, capsys):
    n, T = 2, 24
    hp = S.HParams(delta_t=1.0 / 16000, h_reg=200.0 / (np.pi * 16000) ** 2, minibatch_size=n, bond_dim=D, initial_rank=RANK)   # what sample.main assumes
    bank = RhoBank(hp, MEMBERS, backend=RhoScoreBackend(D))
    bt = BankTrainer(bank)
    bt.step(make_audio(n, T, hp.delta_t, seed=1))
    d, out = str(tmp_path / "bank"), str(tmp_path / "out")
    bt.save(d)
    with open(os.path.join(d, "bank.json")) as f:
        assert json.load(f)["model"] == "rho_mps"
    M = len(MEMBERS)
    loaded = S.load_bank(d, 16000, backend=RhoScoreBackend(D))
    assert isinstance(loaded, RhoBank) and loaded.rank == RANK and loaded.bond_d == D and len(loaded) == M
    for m in range(M):
        for k, v in bt.member(m).variables.items():
            assert np.array_equal(loaded.models[m].variables[k], v), (m, k)
    waves = S.main(["--bankdir", d, "--out_dir", out, "--num_samples", "2", "--sample_duration", "20", "--temp", "0.5", "--seed", "3"],
                   backend=RhoScoreBackend(D))
    assert waves.shape == (M, 2, 20) and np.array_equal(np.load(os.path.join(out, "samples.npy")), waves)
    assert sorted(f for f in os.listdir(out) if f.endswith(".wav")) == sorted(f"sample_m{m}_{i}.wav" for m in range(M) for i in range(2))
    for m in range(M):                                                                 # member m's files are what --modeldir gives for its checkpoint
        one = S.main(["--modeldir", BankTrainer.member_path(d, m), "--hparams", ",".join(f"{k}={v}" for k, v in MEMBERS[m].items() if k != "seed"),
                      "--out_dir", str(tmp_path / f"one{m}"), "--num_samples", "2", "--sample_duration", "20", "--temp", "0.5", "--seed", "3"],
                     backend=RhoScoreBackend(D))
        assert np.array_equal(waves[m], one), m
    native = S.main(["--bankdir", d, "--out_dir", out, "--num_samples", "2", "--sample_duration", "20", "--temp", "0.5", "--seed", "3"],
                    backend=RhoBankBackend(D))
    assert np.array_equal(native, waves)
    cut = S.main(["--bankdir", d, "--out_dir", out, "--num_samples", "2", "--sample_duration", "20", "--temp", "0.5", "--seed", "3", "--segment", "7"],
                 backend=RhoScoreBackend(D))
    assert cut.shape == waves.shape and np.allclose(cut, waves, rtol=0, atol=1e-6)     # (the stand-in's time table per segment: rounding)
    clip_path = str(tmp_path / "clip.npy")
    np.save(clip_path, make_audio(1, 15, hp.delta_t, seed=4)[0])
    cont = S.main(["--bankdir", d, "--out_dir", out, "--num_samples", "2", "--sample_duration", "9", "--prime", clip_path],
                  backend=RhoScoreBackend(D))
    assert cont.shape == (M, 2, 15 + 9) and np.array_equal(cont[:, :, :15], np.broadcast_to(np.load(clip_path), (M, 2, 15)))
    capsys.readouterr()
    nll = S.main(["--bankdir", d, "--out_dir", out, "--score", clip_path, "--segment", "5"], backend=RhoScoreBackend(D))
    text = capsys.readouterr().out
    assert nll.shape == (M, 14) and np.array_equal(np.load(os.path.join(out, "nll.npy")), nll)
    assert np.load(os.path.join(out, "pred.npy")).shape == (M, 14)
    lines = text.strip().splitlines()
    assert len(lines) == M + 1 and all(lines[m].startswith(f"member {m}: total nll") and str(MEMBERS[m]["seed"]) in lines[m] for m in range(M))
    best = int(np.argmin(nll.astype(np.float64).sum(axis=1)))
    assert lines[-1].startswith(f"best member {best} of {M}")
    # what the command line refuses: a backend that streams no RhoCMPS, and a rho_mps bank.json over PsiCMPS checkpoints
    with pytest.raises(ValueError, match="rho_mps"):
        S.main(["--bankdir", d, "--out_dir", out], backend=ScoreBackend(D))
    psi = BankTrainer(PsiBank(S.HParams(minibatch_size=n, bond_dim=D), MEMBERS, backend=ScoreBackend(D)))
    pd = str(tmp_path / "psi")
    psi.save(pd)
    with open(os.path.join(pd, "bank.json")) as f:
        meta = json.load(f)
    meta["model"] = "rho_mps"
    with open(os.path.join(pd, "bank.json"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match="rho_mps"):
        S.main(["--bankdir", pd, "--out_dir", out], backend=RhoScoreBackend(D))
