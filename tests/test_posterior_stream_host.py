"""Host layer of the streaming classifier without a GPU: BankStream.score_posterior (its bookkeeping against `score` on a twin stream, the
decision carried across calls, prior / temperature / threshold), the refusal on a backend without the entry, PsiBank.posterior_trace, and
the two command lines (`sample --bankdir --score --posterior`, `evaluate --bankdir --listen`), on stand-in backends whose
`bank_stream_posterior` is the restatement of tests/_posterior_ref.py over the stand-in's own scored segment.  The kernel is tested in
tests/test_gpu_posterior.py, the real backends in tests/test_gpu_stream_posterior.py."""
import json
import os

import numpy as np
import pytest

import _eval_ref as ER
import _posterior_ref as PR
from _util import make_audio
from test_bank_stream_host import D, MEMBERS, N_PATHS, BankBackend, _clip, make_bank
from test_score_host import ScoreBackend

from audio_mps_amd import HParams
from audio_mps_amd import evaluate as EV
from audio_mps_amd import sample as S
from audio_mps_amd.bank import BankTrainer, PsiBank
from audio_mps_amd.stream import PosteriorTrace, log_prior_of


class PosteriorBackend(PR.PosteriorEntries, ER.EvalMethods, BankBackend):
    def __init__(self, D, dtype="f32"):
        super().__init__(D, dtype)
        self._eval_init()


CUTS = (1, 17, 22)


def _run(st, clip, how):
    """The clip through the stream in cuts of 1 + 17 + 22 steps by `how` (a method name): the results in order."""
    out, a = [], 0
    for i, c in enumerate(CUTS):
        out.append(getattr(st, how)(clip[:, a:a + c + (i == 0)]))
        a += c + (i == 0)
    return out


def test_score_posterior_keeps_the_books_of_score():
    M, n, T = len(MEMBERS), N_PATHS, 41
    clip = _clip(n, T, seed=5)
    prior = [0.5, 0.2, 0.3]
    twin = make_bank(PosteriorBackend).open_stream(n, 60, seed=3)
    st = make_bank(PosteriorBackend).open_stream(n, 60, seed=3, prior=prior, temperature=2.0, threshold=0.4)
    assert np.array_equal(st.decided_at, [-1, -1]) and np.array_equal(st.decided_as, [-1, -1]) and st.decided_at.dtype == np.int64
    nll = _run(twin, clip, "score")
    preds, traces, pos = [], [], 0
    for i, c in enumerate(CUTS):
        tr = st.score_posterior(clip[:, pos:pos + c + (i == 0)], want_nll=(i == 1), want_post=(i != 1))
        pos += c + (i == 0)
        assert isinstance(tr, PosteriorTrace) and tr.best.shape == (n, c) and tr.conf.shape == (n, c) and tr.best.dtype == np.int32
        assert (tr.nll is not None) == (i == 1) and (tr.post is not None) == (i != 1)
        if i == 1:
            assert np.array_equal(tr.nll, nll[1])
        preds.append(st.last_pred)
        traces.append(tr)
    assert np.array_equal(st.total_nll, twin.total_nll) and st.total_nll.dtype == np.float32
    assert np.array_equal(st.last_pred, twin.last_pred) and np.array_equal(st.last, twin.last) and st.position == twin.position == 40
    assert all(p.shape == (M, n, c) for p, c in zip(preds, CUTS))
    assert np.array_equal(st.generate(6), twin.generate(6))                           # the state is score's: what follows is the same
    # against the restatement on the twin's nll, whole: a cut changes nothing, and the decision is carried across the cuts
    ref = PR.posterior(np.concatenate(nll, axis=-1), log_prior=log_prior_of(prior, M), inv_temp=0.5, threshold=0.4)
    assert np.array_equal(np.concatenate([t.best for t in traces], axis=1), ref["best"])
    assert np.array_equal(np.concatenate([t.conf for t in traces], axis=1), ref["conf"])
    assert np.array_equal(traces[2].post, ref["post"][:, :, 18:])
    assert np.array_equal(st.decided_at, ref["decision"]["step"]) and np.array_equal(st.decided_as, ref["decision"]["member"])
    assert np.all(st.decided_at >= 0) and np.array_equal(traces[-1].decided_at, st.decided_at)
    assert np.array_equal(st.total_nll, ref["total_out"])
    calls = st._be.posterior_calls
    assert [c[0] for c in calls] == [0, 1, 18] and [c[3:] for c in calls] == [(True, False, "lazy"), (False, True, "lazy"), (True, False, "lazy")]
    # the defaults: a uniform prior at temperature 1 and no decision; `best` at the end is the arg-min of the totals
    plain = make_bank(PosteriorBackend).open_stream(n, 60)
    tr = plain.score_posterior(clip)
    assert np.array_equal(tr.best[:, -1], plain.best()) and np.all(tr.decided_at == -1) and plain._decision is None
    assert np.array_equal(tr.best, PR.posterior(np.concatenate(nll, axis=-1))["best"])
    # an anchor alone makes no step and returns an empty trace; `score` and `score_posterior` alternate
    st2 = make_bank(PosteriorBackend).open_stream(n, 60, threshold=0.9)
    empty = st2.score_posterior(clip[:, :1])
    assert empty.best.shape == (n, 0) and st2.position == 0 and st2.last_pred.shape == (M, n, 0)
    a = st2.score(clip[:, 1:10])
    b = st2.score_posterior(clip[:, 10:20], want_nll=True)
    assert np.array_equal(np.concatenate([a, b.nll], axis=-1), np.concatenate(nll, axis=-1)[:, :, :19])


def test_refusals():
    bank = make_bank(BankBackend)                                                      # the bank entries, but no bank_stream_posterior
    st = bank.open_stream(N_PATHS, 10, threshold=0.9)
    with pytest.raises(ValueError, match="bank_stream_posterior") as e:
        st.score_posterior(_clip(N_PATHS, 5, seed=1))
    assert "BankBackend" in str(e.value) and st.position == 0
    looped = make_bank(ScoreBackend).open_stream(N_PATHS, 10)                          # a loop over plain members: the same refusal
    with pytest.raises(ValueError, match="ScoreBackend"):
        looped.score_posterior(_clip(N_PATHS, 5, seed=1))
    assert looped.score(_clip(N_PATHS, 5, seed=1)).shape == (len(MEMBERS), N_PATHS, 4)  # ... and `score` is untouched
    ok = make_bank(PosteriorBackend)
    for kw, match in ((dict(prior=[1, 2]), "prior"), (dict(prior=[1, -1, 1]), "prior"), (dict(prior=[0, 0, 0]), "prior"),
                      (dict(prior=[1, float("nan"), 1]), "prior"), (dict(temperature=0.0), "temperature"),
                      (dict(temperature=float("inf")), "temperature"), (dict(threshold=0.0), "threshold"), (dict(threshold=1.5), "threshold")):
        with pytest.raises(ValueError, match=match):
            ok.open_stream(N_PATHS, 10, **kw)
    st = ok.open_stream(N_PATHS, 10, threshold=0.9)
    with pytest.raises(ValueError, match="max_steps=10"):
        st.score_posterior(_clip(N_PATHS, 12, seed=1))
    assert st.position == 0 and not getattr(st._be, "posterior_calls", [])
    assert np.array_equal(log_prior_of([2, 0, 6], 3), [np.log(0.25), -np.inf, np.log(0.75)]) and log_prior_of(None, 3) is None
    assert np.array_equal(log_prior_of("empirical", 3, class_counts=[2, 0, 6]), log_prior_of([2, 0, 6], 3))
    assert np.array_equal(log_prior_of([[2, 0, 6]], 3), log_prior_of([2, 0, 6], 3))      # flattened, as calibrate always took a prior
    with pytest.raises(ValueError, match="listen: .*class counts"):
        log_prior_of("empirical", 3, who="listen")
    for bad in ([2, 6], [2, 0, 6, 1], [2, -1, 6], [2, float("nan"), 6], [0, 0, 0], "uniform"):
        with pytest.raises(ValueError, match="prior"):
            log_prior_of(bad, 3, class_counts=[2, 0, 6])


def test_posterior_trace_is_classify_after_every_sample():
    n, T = 3, 30
    bank = make_bank(PosteriorBackend, n=n)
    clips = _clip(n, T, seed=8)
    best, total = bank.classify(clips)
    tr = bank.posterior_trace(clips, threshold=0.5)
    assert tr.best.shape == (n, T - 1) and tr.conf.shape == (n, T - 1) and tr.post is None
    assert np.array_equal(tr.best[:, -1], best) and tr.decided_at.shape == (n,) and tr.decided_as.shape == (n,)
    ref = PR.posterior(bank.nll_per_step(clips), threshold=0.5)
    assert np.array_equal(tr.best, ref["best"]) and np.array_equal(tr.conf, ref["conf"])
    assert np.array_equal(tr.decided_at, ref["decision"]["step"]) and np.array_equal(tr.decided_as, ref["decision"]["member"])
    cut = bank.posterior_trace(clips, threshold=0.5, segment=7, want_post=True)
    assert np.array_equal(cut.best, tr.best) and np.array_equal(cut.conf, tr.conf) and np.array_equal(cut.decided_at, tr.decided_at)
    assert np.array_equal(cut.post, ref["post"])
    skew = bank.posterior_trace(clips, prior=[0.0, 1.0, 1.0], temperature=3.0)
    assert np.all(skew.best != 0) and np.all(skew.decided_at == -1)
    with pytest.raises(ValueError):
        bank.posterior_trace(clips, segment=0)


def _saved_bank(tmp_path, classes=("bass", "flute", "organ"), counts=None):
    hp = HParams(delta_t=1.0 / 16000, h_reg=200.0 / (np.pi * 16000) ** 2, minibatch_size=2, bond_dim=D)      # what sample.main assumes
    bank = PsiBank(hp, MEMBERS, backend=PosteriorBackend(D), classes=list(classes), label_key="fam")
    bank.class_counts = counts
    d = str(tmp_path / "bank")
    BankTrainer(bank).save(d)
    return d, hp


def test_sample_score_posterior_on_a_saved_bank(tmp_path, capsys):
    d, hp = _saved_bank(tmp_path, counts=[6, 1, 3])
    with open(os.path.join(d, "bank.json")) as f:
        assert json.load(f)["class_counts"] == [6, 1, 3]
    out, clip = str(tmp_path / "out"), str(tmp_path / "clip.npy")
    np.save(clip, make_audio(1, 21, hp.delta_t, seed=4)[0])
    M, names = len(MEMBERS), ["bass", "flute", "organ"]
    post = S.main(["--bankdir", d, "--out_dir", out, "--score", clip, "--posterior", "--threshold", "0.34", "--segment", "6"],
                  backend=PosteriorBackend(D))
    lines = capsys.readouterr().out.strip().splitlines()
    assert post.shape == (M, 20) and np.array_equal(np.load(os.path.join(out, "posterior.npy")), post)
    best, conf = np.load(os.path.join(out, "best.npy")), np.load(os.path.join(out, "conf.npy"))
    assert best.shape == (20,) and conf.shape == (20,) and np.array_equal(conf, post.max(axis=0)) and np.array_equal(best, post.argmax(axis=0))
    assert np.allclose(post.sum(axis=0), 1.0, rtol=0, atol=1e-6)
    assert len(lines) == M + 2 and all(lines[m].startswith(f"member {m} (class '{names[m]}'): final posterior") for m in range(M))
    b = int(best[-1])
    assert lines[M].startswith(f"clip 0: final best member {b} (class '{names[b]}')") and "decided at sample" in lines[M]
    first = int(np.flatnonzero(conf >= 0.34)[0])
    assert f"decided at sample {first} as member {int(best[first])} (class '{names[int(best[first])]}')" in lines[M]
    assert not os.path.exists(os.path.join(out, "nll.npy"))
    whole = S.main(["--bankdir", d, "--out_dir", out, "--score", clip, "--posterior", "--threshold", "1"], backend=PosteriorBackend(D))
    assert np.array_equal(whole, post) and "undecided" in capsys.readouterr().out
    # the priors: given, empirical (the counts of bank.json), and what is refused
    given = S.main(["--bankdir", d, "--out_dir", out, "--score", clip, "--posterior", "--prior", "6,1,3", "--temperature", "2"],
                   backend=PosteriorBackend(D))
    emp = S.main(["--bankdir", d, "--out_dir", out, "--score", clip, "--posterior", "--prior", "empirical", "--temperature", "2"],
                 backend=PosteriorBackend(D))
    assert np.array_equal(given, emp) and not np.array_equal(given, post)
    with pytest.raises(ValueError, match="3 members"):
        S.main(["--bankdir", d, "--out_dir", out, "--score", clip, "--posterior", "--prior", "1,2"], backend=PosteriorBackend(D))
    with pytest.raises(ValueError, match="--bankdir and --score"):
        S.main(["--bankdir", d, "--out_dir", out, "--posterior"], backend=PosteriorBackend(D))
    with pytest.raises(ValueError, match="--posterior"):
        S.main(["--bankdir", d, "--out_dir", out, "--score", clip, "--threshold", "0.5"], backend=PosteriorBackend(D))
    d2, _ = _saved_bank(tmp_path / "second")
    with pytest.raises(ValueError, match="class counts"):
        S.main(["--bankdir", d2, "--out_dir", out, "--score", clip, "--posterior", "--prior", "empirical"], backend=PosteriorBackend(D))


def test_evaluate_listen_on_a_saved_bank(tmp_path, capsys):
    from audio_mps_amd import tfrecord as tfr
    d, hp = _saved_bank(tmp_path, counts=[2, 2, 3])
    T, labels = 26, ["organ", "bass", "flute", "bass", "nobody", "organ", "flute"]
    from test_classify_host import quiet
    clips = quiet(len(labels), T, seed=6)
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "held.tfrecords"), clips, bytes_features={"fam": labels})
    curve = str(tmp_path / "curve.npy")
    argv = ["--bankdir", d, "--datadir", str(tmp_path), "--dataset", "held", "--sample_duration", str(T), "--minibatch_size", "3",
            "--storage", "float32", "--listen", "--threshold", "0.45", "--listen_curve", curve, "--json"]
    res = EV.main(argv, backend=PosteriorBackend(D))
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("listen held: decided=") and all(k in lines[0] for k in ("acc@1/16=", "acc@1/1=", "median_sample="))
    rec = json.loads(lines[1])
    assert rec["clips"] == 7 and rec["labelled"] == 6 and rec["accuracy_after"] == res["accuracy_after"] and rec["decided"] == res["decided"]
    # the same numbers by hand, from one trace over all the clips
    bank = S.load_bank(d, 16000, backend=PosteriorBackend(D))
    from audio_mps_amd.device_data import ResidentDataset
    ds = ResidentDataset.from_tfrecord(os.path.join(tmp_path, "held.tfrecords"), T, PosteriorBackend(D), storage="float32", label_key="fam")
    tr = bank.posterior_trace(ds.clips.numpy(), threshold=0.45)
    y = ds.class_positions(bank.classes)
    known = y >= 0
    want = (tr.best[known] == y[known, None]).mean(axis=0)
    assert np.array_equal(np.load(curve), want) and np.load(curve).shape == (T - 1,)
    assert res["accuracy_after"] == {"1/16": want[0], "1/8": want[2], "1/4": want[5], "1/2": want[11], "1/1": want[24]}
    dec = tr.decided_at >= 0
    assert res["decided"] == dec.mean() and (not dec.any() or res["mean_decision_sample"] == tr.decided_at[dec].mean())
    both = dec & known
    assert not both.any() or res["accuracy_at_decision"] == np.mean(tr.decided_as[both] == y[both])
    emp = EV.main(argv[:-5] + ["--prior", "empirical", "--temperature", "2"], backend=PosteriorBackend(D))
    assert emp["temperature"] == 2.0 and emp["clips"] == 7
    with pytest.raises(ValueError, match="--bankdir"):
        EV.main(["--datadir", str(tmp_path), "--dataset", "held", "--sample_duration", str(T), "--listen"], backend=PosteriorBackend(D))
    with pytest.raises(ValueError, match="--threshold"):
        EV.main(argv + ["--threshold", "0"], backend=PosteriorBackend(D))


def test_a_class_bank_records_its_class_counts(tmp_path):
    from test_classify_host import Backend, _argv, _files
    from audio_mps_amd import train
    _files(tmp_path)
    tr = train.main(_argv(tmp_path, ["--bank_by", "fam"]), backend=Backend())
    assert tr.bank.class_counts == [3, 4]                                             # x, y among the seven training clips
    logdir = os.path.join(tmp_path, "log", "guitar", f"4_{1.0 / 16000}_2")
    with open(os.path.join(logdir, "bank.json")) as f:
        assert json.load(f)["class_counts"] == [3, 4]
    assert S.load_bank(logdir, 16000, backend=Backend()).class_counts == [3, 4]
