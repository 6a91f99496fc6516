"""BankStream.score_posterior on real banks (a PsiBank of D = 3, M = 3, n = 2 and a RhoBank of D = 3, rank 3, M = 3): 40 steps in cuts of
1 + 17 + 22 against `score` on a twin stream -- total_nll, last_pred and the state records bit for bit, and the same `generate` behind
them -- and against the restatement of tests/_posterior_ref.py applied to the twin's downloaded nll: `best` and the decisions equal,
`post` and `conf` within twice the bound of include/cmps.h (cmps_bank_posterior, ROUNDING).  Then posterior_trace against classify, and
the two command lines end to end on a saved two-member bank."""
import json
import os

import numpy as np
import pytest
import torch

import _posterior_ref as PR
from _util import make_audio

from audio_mps_amd import HParams
from audio_mps_amd.bank import BankTrainer, PsiBank, RhoBank
from audio_mps_amd.stream import log_prior_of

pytestmark = pytest.mark.gpu

D, RANK, M, N = 3, 3, 3, 2
CUTS = (1, 17, 22)
STEPS = sum(CUTS)
PRIOR, TEMPERATURE, THRESHOLD = [0.5, 0.2, 0.3], 0.01, 0.9


def make_bank(kind, members=M):
    """Members as in the bank stream tests: sigma = 0.1, Rx, Ry x 0.3, a seed and an A of their own."""
    hp = HParams(minibatch_size=N, bond_dim=D, sigma=0.1, A=5.0, initial_rank=RANK)
    bank = (RhoBank if kind == "rho" else PsiBank)(hp, [{"seed": 100 + m} for m in range(members)])
    for m, mo in enumerate(bank.models):
        mo.variables["Rx"] *= np.float32(0.3)
        mo.variables["Ry"] *= np.float32(0.3)
        mo.variables["A"] = np.asarray(np.float32(5.0 + m))
    return bank


def _clip():
    return make_audio(N, STEPS + 1, HParams().delta_t, seed=11).astype(np.float32)


def _cut(st, clip, how, **kw):
    out, a = [], 0
    for i, c in enumerate(CUTS):
        out.append(getattr(st, how)(clip[:, a:a + c + (i == 0)], **kw))
        a += c + (i == 0)
    return out


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_score_posterior_against_score_on_a_twin_and_the_restatement(kind):
    bank, clip = make_bank(kind), _clip()
    twin = bank.open_stream(N, 60, seed=3)
    st = bank.open_stream(N, 60, seed=3, prior=PRIOR, temperature=TEMPERATURE, threshold=THRESHOLD)
    assert st.native and twin.native
    nll = np.concatenate(_cut(twin, clip, "score"), axis=-1)
    traces = _cut(st, clip, "score_posterior", want_post=True)
    assert np.array_equal(st.total_nll.view(np.uint32), twin.total_nll.view(np.uint32)), "total_out is score's running loss"
    assert np.array_equal(st.last_pred.view(np.uint32), twin.last_pred.view(np.uint32)) and st.position == twin.position == STEPS
    assert np.array_equal(st.last, twin.last)
    torch.cuda.synchronize()
    assert torch.equal(st._state, twin._state), "the state records"
    assert np.array_equal(st.generate(9).view(np.uint32), twin.generate(9).view(np.uint32))
    # the restatement on the twin's nll, whole
    ref = PR.posterior(nll, log_prior=log_prior_of(PRIOR, M), inv_temp=1.0 / TEMPERATURE, threshold=THRESHOLD)
    near, close = PR.ill_posed(ref, (THRESHOLD,))
    assert len(near) == 0 and len(close) == 0, "the comparison of best and the decisions is well-posed"
    assert np.array_equal(ref["total_out"].view(np.uint32), twin.total_nll.view(np.uint32))
    best, conf, post = (np.concatenate([getattr(t, k) for t in traces], axis=-1) for k in ("best", "conf", "post"))
    assert np.array_equal(best, ref["best"])
    for got, exact, scale, what in ((post, ref["post64"], ref["scale"][None], "post"), (conf, ref["conf64"], ref["scale"], "conf")):
        err, bar = np.abs(got.astype(np.float64) - ref[what].astype(np.float64)), 2.0 * PR.bound(exact, M, scale)
        print(f"{kind}: {what} worst error {err.max():.3e}, worst error / (2 x bound) {float((err / bar).max()):.3f}; "
              f"conf from {conf.min():.3f} to {conf.max():.3f}")
        assert np.all(err <= bar), (what, float(err.max()))
    assert np.array_equal(st.decided_at, ref["decision"]["step"]) and np.array_equal(st.decided_as, ref["decision"]["member"])
    first = [t.decided_at.copy() for t in traces]                    # carried across the cuts: once decided, a path stays as it is
    for a, b in zip(first[:-1], first[1:]):
        assert np.array_equal(b[a >= 0], a[a >= 0])
    print(f"{kind}: decided at {st.decided_at.tolist()} as {st.decided_as.tolist()}")


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_posterior_trace_ends_where_classify_does(kind):
    bank, clips = make_bank(kind), _clip()
    best, total = bank.classify(clips)
    tr = bank.posterior_trace(clips, threshold=0.99)
    assert tr.best.shape == (N, STEPS) and np.array_equal(tr.best[:, -1], best)
    cut = bank.posterior_trace(clips, threshold=0.99, segment=13, want_post=True)
    assert np.array_equal(cut.best, tr.best) and np.array_equal(cut.conf.view(np.uint32), tr.conf.view(np.uint32))
    assert np.array_equal(cut.decided_at, tr.decided_at) and cut.post.shape == (M, N, STEPS)
    assert np.allclose(cut.post.sum(axis=0), 1.0, rtol=0, atol=1e-6)


def test_the_two_command_lines_on_a_saved_bank(tmp_path, capsys):
    from audio_mps_amd import evaluate as EV
    from audio_mps_amd import sample as S
    from audio_mps_amd import tfrecord as tfr
    hp = HParams(delta_t=1.0 / 16000, h_reg=200.0 / (np.pi * 16000) ** 2, minibatch_size=N, bond_dim=D)      # what sample.main assumes
    bank = PsiBank(hp, [{"seed": 3}, {"seed": 4}], classes=["x", "y"], label_key="fam")
    bank.class_counts = [3, 1]
    d, out = str(tmp_path / "bank"), str(tmp_path / "out")
    BankTrainer(bank).save(d)
    T, labels = 33, ["x", "y", "y", "x", "y"]
    rng = np.random.default_rng(2)
    clips = rng.integers(-3000, 3000, size=(len(labels), T)).astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15)
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "held.tfrecords"), clips, bytes_features={"fam": labels})
    curve = str(tmp_path / "curve.npy")
    res = EV.main(["--bankdir", d, "--datadir", str(tmp_path), "--dataset", "held", "--sample_duration", str(T), "--minibatch_size", "2",
                   "--listen", "--threshold", "0.55", "--prior", "empirical", "--listen_curve", curve, "--json"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0].startswith("listen held: decided=") and json.loads(lines[1])["clips"] == 5 and res["labelled"] == 5
    assert np.load(curve).shape == (T - 1,) and set(res["accuracy_after"]) == {"1/16", "1/8", "1/4", "1/2", "1/1"}
    np.save(os.path.join(tmp_path, "clip.npy"), clips[0])
    post = S.main(["--bankdir", d, "--out_dir", out, "--score", os.path.join(tmp_path, "clip.npy"), "--posterior", "--threshold", "0.55",
                   "--segment", "10"])
    text = capsys.readouterr().out
    assert post.shape == (2, T - 1) and np.allclose(post.sum(axis=0), 1.0, rtol=0, atol=1e-6)
    assert np.array_equal(np.load(os.path.join(out, "conf.npy")), post.max(axis=0)) and "final best member" in text
    assert "member 0 (class 'x'): final posterior" in text and ("decided at sample" in text or "undecided" in text)
