"""Calibration of a class bank without a GPU: the numpy restatement of cmps_bank_calibrate (tests/_calib_ref.py) against itself in long
double within the header's bounds, the well-posedness of every draw the GPU tests run on, the closed forms, and the host layer on a stand-in
backend -- BankTrainer.calibrate / cross_entropy, the bank.json round trip, and the flags of evaluate and sample."""
import json
import os

import numpy as np
import pytest
import torch

import _calib_ref as R
import _classify_ref as CR
import _eval_ref as ER
from _util import OracleBackend

TOL = 1e-9


class Backend(R.CalibMethods, CR.ClassifyMethods, ER.EvalMethods, OracleBackend):
    def __init__(self, D=4):
        super().__init__(D)
        self._eval_init()
        self._classify_init()
        self._calib_init()


class NoCalibBackend(CR.ClassifyMethods, ER.EvalMethods, OracleBackend):
    def __init__(self, D=4):
        super().__init__(D)
        self._eval_init()
        self._classify_init()


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", R.SHAPES)
def test_float64_meets_the_headers_bounds_and_every_draw_is_well_posed(M, N):
    loss, labels, N = R.draw(M, N, seed=100 + M)
    assert loss.shape == (M, N + 3) and np.all(loss[:, N:].view(np.uint32) == 0x7FC5A5A5)
    l = loss[:, :N]
    if N >= 30:
        assert np.isnan(l).any() and np.isposinf(l).any() and np.isneginf(l).any() and -1 in labels and M in labels
    for fit in (1, 2, 3):
        k0, c0 = R.start(l, labels, fit)
        kr, cr, _ = R.optimise(l, labels, fit, k0, c0)
        for kappa, c in ((k0, c0), (float(kr), np.asarray(cr, dtype=np.float64))):
            lo, hi = R.evaluate(l, labels, kappa, c, np.float64), R.evaluate(l, labels, kappa, c, np.longdouble)
            eJ, eg, eq = hi.bounds()
            assert abs(float(lo.J - hi.J)) <= eJ and abs(float(lo.g - hi.g)) <= eg and np.max(np.abs((lo.q - hi.q).astype(np.float64))) <= eq
            assert lo.n == hi.n > 0 and (lo.n_unlabelled, lo.n_own_absent) == (hi.n_unlabelled, hi.n_own_absent)
            if N >= 30:
                assert hi.n_unlabelled == 2 and hi.n_own_absent == 2
        # well-posed: the optimum strictly inside the box, and the rounding bound an order of magnitude below the tolerance there
        best = R.evaluate(l, labels, kr, cr, np.longdouble)
        if fit & R.FIT_TEMPERATURE:
            assert 1e-6 < float(kr) < 1e6 and abs(float(kr * best.g)) <= 1e-13
            assert float(kr) * best.bounds()[1] <= TOL / 10
        if fit & R.FIT_PRIOR:
            assert best.resid() <= 1e-13 and best.bounds()[2] / best.n <= TOL / 10
        accuracy = np.mean(np.argmin(np.where(np.isfinite(l), l, np.inf), axis=0)[best.used] == labels[best.used])
        assert 0.2 <= accuracy <= 0.9                         # some clips wrong: the temperature has something to balance


def test_closed_forms_hold_for_the_reference():
    loss = np.array([[2000.0, 2001.0, 1999.0, 2004.0], [2001.0, 2000.0, 2000.0, 2003.0]], dtype=np.float32)
    labels = np.array([0, 1, 0, 0], dtype=np.int32)
    kr, cr, _ = R.optimise(loss, labels, R.FIT_TEMPERATURE, 1.0, np.zeros(2))
    ev = R.evaluate(loss, labels, kr, cr, np.longdouble)
    assert abs(float(kr) - np.log(3.0)) <= 1e-14 and abs(float(ev.h) - 3.0 / 16.0) <= 1e-14
    assert abs(float(ev.J) - (0.75 * np.log(4.0 / 3.0) + 0.25 * np.log(4.0))) <= 1e-14
    flat = np.full((2, 8), 1234.5, dtype=np.float32)
    y = np.array([0, 1, 0, 0, 1, 0, 1, 0], dtype=np.int32)
    kr, cr, rounds = R.optimise(flat, y, R.FIT_PRIOR | R.FIT_TEMPERATURE, 0.37, np.zeros(2))
    assert np.max(np.abs(R.normalised_prior(cr) - [5 / 8, 3 / 8])) <= 1e-15 and rounds == 2
    ev = R.evaluate(flat, y, kr, cr)
    assert float(ev.g) == 0.0 and float(ev.h) == 0.0
    # the gradient with respect to c is (q - n_m) / n, and J is what the classifier record calls the cross-entropy at kappa = 1, c = 0
    loss, labels, N = R.draw(5, 300, seed=105)
    l = loss[:, :N]
    c = np.array([0.3, -0.2, 0.1, 0.0, 0.5])
    ev = R.evaluate(l, labels, 0.8, c, np.longdouble)
    for m in range(5):
        step = np.zeros(5)
        step[m] = 1e-6
        num = (R.evaluate(l, labels, 0.8, c + step, np.longdouble).J - R.evaluate(l, labels, 0.8, c - step, np.longdouble).J) / 2e-6
        assert abs(float(num - (ev.q[m] - ev.n_m[m]) / ev.n)) <= 1e-9
    num = (R.evaluate(l, labels, 0.8 + 1e-6, c, np.longdouble).J - R.evaluate(l, labels, 0.8 - 1e-6, c, np.longdouble).J) / 2e-6
    assert abs(float(num - ev.g)) <= 1e-9
    rec = CR.Record(5).add(l, labels, 0).record()
    assert abs(rec["sum_xent"] / rec["n_xent"] - float(R.evaluate(l, labels, 1.0, np.zeros(5)).J)) <= 1e-12


# ---------------------------------------------------------------------------------------------------
# the bank
# ---------------------------------------------------------------------------------------------------
D, T, MB = 4, 24, 4


def hparams():
    from audio_mps_amd import HParams
    return HParams(minibatch_size=MB, bond_dim=D, delta_t=1.0 / 16000)


def class_bank(classes=("a", "b", "c"), be=None):
    from audio_mps_amd.bank import PsiBank
    return PsiBank(hparams(), [{"seed": 3 + m} for m in range(len(classes))], backend=be or Backend(), classes=list(classes), label_key="family")


def quiet(n, length, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3000, 3000, size=(n, length)).astype(np.int16)).astype(np.float32) * np.float32(2.0 ** -15)


LABELS = np.array(list("abcabczabcab"), dtype=object)          # clip 6 carries a label the bank has no member for


def test_calibrate_and_cross_entropy_on_a_stand_in_backend():
    from audio_mps_amd.bank import BankTrainer, CalibrationResult, PsiBank
    from audio_mps_amd.device_data import ResidentDataset
    be = Backend()
    bt = BankTrainer(class_bank(be=be))
    clips = quiet(12, T)
    ds = ResidentDataset(clips, be, labels=LABELS)
    res = bt.calibrate(ds, 5, fit="both", temperature=2.0, prior=[0.5, 0.25, 0.25], tol=1e-8, max_iter=77, kappa_min=1e-3, kappa_max=1e3)
    assert isinstance(res, CalibrationResult) and be.calib_downloads == 1 and len(be.calib_calls) == 1
    call = be.calib_calls[0]
    assert (call["shape"], call["fit"], call["kappa"], call["tol"], call["max_iter"], call["kappa_min"], call["kappa_max"]) == \
        ((3, 12), 3, 0.5, 1e-8, 77, 1e-3, 1e3)
    assert np.array_equal(call["log_prior"], np.log([0.5, 0.25, 0.25]))
    loss = np.stack([np.concatenate([m.loss_per_clip(clips[i:i + 5]) for i in range(0, 12, 5)]) for m in bt.bank.models])
    assert np.array_equal(call["loss"].view(np.uint32), loss.astype(np.float32).view(np.uint32))          # the ordered pass, batch by batch
    assert np.array_equal(call["labels"], ds.class_positions(["a", "b", "c"]))
    assert (res.n_used, res.n_unlabelled, res.n_own_absent, res.T, res.fit, res.unfitted) == (11, 1, 0, T, "both", [])
    assert res.xent_after <= res.xent_before and res.passes >= 1 and isinstance(res.converged, bool) and isinstance(res.at_bound, bool)
    assert abs(res.prior.sum() - 1.0) <= 1e-15 and np.allclose(res.prior, np.exp(res.log_prior) / np.exp(res.log_prior).sum(), rtol=1e-14, atol=0)
    assert "temperature=" in res.line() and "xent_before=" in res.line() and "unfitted=0" in res.line()
    json.dumps(res.scalars())
    assert bt.calibration == res.meta() and set(bt.calibration) == {"temperature", "log_prior", "fit", "dataset", "clips", "T", "xent_before",
                                                                     "xent_after"}
    # cross_entropy: the zero-iteration call, at the given values
    x = bt.cross_entropy(ds, res.temperature, log_prior=res.log_prior, minibatch_size=5)
    assert be.calib_calls[-1]["fit"] == 0 and be.calib_calls[-1]["max_iter"] == 0
    assert abs(x - res.xent_after) <= 1e-12
    plain = bt.evaluate_classifier(ds, 5)
    assert abs(bt.cross_entropy(ds, 1.0, None, 5) - plain.cross_entropy) <= 1e-12
    # a class without a held-out clip is reported, and "empirical" needs the counts
    two = ResidentDataset(clips, be, labels=np.where(LABELS == "c", "a", LABELS))
    assert bt.calibrate(two, 5, fit="prior").unfitted == ["c"]
    with pytest.raises(ValueError, match="class counts"):
        bt.calibrate(ds, 5, prior="empirical")
    bt.bank.class_counts = [6, 3, 3]
    bt.calibrate(ds, 5, prior="empirical")
    assert np.array_equal(be.calib_calls[-1]["log_prior"], np.log([0.5, 0.25, 0.25]))
    # a prior of zero: fine for a class without a held-out clip (null in JSON, which has no -inf), refused for one that has clips
    res0 = bt.calibrate(two, 5, fit="prior", prior=[0.5, 0.5, 0.0])
    assert res0.log_prior[2] == -np.inf and res0.prior[2] == 0.0 and res0.meta()["log_prior"][2] is None
    json.dumps(res0.meta(), allow_nan=False), json.dumps(res0.scalars(), allow_nan=False)
    assert bt.cross_entropy(two, res0.temperature, log_prior=res0.meta()["log_prior"], minibatch_size=5) == pytest.approx(res0.xent_after, abs=1e-12)
    with pytest.raises(ValueError, match="prior is zero for \\['c'\\]"):
        bt.calibrate(ds, 5, fit="temperature", prior=[0.5, 0.5, 0.0])
    # errors
    for kw, match in ((dict(fit="all"), "fit"), (dict(temperature=0.0), "temperature"), (dict(prior=[1.0, 1.0]), "prior"),
                      (dict(prior=[1.0, -1.0, 1.0]), "prior"), (dict(prior="guess"), "prior")):
        with pytest.raises(ValueError, match=match):
            bt.calibrate(ds, 5, **kw)
    with pytest.raises(ValueError, match="no labels"):
        bt.calibrate(ResidentDataset(clips, be), 5)
    with pytest.raises(ValueError, match="no clip"):                                   # NO_DATA
        bt.calibrate(ResidentDataset(clips, be, labels=np.array(["z"] * 12, dtype=object)), 5)
    nb = NoCalibBackend()
    with pytest.raises(ValueError, match="bank_calibrate") as e:
        BankTrainer(class_bank(be=nb)).calibrate(ResidentDataset(clips, nb, labels=LABELS), 5)
    assert "NoCalibBackend" in str(e.value)
    with pytest.raises(ValueError, match="class bank"):
        BankTrainer(PsiBank(hparams(), [{"seed": 1}], backend=be)).calibrate(ds, 5)


def test_every_held_out_pass_starts_afresh():
    """One trainer judged and then calibrated gives what two fresh trainers give, bit for bit: a pass carries nothing over to the next.
    A dataset without a batch is refused by every caller, in its own name.  The stand-in has no bank entries, so this is the pass with the
    member-loop forward, and `evaluate` is every member's Trainer.evaluate; the native fold is the GPU tests'."""
    from audio_mps_amd.bank import BankTrainer
    from audio_mps_amd.device_data import ResidentDataset
    clips = quiet(12, T)

    def fresh():
        be = Backend()
        return be, BankTrainer(class_bank(be=be)), ResidentDataset(clips, be, labels=LABELS)

    def same(a, b):
        return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=not isinstance(a[k], (list, str))) for k in a)
    be, bt, ds = fresh()
    judged, fitted = bt.evaluate_classifier(ds, 5, keep_best=True), bt.calibrate(ds, 5, fit="both")
    be1, bt1, ds1 = fresh()
    be2, bt2, ds2 = fresh()
    alone, fit_alone = bt1.evaluate_classifier(ds1, 5, keep_best=True), bt2.calibrate(ds2, 5, fit="both")
    assert same(judged.scalars(), alone.scalars()) and np.array_equal(judged.confusion, alone.confusion)
    assert np.array_equal(judged.best, alone.best) and np.array_equal(judged.unlabelled_best, alone.unlabelled_best)
    assert same(fitted.scalars(), fit_alone.scalars())
    assert np.array_equal(be.calib_calls[-1]["loss"].view(np.uint32), be2.calib_calls[-1]["loss"].view(np.uint32))
    assert [r.scalars() for r in bt.evaluate(ds, 5)] == [r.scalars() for r in bt1.evaluate(ds1, 5)]
    ds.ordered = lambda minibatch_size, T=None: iter(())
    for who, call in (("evaluate", bt.evaluate), ("evaluate_classifier", bt.evaluate_classifier), ("calibrate", bt.calibrate),
                      ("cross_entropy", bt.cross_entropy)):
        with pytest.raises(ValueError, match=f"^{who}: the dataset yielded no batch"):
            call(ds, minibatch_size=5)


def test_bank_json_round_trip(tmp_path):
    from audio_mps_amd.bank import BankTrainer
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.sample import load_bank
    be = Backend()
    bt = BankTrainer(class_bank(be=be))
    d0, d1 = str(tmp_path / "before"), str(tmp_path / "after")
    bt.save(d0)
    with open(os.path.join(d0, "bank.json"), "rb") as f:
        before = f.read()
    meta = json.loads(before)
    assert "calibration" not in meta
    # without a calibration the file is byte for byte what `save` always wrote: the keys it had, dumped by json.dump
    want = {"members": bt.bank.overrides, "adam_step": 0, "global_step": 0, "label_key": "family", "classes": ["a", "b", "c"]}
    assert before == json.dumps(want).encode()
    assert load_bank(d0, 16000, backend=Backend()).calibration is None
    res = bt.calibrate(ResidentDataset(quiet(12, T), be, labels=LABELS), 5, fit="both")
    bt.save(d1)
    with open(os.path.join(d1, "bank.json")) as f:
        meta = json.load(f)
    assert {k: v for k, v in meta.items() if k != "calibration"} == want and meta["calibration"] == res.meta()
    other = BankTrainer(class_bank())
    assert other.calibration is None and other.restore(d1) and other.calibration == res.meta()
    assert other.restore(d0) and other.calibration is None
    assert load_bank(d1, 16000, backend=Backend()).calibration == res.meta()


# ---------------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------------
def _bankdir(tmp):
    from audio_mps_amd import tfrecord as tfr
    from audio_mps_amd.bank import BankTrainer
    d = os.path.join(tmp, "bank")
    bank = class_bank(("x", "y"))
    bank.label_key = "fam"
    BankTrainer(bank).save(d)
    held = ["y", "x", "x", "y", "q", "x", "y"]
    tfr.write_audio_tfrecord(os.path.join(tmp, "organ.tfrecords"), quiet(7, T, 4), {"pitch": [60] * 7}, {"fam": held})
    return d


def _eval(tmp, d, extra):
    from audio_mps_amd import evaluate as EV
    return EV.main(["--bankdir", d, "--datadir", str(tmp), "--dataset", "organ", "--sample_duration", str(T), "--minibatch_size", "4"] + extra,
                   backend=Backend())


def test_evaluate_calibrate_save_and_calibrated(tmp_path, capsys):
    d = _bankdir(str(tmp_path))
    with open(os.path.join(d, "bank.json")) as f:
        before = json.load(f)
    _eval(tmp_path, d, ["--calibrate", "both", "--json"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[1].startswith("calibration temperature=") and all(k in lines[1] for k in ("xent_before=", "xent_after=", "converged=", "passes=",
                                                                                             "unfitted="))
    assert lines[2].startswith("class 'x': prior ") and lines[3].startswith("class 'y': prior ")
    cal = json.loads(lines[-1])["calibration"]
    assert cal["fit"] == "both" and cal["xent_after"] <= cal["xent_before"] and len(cal["prior"]) == 2
    with open(os.path.join(d, "bank.json")) as f:
        assert json.load(f) == before                                                  # nothing is saved unless asked
    _eval(tmp_path, d, ["--calibrate", "both", "--save_calibration"])
    with open(os.path.join(d, "bank.json")) as f:
        after = json.load(f)
    assert {k: v for k, v in after.items() if k != "calibration"} == before and not os.path.exists(os.path.join(d, "bank.json.tmp"))
    saved = after["calibration"]
    assert set(saved) == {"temperature", "log_prior", "fit", "dataset", "clips", "T", "xent_before", "xent_after"}
    assert (saved["fit"], saved["dataset"], saved["clips"], saved["T"]) == ("both", "organ", 6, T) and saved["temperature"] == cal["temperature"]
    capsys.readouterr()
    _eval(tmp_path, d, ["--calibrated", "--json"])
    out = capsys.readouterr().out.strip().splitlines()
    assert out[1].startswith("calibrated organ: xent_calibrated=")
    rec = json.loads(out[-1])
    assert abs(rec["xent_calibrated"] - saved["xent_after"]) <= 1e-12                   # (kappa goes through 1 / temperature twice)
    assert rec["cross_entropy"] >= rec["xent_calibrated"]


@pytest.mark.parametrize("extra, match", [
    (["--calibrated"], "no calibration"), (["--calibrated", "--listen"], "no calibration"),
    (["--calibrated", "--temperature", "2"], "--temperature"), (["--calibrated", "--prior", "0.5,0.5"], "--prior"),
    (["--save_calibration"], "--calibrate"), (["--calibrate", "both", "--calibrated"], "one at a time"),
    (["--calibrate", "both", "--listen"], "--listen")])
def test_evaluate_flag_errors(tmp_path, extra, match):
    d = _bankdir(str(tmp_path))
    with pytest.raises(ValueError, match=match):
        _eval(tmp_path, d, extra)
    from audio_mps_amd import evaluate as EV
    with pytest.raises(ValueError, match="--bankdir"):
        EV.main(["--dataset", "organ", "--datadir", str(tmp_path), "--calibrate", "both"], backend=Backend())


def test_evaluate_keeps_its_old_arguments():
    from audio_mps_amd import evaluate as EV, sample as S
    for parser in (EV.build_parser(), S.build_parser()):
        acts = {a.dest: a for a in parser._actions}
        assert acts["temperature"].type is float and acts["temperature"].default == 1.0 and acts["prior"].default is None
        assert acts["prior"].metavar == "P0,P1,...|empirical" and acts["calibrated"].default is False


def test_sample_flag_errors(tmp_path):
    from audio_mps_amd import sample as S
    d = _bankdir(str(tmp_path))
    clip = str(tmp_path / "clip.npy")
    np.save(clip, quiet(1, T, 9)[0])
    base = ["--bankdir", d, "--out_dir", str(tmp_path / "out"), "--score", clip]
    for extra, match in ((["--calibrated"], "--posterior"), (["--posterior", "--calibrated", "--temperature", "2"], "--temperature"),
                         (["--posterior", "--calibrated", "--prior", "0.5,0.5"], "--prior"), (["--posterior", "--calibrated"], "no calibration")):
        with pytest.raises(ValueError, match=match):
            S.main(base + extra, backend=Backend())
