"""Held-out evaluation: the loss of a model over a dataset it has not seen, reduced on the device.

  reference          training_estimators.py:70-74   eval_metric_ops={"loss": tf.metrics.mean(loss)} -- declared, never run
  evaluate(...)      a pass over a ResidentDataset in file order (ResidentDataset.ordered): every batch runs the model's own forward scan
                     (what loss_per_clip runs: cmps_psi_loss_fwd / cmps_rho_loss_fwd / cmps_legacy_loss_fwd), its per-clip losses are folded
                     into one 64-byte record where they are (HipScan.loss_stats, cmps_loss_stats), and the record is downloaded ONCE at the
                     end -- not one download per batch, as model.loss_per_clip makes.
  EvalResult         the mean the reference declares, and what a bare mean hides: how many clips came out non-finite (1 + z <= 0,
                     model.py:294) and which was the first, the worst and the best clip, the spread.

A clip's id is its position in the dataset's file.  Needs a backend with loss_stats; one without it (the stand-ins of the host tests that
lack it) is a ValueError, as with draw_noise and gather_batch.
Run:  python -m audio_mps_amd.evaluate --modeldir=LOGDIR --datadir=DIR --dataset=nsynth_valid --sample_duration=16000 --storage=auto
"""
from __future__ import annotations

import argparse
import json
import math
import os
from dataclasses import dataclass, fields
from typing import Callable, Optional

import numpy as np


@dataclass
class EvalResult:
    mean: float                    # sum / n_finite: the mean loss per clip over the finite ones (NaN while there is none)
    per_sample: float              # mean / (T - 1): per scored sample, the figure that compares runs of different T
    std: float                     # unbiased standard deviation of the finite losses (0 below two of them)
    sem: float                     # std / sqrt(n_finite)
    n_clips: int                   # clips evaluated, finite or not
    n_nonfinite: int
    first_nonfinite: int           # id of the first clip whose loss is NaN or +-Inf, -1 when there is none
    min: float
    max: float
    argmin: int                    # id of the clip with the smallest finite loss (lowest id on ties), -1 when there is none
    argmax: int
    T: int
    losses: Optional[np.ndarray] = None        # keep_losses: float32 [n_clips], in the dataset's order

    @classmethod
    def from_stats(cls, stats: dict, T: int, losses: Optional[np.ndarray] = None) -> "EvalResult":
        """From the record of cmps_loss_stats (HipScan.read_stats).  The variance is (sumsq - sum^2 / n) / (n - 1) in float64, clamped at 0
        (the difference of two rounded sums can come out a hair negative for equal losses)."""
        n, s, q = int(stats["n_finite"]), float(stats["sum"]), float(stats["sumsq"])
        mean = s / n if n else float("nan")
        var = max((q - s * s / n) / (n - 1), 0.0) if n > 1 else 0.0
        std = math.sqrt(var)
        return cls(mean=mean, per_sample=mean / (T - 1) if T > 1 else float("nan"), std=std, sem=std / math.sqrt(n) if n else float("nan"),
                   n_clips=n + int(stats["n_nonfinite"]), n_nonfinite=int(stats["n_nonfinite"]), first_nonfinite=int(stats["first_nonfinite"]),
                   min=float(stats["min"]), max=float(stats["max"]), argmin=int(stats["argmin"]), argmax=int(stats["argmax"]), T=int(T),
                   losses=losses)

    def scalars(self) -> dict:
        """Everything but ``losses``, as JSON takes it."""
        return {f.name: getattr(self, f.name) for f in fields(self) if f.name != "losses"}


@dataclass
class ClassifierResult:
    """A class bank judged as a classifier (BankTrainer.evaluate_classifier), from the record of cmps_bank_classify_stats."""
    accuracy: float                # n_correct / n_labelled: over the decided clips with a label among the classes (NaN without any)
    cross_entropy: float           # sum_xent / n_xent: mean -log p(label | clip) under a uniform prior (NaN while n_xent == 0)
    mean_margin: float             # sum_margin / n_margin: mean gap between the best and the second-best member's loss
    n_clips: int                   # clips evaluated: decided + undecided
    n_labelled: int                # decided clips whose label is one of the bank's classes: the confusion matrix's total
    n_correct: int
    n_undecided: int               # clips under which no member's loss was finite
    n_unlabelled: int              # decided clips without a label among the classes
    first_undecided: int           # id of the first undecided clip, -1 when there is none
    n_xent: int
    n_margin: int
    T: int
    classes: list
    confusion: np.ndarray          # int64 [M, M]: row = the clip's class, column = the member that won it
    recall: np.ndarray             # float64 [M]: confusion[m, m] / confusion[m].sum() (NaN for a class without a decided clip)
    unlabelled_best: np.ndarray    # int64 [M]: the decided unlabelled clips by the member that won them
    best: Optional[np.ndarray] = None          # keep_best: int32 [n_clips], the winning member of every clip, -1 for undecided

    @classmethod
    def from_stats(cls, stats: dict, classes, T: int, best: Optional[np.ndarray] = None) -> "ClassifierResult":
        conf = np.asarray(stats["confusion"], dtype=np.int64)
        rows = conf.sum(axis=1)
        n_lab = int(conf.sum())
        nan = float("nan")
        with np.errstate(invalid="ignore", divide="ignore"):
            recall = np.where(rows > 0, np.diagonal(conf) / np.maximum(rows, 1), np.nan).astype(np.float64)
        return cls(accuracy=int(stats["n_correct"]) / n_lab if n_lab else nan,
                   cross_entropy=float(stats["sum_xent"]) / int(stats["n_xent"]) if stats["n_xent"] else nan,
                   mean_margin=float(stats["sum_margin"]) / int(stats["n_margin"]) if stats["n_margin"] else nan,
                   n_clips=int(stats["n_decided"]) + int(stats["n_undecided"]), n_labelled=n_lab, n_correct=int(stats["n_correct"]),
                   n_undecided=int(stats["n_undecided"]), n_unlabelled=int(stats["n_unlabelled"]),
                   first_undecided=int(stats["first_undecided"]), n_xent=int(stats["n_xent"]), n_margin=int(stats["n_margin"]), T=int(T),
                   classes=list(classes), confusion=conf, recall=recall,
                   unlabelled_best=np.asarray(stats["unlabelled_best"], dtype=np.int64), best=best)

    def scalars(self) -> dict:
        """The figures and the per-class recall, as a JSON line takes them (the matrix and ``best`` are files of their own)."""
        out = {f.name: getattr(self, f.name) for f in fields(self) if f.name not in ("confusion", "recall", "unlabelled_best", "best")}
        out["recall"] = [None if np.isnan(r) else float(r) for r in self.recall]
        return out

    def line(self) -> str:
        return (f"accuracy={self.accuracy:.4f} xent={self.cross_entropy:.6g} margin={self.mean_margin:.6g} clips={self.n_clips} "
                f"undecided={self.n_undecided}")


def _need_stats(backend):
    if not (hasattr(backend, "loss_stats") and hasattr(backend, "read_stats")):
        raise ValueError(f"evaluate needs a backend that reduces the per-clip losses on the device (loss_stats): {type(backend).__name__} "
                         "has none")


def pass_shape(backend, dataset, minibatch_size, default_minibatch, T):
    """(clips per batch, T, largest batch) of a trainer's ``evaluate``: ``minibatch_size`` None or 0 is the training one, ``T`` None the clips' length."""
    _need_stats(backend)
    mb = int(minibatch_size) if minibatch_size else int(default_minibatch)
    T = dataset.clip_len if T is None else int(T)
    if T < 2 or mb < 1:
        raise ValueError("evaluate needs T >= 2 and minibatch_size >= 1")
    return mb, T, min(mb, dataset.n_clips)


def run_pass(batches, forward: Callable, backend, T: int, keep_losses: bool = False) -> EvalResult:
    """The loop of `evaluate` over ``batches`` (an iterable of (first_id, batch)) with ``forward(batch)`` -> per-clip losses on the device:
    one loss_stats per batch, ONE download at the end (two with keep_losses: the record and the concatenated losses)."""
    import torch
    _need_stats(backend)
    stats, kept = None, []
    for first_id, batch in batches:
        loss = forward(batch)
        stats = backend.loss_stats(loss, first_id, stats, reset=stats is None)
        if keep_losses:
            kept.append(loss.clone())              # (the backend's loss tensor is overwritten by the next forward)
    if stats is None:
        raise ValueError("evaluate: the dataset yielded no batch")
    losses = torch.cat(kept).cpu().numpy() if keep_losses else None
    return EvalResult.from_stats(backend.read_stats(stats), T, losses)


def evaluate(model, dataset, minibatch_size: int, T: Optional[int] = None, keep_losses: bool = False) -> EvalResult:
    """The model's loss over every clip of ``dataset`` (a ResidentDataset of either storage) once, in file order, in batches of
    ``minibatch_size`` (the short last batch included); ``T < L`` scores the first T samples of every clip.  The parameters are uploaded
    once, every batch then costs a gather, the forward scan and the 64-byte update; ``keep_losses`` also brings the per-clip losses back."""
    T = dataset.clip_len if T is None else int(T)
    if T < 2:
        raise ValueError("evaluate needs T >= 2 (one increment)")
    be = model._get_backend()
    _need_stats(be)
    B_max = min(int(minibatch_size), dataset.n_clips)
    be = model._prepare(B_max, T, train=False)
    fwd = model._forward_entry(be)
    return run_pass(dataset.ordered(minibatch_size, T), lambda batch: fwd(batch, save_for_bwd=False), be, T, keep_losses)


def build_parser():
    p = argparse.ArgumentParser(description="Evaluate a trained PsiCMPS or RhoCMPS on a held-out TFRecord dataset (MI355X)")
    p.add_argument("--modeldir", default="./data", help="directory holding model.ckpt.npz, or a checkpoint file (either model)")
    p.add_argument("--datadir", default="./data")
    p.add_argument("--dataset", required=True, help="NAME of NAME.tfrecords in --datadir")
    p.add_argument("--sample_duration", type=int, default=2 ** 16, help="samples per record; the model scores all of them")
    p.add_argument("--sample_rate", type=int, default=16000)
    p.add_argument("--minibatch_size", type=int, default=64)
    p.add_argument("--storage", default="auto", choices=["float32", "int16", "auto"],
                   help="how the dataset is held on the device: int16 halves the memory of 16-bit PCM data without changing a bit")
    p.add_argument("--per_clip", default=None, metavar="OUT.npy", help="also write the per-clip losses, float32 [clips], in file order")
    p.add_argument("--hparams", default="", help="as for training (r_reg, h_reg, sigma, delta_t must be the training run's)")
    p.add_argument("--kernel_variant", type=int, default=0, help="as in audio_mps_amd.train")
    p.add_argument("--json", action="store_true", help="print the result as one JSON line as well")
    p.add_argument("--bankdir", default=None, metavar="DIR",
                   help="instead of --modeldir: a class bank that train --bank_by saved (bank.json with its classes + model.<m>.ckpt.npz, "
                        "either model), judged as a classifier on the dataset's labels; --per_clip then writes every clip's winning member "
                        "(int32, -1: undecided)")
    p.add_argument("--confusion", default=None, metavar="OUT.npy", help="with --bankdir: write the confusion matrix, int64 [M, M] "
                   "(row = the clip's class, column = the member that won it)")
    p.add_argument("--listen", action="store_true", help="with --bankdir: judge the bank as a STREAMING classifier (cmps_bank_posterior): "
                   "how many samples it hears before it is sure, and whether it is right then")
    p.add_argument("--threshold", type=float, default=0.99, metavar="P", help="with --listen: sure means the best member's posterior "
                   "probability reached P")
    p.add_argument("--temperature", type=float, default=1.0, help="with --listen: the members' total losses are divided by it")
    p.add_argument("--prior", default=None, metavar="P0,P1,...|empirical", help="with --listen: the members' prior probabilities, or "
                   "'empirical': the class counts bank.json holds (default: uniform)")
    p.add_argument("--calibrate", default=None, choices=["temperature", "prior", "both"],
                   help="with --bankdir: fit the temperature and (or) the prior of p_m ~ prior_m exp(-loss_m / temperature) on this dataset's "
                        "labelled clips (cmps_bank_calibrate), from --temperature and --prior as the start; the dataset should be held out")
    p.add_argument("--save_calibration", action="store_true", help="with --calibrate: write the fit into bank.json of --bankdir")
    p.add_argument("--calibrated", action="store_true", help="with --bankdir: take temperature and prior from the calibration bank.json "
                   "holds, instead of --temperature and --prior; without --listen also report the cross-entropy under them, xent_calibrated")
    p.add_argument("--listen_curve", default=None, metavar="OUT.npy", help="with --listen: write the accuracy of the best member after "
                   "every sample, float64 [steps]")
    return p


LISTEN_FRACTIONS = ((1, 16), (1, 8), (1, 4), (1, 2), (1, 1))


def _bank_and_dataset(args, backend):
    """(bank, load) of ``--bankdir``: the saved class bank, and ``load()`` -> the TFRecord file it is judged on as a ResidentDataset labelled
    by the bank's label key.  The file is only looked for here: a caller refuses what it can tell from the bank before it reads the file."""
    from .device_data import ResidentDataset
    from .sample import load_bank
    bank = load_bank(args.bankdir, args.sample_rate, args.hparams, args.kernel_variant, backend)
    if bank.classes is None or bank.label_key is None:
        raise ValueError(f"{args.bankdir} holds a bank without classes: --bankdir judges what train --bank_by saved")
    path = os.path.join(str(args.datadir), f"{args.dataset}.tfrecords")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    return bank, lambda: ResidentDataset.from_tfrecord(path, args.sample_duration, bank.backend, storage=args.storage, label_key=bank.label_key)


def listen_main(args, backend=None) -> dict:
    """``--bankdir --listen``: one pass of the dataset through ``bank.posterior_trace``, a batch of clips per scored bank stream.  Per batch
    ``best`` [B, steps] and the decisions come down once; the accuracy after every sample is counted here from ``best``."""
    from .sample import posterior_settings
    bank, load = _bank_and_dataset(args, backend)
    args.temperature, prior = posterior_settings(bank, args)
    ds = load()
    labels = ds.class_positions(bank.classes)
    steps = ds.clip_len - 1
    right = np.zeros(steps, dtype=np.int64)                              # labelled clips whose best member after step k is their own
    at, as_, n_lab = [], [], 0
    for first_id, batch in ds.ordered(args.minibatch_size):
        tr = bank.posterior_trace(batch, prior=prior, temperature=args.temperature, threshold=args.threshold)
        y = labels[first_id:first_id + tr.best.shape[0]]
        known = y >= 0
        right += np.sum(tr.best[known] == y[known, None], axis=0)
        n_lab += int(known.sum())
        at.append(tr.decided_at)
        as_.append(tr.decided_as)
    if not at:
        raise ValueError("evaluate --listen: the dataset yielded no batch")
    at, as_ = np.concatenate(at), np.concatenate(as_)
    known, decided = labels[:len(at)] >= 0, at >= 0
    both = known & decided
    curve = right / max(n_lab, 1)
    res = {"clips": int(len(at)), "labelled": n_lab, "threshold": float(args.threshold), "temperature": float(args.temperature),
           "decided": float(decided.mean()), "mean_decision_sample": float(at[decided].mean()) if decided.any() else None,
           "median_decision_sample": float(np.median(at[decided])) if decided.any() else None,
           "accuracy_at_decision": float(np.mean(as_[both] == labels[:len(at)][both])) if both.any() else None,
           "accuracy_after": {f"{a}/{b}": float(curve[max(steps * a // b, 1) - 1]) for a, b in LISTEN_FRACTIONS}}
    if args.listen_curve is not None:
        np.save(args.listen_curve, curve)
    fmt = lambda x: "-" if x is None else f"{x:.6g}"                       # noqa: E731
    print(f"listen {args.dataset}: decided={res['decided']:.4f} mean_sample={fmt(res['mean_decision_sample'])} "
          f"median_sample={fmt(res['median_decision_sample'])} accuracy_at_decision={fmt(res['accuracy_at_decision'])} "
          + " ".join(f"acc@{k}={v:.4f}" for k, v in res["accuracy_after"].items())
          + f" clips={res['clips']} threshold={args.threshold:g} temperature={args.temperature:g} storage={ds.storage}")
    if args.json:
        print(json.dumps({"dataset": args.dataset, "storage": ds.storage, **res}))
    return res


def bank_main(args, backend=None) -> ClassifierResult:
    """``--bankdir``: a saved class bank judged on a labelled TFRecord file (BankTrainer.evaluate_classifier)."""
    from .bank import BankTrainer
    from .sample import parse_prior, saved_calibration
    bank, load = _bank_and_dataset(args, backend)
    if args.calibrated:
        saved_calibration(bank, args.bankdir)              # (a bank.json without a calibration: a ValueError before anything is scored)
    ds = load()
    trainer = BankTrainer(bank)
    res = trainer.evaluate_classifier(ds, args.minibatch_size, keep_best=args.per_clip is not None)
    if args.per_clip is not None:
        np.save(args.per_clip, res.best)
    if args.confusion is not None:
        np.save(args.confusion, res.confusion)
    print(f"eval {args.dataset}: {res.line()} classes={len(res.classes)} unlabelled={res.n_unlabelled} storage={ds.storage}")
    extra = {}
    if args.calibrated:
        cal = bank.calibration
        extra["xent_calibrated"] = trainer.cross_entropy(ds, cal["temperature"], minibatch_size=args.minibatch_size, log_prior=cal["log_prior"])
        print(f"calibrated {args.dataset}: xent_calibrated={extra['xent_calibrated']:.6g} temperature={cal['temperature']:.6g} "
              f"(fitted on {cal['dataset']}, {cal['clips']} clips of T={cal['T']})")
    if args.calibrate is not None:
        cal = trainer.calibrate(ds, args.minibatch_size, fit=args.calibrate, temperature=args.temperature,
                                prior=parse_prior(args.prior, bank, args.bankdir))
        print(f"calibration {cal.line()}")
        for m, c in enumerate(res.classes):
            print(f"class {c!r}: prior {cal.prior[m]:.6g}" + (" (no held-out clip: not fitted)" if c in cal.unfitted else ""))
        extra["calibration"] = cal.scalars()
        if args.save_calibration:
            save_calibration(args.bankdir, cal.meta(args.dataset))
    if args.json:
        print(json.dumps({"dataset": args.dataset, "storage": ds.storage, **res.scalars(), **extra}))
    return res


def save_calibration(bankdir: str, calibration: dict):
    """Rewrite bank.json of ``bankdir`` with ``calibration`` under "calibration" and every other key as it was: a temporary file, then
    os.replace, as BankTrainer.save writes it."""
    path = os.path.join(bankdir, "bank.json")
    with open(path) as f:
        meta = json.load(f)
    meta["calibration"] = calibration
    tmp = os.path.join(bankdir, "bank.json.tmp")
    with open(tmp, "w") as f:
        json.dump(meta, f)
    os.replace(tmp, path)


def main(argv=None, backend=None) -> EvalResult:
    """``backend``: a scan backend to use instead of HipScan (CPU tests of the host logic inject one)."""
    from .device_data import ResidentDataset
    from .sample import build_model, load_variables
    args = build_parser().parse_args(argv)
    if args.sample_duration < 2 or args.minibatch_size < 1:
        raise ValueError("--sample_duration must be at least 2 and --minibatch_size positive")
    if (args.calibrate is not None or args.calibrated or args.save_calibration) and args.bankdir is None:
        raise ValueError("--calibrate, --save_calibration and --calibrated are a class bank's: they need --bankdir")
    if args.save_calibration and args.calibrate is None:
        raise ValueError("--save_calibration saves what --calibrate fitted: it needs --calibrate")
    if args.calibrated and (args.temperature != 1.0 or args.prior is not None):
        raise ValueError("--calibrated takes temperature and prior from bank.json: it goes with neither --temperature nor --prior")
    if args.calibrated and args.calibrate is not None:
        raise ValueError("--calibrated uses a saved calibration and --calibrate fits a new one: one at a time")
    if args.calibrate is not None and (args.listen or not args.temperature > 0.0):
        raise ValueError("--calibrate fits on whole clips: it does not go with --listen, and its start --temperature must be positive")
    if args.listen:
        if args.bankdir is None:
            raise ValueError("--listen judges a class bank: it needs --bankdir")
        if not (0.0 < args.threshold <= 1.0 and args.temperature > 0.0):
            raise ValueError("--listen needs --threshold in (0, 1] and --temperature > 0")
        return listen_main(args, backend)
    if args.bankdir is not None:
        return bank_main(args, backend)
    if args.confusion is not None:
        raise ValueError("--confusion is a class bank's (--bankdir)")
    model = build_model(load_variables(args.modeldir), args.sample_rate, args.hparams, args.kernel_variant, 0, backend)
    path = os.path.join(str(args.datadir), f"{args.dataset}.tfrecords")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    ds = ResidentDataset.from_tfrecord(path, args.sample_duration, model._get_backend(), storage=args.storage)
    res = evaluate(model, ds, args.minibatch_size, keep_losses=args.per_clip is not None)
    if args.per_clip is not None:
        np.save(args.per_clip, res.losses)
    print(f"eval {args.dataset}: loss={res.mean:.6f} per_sample={res.per_sample:.6g} std={res.std:.6g} sem={res.sem:.6g} "
          f"clips={res.n_clips} nonfinite={res.n_nonfinite} min={res.min:.6g} (clip {res.argmin}) max={res.max:.6g} (clip {res.argmax}) "
          f"storage={ds.storage}")
    if args.json:
        print(json.dumps({"dataset": args.dataset, "storage": ds.storage, **res.scalars()}))
    return res


if __name__ == "__main__":
    main()
