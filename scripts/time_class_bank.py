"""Time a class bank: its training step fed by ClassBatches, its classifier pass, k_classify_stats alone, and what a small bank learns.

  python scripts/time_class_bank.py [--out profiles/class_bank_times.json]

Per timed figure: 2 warm-ups, then 5 measurements, each the wall clock between two device synchronisations; the two methods of a comparison
alternate inside one run, on one stream.  Reported: the median of the five with [min, max].
  step        D = 8, B = 8, T = 16000, M = 64: one BankTrainer step fed by ResidentDataset.class_batches (64 classes of 16 clips) against the
              same step on one fixed, pre-uploaded [M, B, T] batch.  The gate is the project's own for device-side input: fed <= 1.05 x fixed.
              Also 600 consecutive steps of each (more than two plan blocks), unsynchronised but for the ends: the amortised cost with the
              planning included.
  classifier  the same bank: evaluate_classifier per batch against BankTrainer.evaluate per batch (M cmps_loss_stats launches) over a
              64-clip held-out set in batches of 8.  The new path must not lie above the old one by more than the old one's [min, max] spread.
  kernel      k_classify_stats alone (kernel events) at (M, B) = (64, 1024) and (1024, 64), and at (64, 8) next to the kernels of the bank
              forward it follows.  Recorded, not gated.
  learning    a 12-class PsiBank (D = 8, B = 8, T = 2048) on synthetic damped sines of 12 pitches (a semitone apart from 261.6 Hz, random
              onset and phase, 16-bit grid), 32 training and 16 held-out clips per pitch: held-out accuracy before training and after
              LEARN_STEPS steps.  Recorded only.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_mps_amd import HParams  # noqa: E402
from audio_mps_amd.bank import BankTrainer, PsiBank  # noqa: E402
from audio_mps_amd.device_data import ResidentDataset  # noqa: E402
from audio_mps_amd.scan import HipScan  # noqa: E402

WARMUP, REPS = 2, 5
D, B, T, M = 8, 8, 16000, 64
LEARN_STEPS = 300


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(a, b):
    ta, tb = [], []
    for rep in range(WARMUP + REPS):
        x, y = timed(a), timed(b)
        if rep >= WARMUP:
            ta.append(x)
            tb.append(y)
    return ta, tb


def summary(ts):
    return {"ms": ts, "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def step_and_classifier():
    hp = HParams(minibatch_size=B, bond_dim=D)
    be = HipScan(D)
    classes = list(range(M))
    bank = BankTrainer(PsiBank(hp, [{"seed": m} for m in range(M)], backend=be, classes=classes, label_key="pitch"))
    n = 16 * M
    data = ResidentDataset(be.damped_sine(1, 0, n, T, hp.delta_t), be, labels=np.arange(n) % M)
    stream = data.class_batches(classes, B, seed=0)
    fixed = stream().clone()

    def fed():
        bank.step(stream(), sync=False)

    def on_fixed():
        bank.step(fixed, sync=False)

    t_fed, t_fixed = alternate(fed, on_fixed)
    n_run = 600
    run_fixed = timed(lambda: [on_fixed() for _ in range(n_run)]) / n_run
    run_fed = timed(lambda: [fed() for _ in range(n_run)]) / n_run
    out = {"D": D, "B": B, "T": T, "M": M, "fed": summary(t_fed), "fixed": summary(t_fixed),
           "ratio_fed_over_fixed": statistics.median(t_fed) / statistics.median(t_fixed),
           "run_steps": n_run, "run_fed_ms_per_step": run_fed, "run_fixed_ms_per_step": run_fixed, "run_ratio": run_fed / run_fixed,
           "plan_blocks_uploaded": stream.uploads}
    print(f"step M={M}: fed {out['fed']['median_ms']:.3f} ms [{out['fed']['min_ms']:.3f}, {out['fed']['max_ms']:.3f}]  fixed "
          f"{out['fixed']['median_ms']:.3f} ms [{out['fixed']['min_ms']:.3f}, {out['fixed']['max_ms']:.3f}]  ratio "
          f"{out['ratio_fed_over_fixed']:.4f}; {n_run} steps in a row: fed {run_fed:.3f} fixed {run_fixed:.3f} ms/step", flush=True)

    held = ResidentDataset(be.damped_sine(2, 0, 64, T, hp.delta_t), be, labels=np.arange(64) % M)
    n_batches = 8
    t_new, t_old = alternate(lambda: bank.evaluate_classifier(held, 8), lambda: bank.evaluate(held, 8))
    t_new, t_old = [t / n_batches for t in t_new], [t / n_batches for t in t_old]
    be.kernel_events(True)
    bank.evaluate_classifier(held, 8)
    events = {k: {"ms_per_launch": v[0] / max(v[1], 1), "launches": v[1]} for k, v in be.kernel_times().items()}
    be.kernel_events(False)
    cls = {"M": M, "batch": 8, "batches": n_batches, "T": T, "classifier_per_batch": summary(t_new), "evaluate_per_batch": summary(t_old),
           "kernels_of_a_classifier_pass": events}
    print(f"classifier pass per batch: new {cls['classifier_per_batch']['median_ms']:.3f} ms  old "
          f"{cls['evaluate_per_batch']['median_ms']:.3f} ms [{min(t_old):.3f}, {max(t_old):.3f}]", flush=True)
    return out, cls


def kernel_alone():
    be = HipScan(D)
    rows = []
    for m, b in ((64, 1024), (1024, 64), (64, 8)):
        g = torch.Generator(device="cpu").manual_seed(m)
        loss = (torch.rand((m, b), generator=g) * 100.0).to(be.device)
        labels = torch.randint(0, m, (b,), generator=g, dtype=torch.int32).to(be.device)
        stats = be.classify_stats(loss, labels, 0)
        for _ in range(WARMUP):
            be.classify_stats(loss, labels, 0, stats)
        torch.cuda.synchronize()
        be.kernel_events(True)
        for _ in range(REPS):
            be.classify_stats(loss, labels, 0, stats)
        ms, count = be.kernel_times()["k_classify_stats"][:2]
        be.kernel_events(False)
        rows.append({"M": m, "B": b, "k_classify_stats_ms": ms / count, "launches": count})
        print(f"k_classify_stats M={m} B={b}: {ms / count:.4f} ms", flush=True)
    return rows


def pitched_sines(n_per, pitches, length, dt, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(length) * dt
    clips, labels = [], []
    for k in range(pitches):
        f = 261.6 * 2.0 ** (k / 12.0)
        for _ in range(n_per):
            onset, phase = rng.uniform(0.0, 0.2) * length * dt, rng.uniform(0.0, 2 * np.pi)
            s = t - onset
            x = np.where(s >= 0, np.sin(2 * np.pi * f * s + phase) * np.exp(-np.maximum(s, 0.0) / 0.1), 0.0)
            clips.append(np.round(0.5 * x * 32768.0).astype(np.int16))
            labels.append(k)
    return np.stack(clips), np.array(labels, dtype=np.int64)


def learning():
    P, Tl = 12, 2048
    hp = HParams(minibatch_size=8, bond_dim=8)
    be = HipScan(8)
    bank = BankTrainer(PsiBank(hp, [{"seed": m} for m in range(P)], backend=be, classes=list(range(P)), label_key="pitch"))
    clips, labels = pitched_sines(32, P, Tl, hp.delta_t, 1)
    hclips, hlabels = pitched_sines(16, P, Tl, hp.delta_t, 2)
    train, held = ResidentDataset(clips, be, storage="int16", labels=labels), ResidentDataset(hclips, be, storage="int16", labels=hlabels)
    stream = train.class_batches(list(range(P)), 8, seed=0)
    before = bank.evaluate_classifier(held, 64)
    for _ in range(LEARN_STEPS):
        bank.step(stream(), sync=False)
    after = bank.evaluate_classifier(held, 64)
    out = {"classes": P, "D": 8, "B": 8, "T": Tl, "steps": LEARN_STEPS, "train_clips": int(labels.size), "held_out_clips": int(hlabels.size),
           "before": before.scalars(), "after": after.scalars()}
    print(f"learning: 12 pitches, {LEARN_STEPS} steps: held-out {before.line()} -> {after.line()}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "class_bank_times.json"))
    args = ap.parse_args()
    step, cls = step_and_classifier()
    gc.collect()
    torch.cuda.empty_cache()
    kern = kernel_alone()
    learn = learning()
    old = cls["evaluate_per_batch"]
    cond = {"fed_step_within_1.05_of_fixed": step["ratio_fed_over_fixed"] <= 1.05,
            "classifier_pass_within_old_spread": cls["classifier_per_batch"]["median_ms"] <= old["median_ms"] + (old["max_ms"] - old["min_ms"])}
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "step": step, "classifier": cls, "k_classify_stats": kern,
           "learning": learn, "conditions": cond}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(cond))


if __name__ == "__main__":
    main()
