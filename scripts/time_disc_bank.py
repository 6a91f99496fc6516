"""Time the cross-entropy step of a class bank against the generative step, and record what discriminative fine-tuning does to a small bank.

  python scripts/time_disc_bank.py [--out profiles/disc_bank_times.json]

Per timed figure: 2 warm-ups, then 5 measurements, each the wall clock between two device synchronisations; the two methods alternate inside
one run, on one stream.  Reported: the median of the five with [min, max].
  step      D = 8, B = 8, T = 16000, M = 64: BankTrainer.step_classifier against BankTrainer.step on the same shared, pre-uploaded [B, T] batch
            (sync=False both).  The new step adds one k_classify_weights launch and the weight reads of the reduction; the gate is the
            1.05 x the project uses for a step's feeding: step_classifier <= 1.05 x step.
  kernels   kernel events of one step of each kind, and k_classify_stats on the same [M, B] losses next to k_classify_weights.  Recorded.
  learning  the 12-pitch experiment of scripts/time_class_bank.py (D = 8, B = 8, T = 2048, 32 training and 16 held-out clips per pitch):
            300 generative steps on class_batches, then -- from that checkpoint, once per entry of SETTINGS (temperature, gen_weight,
            disc_weight) -- FINE_STEPS steps of step_classifier on labelled_batches of FINE_BATCH clips.  Held-out accuracy and
            cross-entropy (always judged at temperature 1) before, after the generative steps and after each fine-tuning.  Recorded only.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audio_mps_amd import HParams  # noqa: E402
from audio_mps_amd.bank import BankTrainer, PsiBank  # noqa: E402
from audio_mps_amd.device_data import ResidentDataset  # noqa: E402
from audio_mps_amd.scan import HipScan  # noqa: E402
from time_class_bank import LEARN_STEPS, alternate, pitched_sines, summary  # noqa: E402

D, B, T, M = 8, 8, 16000, 64
FINE_STEPS, FINE_BATCH = 300, 24


def events_of(be, fn):
    be.kernel_events(True)
    fn()
    out = {k: {"ms_per_launch": v[0] / max(v[1], 1), "launches": v[1]} for k, v in be.kernel_times().items()}
    be.kernel_events(False)
    return out


def step():
    hp = HParams(minibatch_size=B, bond_dim=D)
    be = HipScan(D)
    bank = BankTrainer(PsiBank(hp, [{"seed": m} for m in range(M)], backend=be, classes=list(range(M)), label_key="pitch"))
    batch = be.damped_sine(1, 0, B, T, hp.delta_t)
    labels = torch.from_numpy((np.arange(B) * 7 % M).astype(np.int32)).to(be.device)
    kw = dict(gen_weight=0.0, disc_weight=1.0, temperature=float(T), sync=False)
    t_disc, t_gen = alternate(lambda: bank.step_classifier(batch, labels, **kw), lambda: bank.step(batch, sync=False))
    ev_disc = events_of(be, lambda: bank.step_classifier(batch, labels, **kw))
    ev_gen = events_of(be, lambda: bank.step(batch, sync=False))
    loss = be.bank_forward(batch, save_for_bwd=False)
    ev_stats = events_of(be, lambda: [be.classify_stats(loss, labels, 0) for _ in range(5)])
    ev_weights = events_of(be, lambda: [be.classify_weights(loss, labels, 1.0 / T, 0.0, 1.0) for _ in range(5)])
    out = {"D": D, "B": B, "T": T, "M": M, "temperature": float(T), "step_classifier": summary(t_disc), "step": summary(t_gen),
           "ratio_classifier_over_step": statistics.median(t_disc) / statistics.median(t_gen),
           "kernels_of_a_classifier_step": ev_disc, "kernels_of_a_generative_step": ev_gen,
           "k_classify_stats_ms": ev_stats["k_classify_stats"]["ms_per_launch"],
           "k_classify_weights_ms": ev_weights["k_classify_weights"]["ms_per_launch"]}
    print(f"step M={M}: classifier {out['step_classifier']['median_ms']:.3f} ms [{min(t_disc):.3f}, {max(t_disc):.3f}]  generative "
          f"{out['step']['median_ms']:.3f} ms [{min(t_gen):.3f}, {max(t_gen):.3f}]  ratio {out['ratio_classifier_over_step']:.4f}; "
          f"k_classify_weights {out['k_classify_weights_ms']:.4f} ms  k_classify_stats {out['k_classify_stats_ms']:.4f} ms", flush=True)
    return out


SETTINGS = ((1.0, 1.0, 1.0), (1.0, 0.0, 1.0), (2048.0, 0.0, 1.0))      # (temperature, gen_weight, disc_weight) of a fine-tuning run


def learning():
    import tempfile
    P, Tl = 12, 2048
    hp = HParams(minibatch_size=8, bond_dim=8)
    classes = list(range(P))

    def new_bank():
        return BankTrainer(PsiBank(hp, [{"seed": m} for m in range(P)], backend=HipScan(8), classes=classes, label_key="pitch"))
    bank = new_bank()
    be = bank.bank.backend
    clips, labels = pitched_sines(32, P, Tl, hp.delta_t, 1)
    hclips, hlabels = pitched_sines(16, P, Tl, hp.delta_t, 2)
    train, held = ResidentDataset(clips, be, storage="int16", labels=labels), ResidentDataset(hclips, be, storage="int16", labels=hlabels)
    stream = train.class_batches(classes, 8, seed=0)
    before = bank.evaluate_classifier(held, 64)
    for _ in range(LEARN_STEPS):
        bank.step(stream(), sync=False)
    generative = bank.evaluate_classifier(held, 64)
    print(f"learning: held-out {before.line()}\n  after {LEARN_STEPS} generative steps: {generative.line()}", flush=True)
    runs = []
    with tempfile.TemporaryDirectory() as ckpt:
        bank.save(ckpt)
        for temperature, gen_weight, disc_weight in SETTINGS:          # every run starts from the generatively trained bank
            tuned = new_bank()
            assert tuned.restore(ckpt)
            shared = train.labelled_batches(classes, FINE_BATCH, seed=0, order="estimator")
            xent = []
            for it in range(FINE_STEPS):
                batch, lab = shared()
                log = it % 50 == 0 or it == FINE_STEPS - 1
                out = tuned.step_classifier(batch, lab, gen_weight=gen_weight, disc_weight=disc_weight, temperature=temperature, sync=log)
                if log:
                    xent.append({"step": it, "xent": out["xent"], "used": out["used"]})
            res = tuned.evaluate_classifier(held, 64)
            runs.append({"temperature": temperature, "gen_weight": gen_weight, "disc_weight": disc_weight, "after_fine_tuning": res.scalars(),
                         "training_xent_at_temperature": xent})
            print(f"  after {FINE_STEPS} more steps of step_classifier, temperature {temperature:g} gen_weight {gen_weight:g} disc_weight "
                  f"{disc_weight:g}: {res.line()}", flush=True)
    return {"classes": P, "D": 8, "T": Tl, "generative_steps": LEARN_STEPS, "generative_batch_per_class": 8, "fine_tuning_steps": FINE_STEPS,
            "fine_tuning_batch": FINE_BATCH, "train_clips": int(labels.size), "held_out_clips": int(hlabels.size), "before": before.scalars(),
            "after_generative": generative.scalars(), "fine_tuning": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "disc_bank_times.json"))
    args = ap.parse_args()
    st = step()
    learn = learning()
    cond = {"step_classifier_within_1.05_of_step": st["ratio_classifier_over_step"] <= 1.05}
    out = {"device": torch.cuda.get_device_name(0), "warmup": 2, "reps": 5, "step": st, "learning": learn, "conditions": cond}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(cond))


if __name__ == "__main__":
    main()
