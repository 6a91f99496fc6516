"""Time one training step of a bank of M RhoCMPS models against a Python loop over M plain device-resident RhoCMPS steps.

  python scripts/time_rho_bank.py [--out profiles/rho_bank_times.json]

Settings: D = 8, rank 8, B = 8, T = 16000 (the reference's own minibatch_size = 8, bond_dim = 8, rank = bond_dim) with M in {1, 8, 64},
and D = 32, rank 32, B = 8, M = 16.  Per setting and method: 2 warm-up steps, then 5 timed ones, each the wall clock between two device
synchronisations; the two methods alternate inside one run, on one stream, on the same batch.  Reported: the median of the five, their
min and max, and the ratio loop / bank.  The one condition, judged against the loop measured here and never against an expectation:
the bank at M = 1 lies inside [min, max] of the five plain measurements.
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

from audio_mps_amd import HParams, RhoCMPS  # noqa: E402
from audio_mps_amd.bank import BankTrainer, RhoBank  # noqa: E402
from audio_mps_amd.scan import HipScan  # noqa: E402
from audio_mps_amd.train import Trainer  # noqa: E402

#            D  rank B    T     M
SETTINGS = [(8, 8, 8, 16000, 1), (8, 8, 8, 16000, 8), (8, 8, 8, 16000, 64), (32, 32, 8, 16000, 16)]
WARMUP, REPS = 2, 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(D, rank, B, T, M):
    hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=rank)
    audio = HipScan(D).damped_sine(1, 0, B, T, hp.delta_t)           # the device's synthetic damped-sine clips (cmps_damped_sine_fill)
    members = [{"seed": m} for m in range(M)]
    bank = BankTrainer(RhoBank(hp, members, backend=HipScan(D)))
    assert bank.native
    plain = [Trainer(RhoCMPS(hp, seed=m, backend=HipScan(D)), hp, device_step=True) for m in range(M)]

    def loop():
        for tr in plain:
            tr.step(audio, sync=False)

    def banked():
        bank.step(audio, sync=False)

    t_loop, t_bank = [], []
    for rep in range(WARMUP + REPS):
        a, b = timed(loop), timed(banked)
        if rep >= WARMUP:
            t_loop.append(a)
            t_bank.append(b)
    lo = bank.step(audio, sync=True)
    ref = [tr.step(audio, sync=True) for tr in plain]
    same = all(np.float32(r["model_loss"]).tobytes() == lo["model_loss"][m].tobytes() for m, r in enumerate(ref))       # the two methods ran the same steps
    med_l, med_b = statistics.median(t_loop), statistics.median(t_bank)
    return {"D": D, "rank": rank, "B": B, "T": T, "M": M, "loop_ms": t_loop, "bank_ms": t_bank, "loop_median_ms": med_l, "bank_median_ms": med_b,
            "loop_min_ms": min(t_loop), "loop_max_ms": max(t_loop), "ratio_loop_over_bank": med_l / med_b, "losses_bit_equal": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "rho_bank_times.json"))
    args = ap.parse_args()
    rows = []
    for D, rank, B, T, M in SETTINGS:
        rows.append(measure(D, rank, B, T, M))
        r = rows[-1]
        print(f"D={D} rank={rank} B={B} T={T} M={M}: loop {r['loop_median_ms']:.3f} ms [{r['loop_min_ms']:.3f}, {r['loop_max_ms']:.3f}]  "
              f"bank {r['bank_median_ms']:.3f} ms  loop/bank {r['ratio_loop_over_bank']:.2f}  bit-equal {r['losses_bit_equal']}", flush=True)
        gc.collect()                                                 # (a stepped model and its trainer hold each other: free the workspaces now)
        torch.cuda.empty_cache()
    by = {(r["D"], r["M"]): r for r in rows}
    cond = {"bank_M1_within_plain_spread": by[(8, 1)]["loop_min_ms"] <= by[(8, 1)]["bank_median_ms"] <= by[(8, 1)]["loop_max_ms"]}
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "settings": rows, "conditions": cond}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(cond))


if __name__ == "__main__":
    main()
