#!/usr/bin/env python3
"""Kernel time of a primed sampler run next to the unprimed sampler over the same number of steps (CMPS_OPT_KERNEL_EVENTS).

usage: python scripts/time_primed_sampler.py [--D 32] [--n 64] [--P 16000] [--length 16000] [--reps 5] [--out FILE]

A forced step does the work of a sampled one, so k_sample_*_primed over P + length steps should cost what k_sample_* costs over
P + length steps.  Writes one JSON record (the median and every repetition, milliseconds) to --out and to stdout."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sampler_entry(times):
    """(name, ms) of the one k_sample_* kernel among the recorded ones"""
    hits = [(k, ms) for k, (ms, _) in times.items() if k.startswith("k_sample_")]
    assert len(hits) == 1, times
    return hits[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--P", type=int, default=16000)
    ap.add_argument("--length", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    from oracle import cmps_oracle as O
    hp = HParams(minibatch_size=a.n, bond_dim=a.D, sigma=1.0, A=10.0)
    be = HipScan(a.D, variant=a.variant)
    m = PsiCMPS(hp, seed=a.D, backend=be)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    total = a.P + a.length
    ohp = O.HParams(**hp.values())
    noise = O.sample_noise(ohp, a.n, total, temp=0.5, seed=1)
    prime = O.damped_sine(a.n, a.P + 1, hp.delta_t, seed=2)
    be.kernel_events(True)
    rec = {"primed": [], "primed_with_pred": [], "unprimed": []}
    for rep in range(a.reps + 1):                      # the first repetition warms up (code object load, tables)
        m.sample(a.n, total, noise=noise)
        t_u = be.kernel_times()
        m.sample(a.n, a.length, noise=noise[a.P:], prime=prime)
        t_p = be.kernel_times()
        m.sample(a.n, a.length, noise=noise[a.P:], prime=prime, return_pred=True)
        t_q = be.kernel_times()
        if rep:
            (ku, mu), (kp, mp), (_, mq) = (sampler_entry(t) for t in (t_u, t_p, t_q))
            rec["unprimed"].append(mu)
            rec["primed"].append(mp)
            rec["primed_with_pred"].append(mq)
    med = {k: statistics.median(v) for k, v in rec.items()}
    out = {"what": "kernel time (HIP events around the launch, CMPS_OPT_KERNEL_EVENTS), milliseconds",
           "device": torch.cuda.get_device_name(0), "D": a.D, "n": a.n, "P": a.P, "length": a.length, "steps": total,
           "kernels": {"unprimed": ku, "primed": kp}, "median_ms": med, "all_ms": rec,
           "us_per_step": {k: 1e3 * v / total for k, v in med.items()},
           "primed_over_unprimed": med["primed"] / med["unprimed"]}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
