#!/usr/bin/env python3
"""RhoCMPS sampler timings at D = 32.

usage: python scripts/time_rho_sample.py [--root DIR] [--n 64] [--P 1000] [--length 1000] [--reps 5] [--inner 20] [--out FILE]

First the host-timed rows of earlier rounds (rank 4 and 32, 8 paths x 2000 steps, noise upload and waveform download included).  Then
device-event times of the sampler entry alone at rank 32 with everything resident (`inner` calls per event pair, median of `reps`):
cmps_rho_sample over P + length steps, and cmps_rho_sample_primed as P + length, (P + length - 1) + 1 (all but one step forced) and
1 + (P + length - 1) (all but one step sampled), so the per-step cost of a forced step stands next to that of a sampled one.
--root selects the checkout the package is imported from (default: the one this script is in): run against a checkout without
cmps_rho_sample_primed, the unprimed rows alone are measured -- alternate the two trees in one session to compare them.  Writes one JSON record to --out and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.abspath(_pre.parse_known_args()[0].root))
import numpy as np, torch
from audio_mps_amd import HParams, RhoCMPS


def host_rows():
    for rank in (4, 32):
        hp = HParams(minibatch_size=8, bond_dim=32, initial_rank=rank, sigma=0.05)
        m = RhoCMPS(hp, seed=2)
        n, length = 8, 2000
        noise = (0.05 * np.sqrt(hp.delta_t) * np.random.default_rng(0).standard_normal((length, n))).astype(np.float32)
        m.sample(n, length, noise=noise)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m.sample(n, length, noise=noise)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        print(f"rank {rank}: sample({n} paths x {length} steps) {dt*1e3:.2f} ms -> {dt/length*1e6:.2f} us/step", file=sys.stderr)


def device_rows(a):
    """{row: [ms per call, ...]} of the sampler entries alone, rank 32"""
    hp = HParams(minibatch_size=a.n, bond_dim=32, initial_rank=32, sigma=0.05)
    m = RhoCMPS(hp, seed=2)
    n, steps = a.n, a.P + a.length
    be = m._prepare(n, steps + 1, train=False)
    lib, h, dev = be._lib, be._h, be.device
    rng = np.random.default_rng(0)
    noise = torch.from_numpy((0.05 * np.sqrt(hp.delta_t) * rng.standard_normal((n, steps))).astype(np.float32)).to(dev)
    t = np.arange(steps + 1, dtype=np.float32) * np.float32(hp.delta_t)
    prime = torch.from_numpy((0.1 * np.sin(2 * np.pi * 261.6 * t) * np.exp(-t / 0.1)).astype(np.float32)).to(dev)      # one clip, shared
    out = torch.empty((n, steps), dtype=torch.float32, device=dev)
    pred = torch.empty((n, steps), dtype=torch.float32, device=dev)
    calls = {"unprimed": lambda: lib.cmps_rho_sample(h, noise.data_ptr(), n, steps, out.data_ptr(), 0, be._stream())}
    if hasattr(lib, "cmps_rho_sample_primed"):
        def primed(P):
            return lambda: lib.cmps_rho_sample_primed(h, prime.data_ptr(), 1, P + 1, noise.data_ptr(), n, steps - P, out.data_ptr(),
                                                      pred.data_ptr(), 0, be._stream())
        calls.update({"primed": primed(a.P), "primed_forced": primed(steps - 1), "primed_sampled": primed(1)})
    rec = {k: [] for k in calls}
    for rep in range(a.reps + 1):                      # the first repetition warms up (code object load)
        for k, f in calls.items():                     # (rows interleaved within a repetition)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(dev))
            for _ in range(a.inner):
                assert f() == 0
            e1.record(torch.cuda.current_stream(dev))
            torch.cuda.synchronize(dev)
            if rep:
                rec[k].append(e0.elapsed_time(e1) / a.inner)
    return rec, steps


def main():
    ap = argparse.ArgumentParser(parents=[_pre])
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--P", type=int, default=1000)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no_host_rows", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.no_host_rows:
        host_rows()
    rec, steps = device_rows(a)
    med = {k: statistics.median(v) for k, v in rec.items()}
    out = {"what": "device-event time of one sampler call (cmps_rho_sample / cmps_rho_sample_primed), milliseconds, everything resident",
           "device": torch.cuda.get_device_name(0), "D": 32, "rank": 32, "n": a.n, "P": a.P, "length": a.length, "steps": steps,
           "calls_per_event_pair": a.inner, "median_ms": med, "all_ms": rec, "us_per_step": {k: 1e3 * v / steps for k, v in med.items()}}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
