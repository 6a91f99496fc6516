#!/usr/bin/env python3
"""Milliseconds per full RhoCMPS training step with the host optimiser (gradient sums to the host, chain rule and Adam in numpy,
parameters and columns uploaded again) and with the device-resident step (cmps_rho_apply_step).

usage: python scripts/time_rho_step.py [--shapes 32:32,64:16] [--T 1000] [--B 256] [--steps 20] [--rounds 7] [--only host] [--out FILE]

Both settings run in the same process on the same clips (resident on the GPU), interleaved: every round times `--steps` host-optimiser
steps and then `--steps` device steps, each block with a host clock that ends in a device synchronise; the figure of a setting is the
median over the rounds.  The device steps run with sync=False; "device_enqueue" is the host time such a block took BEFORE that final
synchronise -- a step that waited on the host anywhere could not leave the host ahead of the GPU.
--only host times the host optimiser alone (it needs nothing of the device step: the figure of an older checkout).
Writes one JSON record to --out and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_trainer(D, rank, B, T, device_step, audio):
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=rank)
    m = RhoCMPS(hp, data_iterator=audio, seed=2, backend=HipScan(D))
    if D > 32:                                          # (the scale scripts/bench_next_rows.py times this shape at)
        m.variables["Rx"] *= np.float32(0.5)
        m.variables["Ry"] *= np.float32(0.5)
    return Trainer(m, hp, device_step=True) if device_step else Trainer(m, hp)


def block(trainer, steps, sync):
    """(ms per step with the final synchronise, ms per step the host needed to issue the steps)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = trainer.step(sync=sync)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return 1e3 * (t2 - t0) / steps, 1e3 * (t1 - t0) / steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:32,64:16", help="D:rank,...")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["host"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from oracle import cmps_oracle as O
    rows = {}
    for spec in a.shapes.split(","):
        D, rank = (int(x) for x in spec.split(":"))
        rng = np.random.default_rng(12347)
        clips = (O.damped_sine(a.B, a.T, 1.0 / 16000, seed=2) + 0.02 * rng.standard_normal((a.B, a.T))).astype(np.float32)
        audio = torch.from_numpy(clips).cuda()
        settings = ["host"] if a.only else ["host", "device"]
        tr = {s: make_trainer(D, rank, a.B, a.T, s == "device", audio) for s in settings}
        rec = {s: [] for s in settings}
        enq = []
        for rnd in range(a.rounds + 1):                 # the first round warms up (code objects, workspaces, pinned buffers)
            for s in settings:
                ms, ms_issue, out = block(tr[s], a.steps, sync=(s == "host"))
                if rnd:
                    rec[s].append(ms)
                    if s == "device":
                        enq.append(ms_issue)
        last = {s: tr[s].step(sync=True)["total_loss"] for s in settings}
        assert all(np.isfinite(v) for v in last.values()), last
        row = {"shape": f"D={D}, rank={rank}, T={a.T}, B={a.B}, full training step", "steps_per_block": a.steps, "rounds": a.rounds,
               "median_ms_per_step": {s: statistics.median(v) for s, v in rec.items()}, "all_ms_per_step": rec,
               "total_loss_after": last}
        if not a.only:
            med = row["median_ms_per_step"]
            row["device_over_host"] = med["device"] / med["host"]
            row["host_over_device"] = med["host"] / med["device"]
            row["device_enqueue_ms_per_step"] = statistics.median(enq)
        rows[f"rho_step_d{D}_rank{rank}"] = row
        del tr
    out = {"what": "wall time of Trainer.step for RhoCMPS (host clock around blocks of steps, ending in a device synchronise), "
                   "milliseconds per step; host = numpy chain rule + Adam, device = cmps_rho_apply_step with sync=False",
           "device": torch.cuda.get_device_name(0), "settings": "host only" if a.only else "interleaved in one process", "rows": rows}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
