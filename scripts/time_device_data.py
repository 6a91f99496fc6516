#!/usr/bin/env python3
"""What feeding a training step from the host costs, and what producing the batch on the device costs instead.

usage: python scripts/time_device_data.py [--out profiles/device_data_times.json] [--reps 5] [--warmup 2] [--steps 20]

Shape: D = 32, T = 16000, 1024 clips per batch, one GPU, PsiCMPS with the device-resident optimiser step (the shape bench.py times).

1. Kernel times.  CMPS_OPT_KERNEL_EVENTS milliseconds of k_damped_sine (one batch) and of k_batch_gather twice -- 1024 random rows out of
   4096 clips of 16000 samples, uncropped, and out of 4096 clips of 64000 samples with random crops of 16000 (source rows at any 4-byte
   alignment) -- each next to torch's device-to-device copy_ of the same 65.5 MB, bracketed by two events in the same run.  Launches
   alternate; --warmup of each are discarded, the median of --reps is kept.  GATE: uncropped gather <= 1.5 x the copy.
2. Step times.  --steps training steps (sync=False, one synchronisation at the end), wall clock between two synchronisations, five ways:
     fixed          one pre-uploaded batch, every step (the floor; what bench.py times)
     device_sine    DampedSineSource: the batch generated on the device every step
     device_gather  ResidentDataset: the batch gathered from the resident dataset every step
     host_sine      data.damped_sine in numpy every step, uploaded (what `--dataset damped_sine` does without --device_data)
     host_tfrecord  tfrecord.audio_batches every step, uploaded (what a TFRecord dataset does without --device_data; the file is in the
                    page cache)
   The five alternate inside every repetition; --warmup repetitions are discarded, the median of --reps is kept.
   GATE: device_sine and device_gather within 5 % of fixed.
A missed gate is recorded (under "gates"), not an error.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, T, B, N_CLIPS, LONG = 32, 16000, 1024, 4096, 64000


def _stats(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med, "all_ms": list(ms)}


def kernel_times(be, reps, warmup):
    """{name: stats} of the three launches and of the copy next to each."""
    import numpy as np
    import torch
    dev = be.device
    rng = np.random.default_rng(0)
    out = {}

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def kernel_ms(fn, name):
        fn()
        (ms, calls), = [v for k, v in be.kernel_times().items() if k == name]
        assert calls == 1
        return ms

    src = torch.empty((B, T), dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    cases = []
    for label, L in (("gather_uncropped", T), ("gather_cropped_from_64000", LONG)):
        data = torch.empty((N_CLIPS, L), dtype=torch.float32, device=dev).normal_()
        index = torch.from_numpy(rng.integers(0, N_CLIPS, size=B).astype(np.int32)).to(dev)
        offset = None if L == T else torch.from_numpy(rng.integers(0, L - T + 1, size=B).astype(np.int32)).to(dev)
        cases.append((label, "k_batch_gather", 2, (lambda data=data, index=index, offset=offset: be.gather_batch(data, index, offset, T=T))))
    cases.append(("damped_sine", "k_damped_sine", 1, lambda: be.damped_sine(1, 0, B, T, 1.0 / 16000)))      # (written only)
    be.kernel_events(True)
    try:
        for label, name, passes, fn in cases:
            k, c = [], []
            for rep in range(warmup + reps):
                a, b = kernel_ms(fn, name), event_ms(lambda: dst.copy_(src))
                if rep >= warmup:
                    k.append(a)
                    c.append(b)
            out[label] = {"kernel": name, **_stats(k), "copy_same_bytes": _stats(c), "kernel_over_copy": statistics.median(k) / statistics.median(c),
                          "bytes_moved": passes * 4 * B * T, "GBps": passes * 4 * B * T / statistics.median(k) / 1e6}
    finally:
        be.kernel_events(False)
    return out


def step_times(be, steps, reps, warmup, workdir):
    import numpy as np
    import torch
    from audio_mps_amd import HParams, PsiCMPS, data as host_data, tfrecord
    from audio_mps_amd.device_data import DampedSineSource, ResidentDataset
    from audio_mps_amd.train import Trainer
    hp = HParams(minibatch_size=B, bond_dim=D)
    trainer = Trainer(PsiCMPS(hp, seed=0, backend=be), hp, device_step=True)
    sine = DampedSineSource(be, B, T, hp.delta_t, seed=0)
    # the dataset: 4096 of the device's own damped sines, written as the reference's TFRecord file and read back both ways
    path = os.path.join(workdir, "sines.tfrecords")
    t0 = time.perf_counter()
    tfrecord.write_audio_tfrecord(path, be.damped_sine(7, 0, N_CLIPS, T, hp.delta_t).cpu().numpy())
    t_write = time.perf_counter() - t0
    t0 = time.perf_counter()
    resident = ResidentDataset.from_tfrecord(path, T, be)
    torch.cuda.synchronize()
    t_load = time.perf_counter() - t0
    gather = resident.batches(B, seed=0, order="data")
    host_batches = tfrecord.audio_batches(path, B, T, seed=0, order="data")
    fixed = sine.next(0)
    count = {"host_sine": 0, "device_sine": 0}

    def next_of(mode):
        if mode == "fixed":
            return fixed
        if mode == "device_gather":
            return gather()
        if mode == "host_tfrecord":
            return host_batches()
        count[mode] += 1
        if mode == "device_sine":
            return sine.next(count[mode])
        return host_data.damped_sine(B, T, hp.delta_t, seed=count[mode])

    modes = ["fixed", "device_sine", "device_gather", "host_sine", "host_tfrecord"]
    ms = {m: [] for m in modes}
    for rep in range(warmup + reps):
        for mode in modes:                                      # alternating: all five see the same machine
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                trainer.step(next_of(mode), sync=False, global_batch=B)
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[mode].append(1e3 * (time.perf_counter() - t0) / steps)
    loss = float(trainer._dev["losses"].cpu().numpy()[0])
    return {m: _stats(v) for m, v in ms.items()}, {"tfrecord_write_s": t_write, "resident_load_s": t_load, "last_model_loss": loss,
                                                   "finite": bool(np.isfinite(loss))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_data_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    kernels = kernel_times(be, a.reps, a.warmup)
    with tempfile.TemporaryDirectory() as workdir:
        steps, aside = step_times(be, a.steps, a.reps, a.warmup, workdir)
    floor = steps["fixed"]["median_ms"]
    over = {m: steps[m]["median_ms"] / floor for m in steps}
    gates = {"gather_uncropped_within_1.5x_copy": {"value": kernels["gather_uncropped"]["kernel_over_copy"], "limit": 1.5},
             "device_sine_within_5pct_of_fixed": {"value": over["device_sine"], "limit": 1.05},
             "device_gather_within_5pct_of_fixed": {"value": over["device_gather"], "limit": 1.05}}
    for g in gates.values():
        g["met"] = bool(g["value"] <= g["limit"])
    doc = {"what": "kernels: CMPS_OPT_KERNEL_EVENTS milliseconds per launch next to torch's device-to-device copy_ of the same bytes (two "
                   "events); steps: wall-clock milliseconds per training step (host clock between two device synchronisations around "
                   f"{a.steps} steps with sync=False), by where the batch comes from",
           "device": "MI355X (gfx950); torch.cuda.get_device_name: " + torch.cuda.get_device_name(0),
           "shape": {"D": D, "T": T, "clips_per_batch": B, "batch_bytes": 4 * B * T, "dataset_clips": N_CLIPS, "long_clip": LONG},
           "reps": a.reps, "warmup": a.warmup, "steps_per_run": a.steps,
           "kernels": kernels, "steps": steps, "step_over_fixed": over, "gates": gates, "aside": aside}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for label, k in kernels.items():
        print(f"{label}: {k['kernel']} {k['median_ms']:.4f} ms, copy {k['copy_same_bytes']['median_ms']:.4f} ms, ratio {k['kernel_over_copy']:.2f}")
    for m in steps:
        print(f"step fed by {m}: {steps[m]['median_ms']:.3f} ms (spread {steps[m]['spread']:.2f}), {over[m]:.3f} x fixed")
    print("gates:", {k: (round(g["value"], 3), g["met"]) for k, g in gates.items()})
    return 0 if aside["finite"] else 1


if __name__ == "__main__":
    sys.exit(main())
