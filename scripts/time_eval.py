#!/usr/bin/env python3
"""What held-out evaluation costs: the int16 gather next to the float32 gather, and the evaluation loop next to its forward scans.

usage: python scripts/time_eval.py [--out profiles/eval_times.json] [--reps 5] [--warmup 2]

The method of scripts/time_device_data.py: --warmup repetitions discarded, the median of --reps kept, wall clock between two device
synchronisations, CMPS_OPT_KERNEL_EVENTS milliseconds for the kernels.  One GPU.

(a) The gathers.  k_batch_gather_i16 and k_batch_gather, alternating in the same run: 1024 rows of 16000 samples cut at random starts out of
    4096 clips of 64000 samples (sources at any 2-byte / 4-byte address), the int16 dataset holding the float32 one's values.  The int16
    kernel moves 0.75 times the bytes (2 + 4 per sample against 4 + 4).  GATE: int16 <= 1.25 x float32 (at about 26 us a few us of jitter
    is that much).
(b) The loop.  evaluate() over 4096 clips of 16000 samples at D = 32, minibatch 1024 (4 batches), from float32 and from int16 storage:
    wall-clock milliseconds per batch, and -- from one more pass with the kernel events on, outside the timed ones -- each kernel's own
    milliseconds per batch.  "loop_adds_ms_per_batch" is the wall clock minus the forward scan's kernels: gather, cmps_loss_stats, launches
    and the one 64-byte download, spread over the batches.
A missed gate is recorded (under "gates"), not an error.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, T, B, N_CLIPS, LONG = 32, 16000, 1024, 4096, 64000


def _stats(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med, "all_ms": list(ms)}


def _pcm(x):
    """A float32 device tensor -> (int16 PCM, the float32 tensor holding exactly its values)."""
    import torch
    i = torch.round(x * 32768.0).clamp_(-32768.0, 32767.0).to(torch.int16)
    return i, i.to(torch.float32) * 2.0 ** -15


def gather_times(be, reps, warmup):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    i16, f32 = _pcm(torch.empty((N_CLIPS, LONG), dtype=torch.float32, device=be.device).normal_(std=0.2))
    index = torch.from_numpy(rng.integers(0, N_CLIPS, size=B).astype(np.int32)).to(be.device)
    offset = torch.from_numpy(rng.integers(0, LONG - T + 1, size=B).astype(np.int32)).to(be.device)
    same = torch.equal(be.gather_batch(i16, index, offset, T=T).view(torch.int32), be.gather_batch(f32, index, offset, T=T).view(torch.int32))

    def kernel_ms(data, name):
        be.gather_batch(data, index, offset, T=T)
        (ms, calls), = [v for k, v in be.kernel_times().items() if k == name]
        assert calls == 1
        return ms

    ms = {"k_batch_gather_i16": [], "k_batch_gather": []}
    be.kernel_events(True)
    try:
        for rep in range(warmup + reps):
            for name, data in (("k_batch_gather_i16", i16), ("k_batch_gather", f32)):       # alternating: both see the same machine
                t = kernel_ms(data, name)
                if rep >= warmup:
                    ms[name].append(t)
    finally:
        be.kernel_events(False)
    out = {k: _stats(v) for k, v in ms.items()}
    out["k_batch_gather_i16"]["bytes_moved"], out["k_batch_gather"]["bytes_moved"] = 6 * B * T, 8 * B * T
    for k in out:
        out[k]["GBps"] = out[k]["bytes_moved"] / out[k]["median_ms"] / 1e6
    out["i16_over_f32"] = out["k_batch_gather_i16"]["median_ms"] / out["k_batch_gather"]["median_ms"]
    out["same_bits"] = bool(same)
    return out


def loop_times(be, reps, warmup):
    import torch
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.evaluate import evaluate
    hp = HParams(minibatch_size=B, bond_dim=D)
    model = PsiCMPS(hp, seed=0, backend=be)
    i16, f32 = _pcm(be.damped_sine(7, 0, N_CLIPS, T, hp.delta_t))
    sets = {"float32": ResidentDataset(f32, be), "int16": ResidentDataset(i16, be, storage="int16")}
    batches = N_CLIPS // B
    ms = {k: [] for k in sets}
    results = {}
    for rep in range(warmup + reps):
        for k, ds in sets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[k] = evaluate(model, ds, B)
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0) / batches)
    out = {}
    for k, ds in sets.items():
        be.kernel_events(True)
        try:
            evaluate(model, ds, B)
            kernels = {name: {"ms_per_batch": t / batches, "launches": n} for name, (t, n) in be.kernel_times().items()}
        finally:
            be.kernel_events(False)
        data_side = ("k_batch_gather", "k_batch_gather_i16", "k_loss_stats")
        forward = sum(v["ms_per_batch"] for name, v in kernels.items() if name not in data_side)
        st = _stats(ms[k])
        out[k] = {"dataset_bytes": ds.nbytes, "ms_per_batch": st, "kernels": kernels, "forward_kernels_ms_per_batch": forward,
                  "loop_adds_ms_per_batch": st["median_ms"] - forward, "mean_loss": results[k].mean, "n_nonfinite": results[k].n_nonfinite}
    out["same_result"] = results["float32"].scalars() == results["int16"].scalars()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    gathers = gather_times(be, a.reps, a.warmup)
    torch.cuda.empty_cache()
    loop = loop_times(be, a.reps, a.warmup)
    gates = {"i16_gather_within_1.25x_of_f32": {"value": gathers["i16_over_f32"], "limit": 1.25}}
    for g in gates.values():
        g["met"] = bool(g["value"] <= g["limit"])
    doc = {"what": "gathers: CMPS_OPT_KERNEL_EVENTS milliseconds per launch, the two kernels alternating; loop: wall-clock milliseconds per "
                   "batch of evaluate() (host clock between two device synchronisations around a whole pass) next to the kernels' own "
                   "milliseconds per batch from one more pass with the kernel events on",
           "device": "MI355X (gfx950); torch.cuda.get_device_name: " + torch.cuda.get_device_name(0),
           "shape": {"D": D, "T": T, "clips_per_batch": B, "dataset_clips": N_CLIPS, "long_clip": LONG},
           "reps": a.reps, "warmup": a.warmup, "gathers": gathers, "loop": loop, "gates": gates}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for k in ("k_batch_gather_i16", "k_batch_gather"):
        print(f"{k}: {gathers[k]['median_ms']:.4f} ms (spread {gathers[k]['spread']:.2f}), {gathers[k]['GBps']:.0f} GB/s")
    print(f"int16 / float32 gather: {gathers['i16_over_f32']:.3f}; same bits: {gathers['same_bits']}")
    for k in ("float32", "int16"):
        v = loop[k]
        print(f"evaluate from {k}: {v['ms_per_batch']['median_ms']:.3f} ms per batch, forward kernels {v['forward_kernels_ms_per_batch']:.3f} ms, "
              f"the loop adds {v['loop_adds_ms_per_batch']:.3f} ms; kernels " +
              ", ".join(f"{n} {x['ms_per_batch']:.4f}" for n, x in v["kernels"].items()))
    print("same result from both storages:", loop["same_result"], "; gates:", {k: (round(g["value"], 3), g["met"]) for k, g in gates.items()})
    return 0 if gathers["same_bits"] and loop["same_result"] else 1


if __name__ == "__main__":
    sys.exit(main())
