#!/usr/bin/env python3
"""What the host-drawn noise costs a generating stream, and what drawing it on the device costs instead.

usage: python scripts/time_device_noise.py [--out profiles/device_noise_times.json] [--reps 5] [--warmup 2]

Shape: D = 32, 1024 paths, 16000 steps generated through one SampleStream in ten `generate` calls of 1600 steps (the wave kernel).
A run opens a stream and makes the ten calls; every call is timed with the host clock between two device synchronisations, so a figure
holds everything a caller waits for: host-noise streams (the parent's code path: numpy Generator, float32 cast, transpose, upload) or
device-noise streams (cmps_noise_fill in front of the sampler kernel), then the sampler kernel, the download of the waveform and its
scaling.  Host and device runs alternate; --warmup runs of each are discarded, --reps are kept: the JSON file gets every per-call time,
each run's mean per call, and the median, minimum, maximum and spread over the runs.  One more run per mode, outside the timing, has
CMPS_OPT_KERNEL_EVENTS on and records the device time of k_noise_philox and k_sample_wave_stream per call.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, PATHS, STEPS, CALLS = 32, 1024, 16000, 10


def _model(backend):
    import numpy as np
    from audio_mps_amd import HParams, PsiCMPS
    hp = HParams(minibatch_size=PATHS, bond_dim=D, sigma=1.0, A=10.0)
    m = PsiCMPS(hp, seed=D, backend=backend)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    return m


def one_run(m, device_noise, seed):
    """Ten generate calls of one stream: (seconds per call, the last waveform's finiteness)."""
    import numpy as np
    import torch
    st = m.open_stream(PATHS, STEPS, temp=0.5, seed=seed, device_noise=device_noise)
    secs, ok = [], True
    for _ in range(CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wave = st.generate(STEPS // CALLS)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        ok = ok and bool(np.all(np.isfinite(wave)))
    return secs, ok


def summary(runs):
    per_run = [1e3 * statistics.mean(r) for r in runs]
    med = statistics.median(per_run)
    return {"median_ms_per_generate": med, "min_ms": min(per_run), "max_ms": max(per_run), "spread": (max(per_run) - min(per_run)) / med,
            "run_means_ms": per_run, "all_calls_ms": [[1e3 * s for s in r] for r in runs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_noise_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    m = _model(be)
    runs = {False: [], True: []}
    finite = True
    for rep in range(a.warmup + a.reps):
        for mode in (False, True):                              # alternating: both see the same machine
            secs, ok = one_run(m, mode, seed=rep)
            finite = finite and ok
            if rep >= a.warmup:
                runs[mode].append(secs)
    kernels = {}
    be.kernel_events(True)
    for mode in (False, True):
        one_run(m, mode, seed=99)
        kernels["device_noise" if mode else "host_noise"] = {k: {"ms_sum": ms, "launches": calls, "ms_per_launch": ms / calls}
                                                             for k, (ms, calls) in be.kernel_times().items()}
    be.kernel_events(False)
    host, dev = summary(runs[False]), summary(runs[True])
    doc = {"what": "wall-clock milliseconds per SampleStream.generate call (host clock between two device synchronisations), host-drawn "
                   "against device-drawn noise; kernels: CMPS_OPT_KERNEL_EVENTS times of one further run per mode",
           "device": "MI355X (gfx950); torch.cuda.get_device_name: " + torch.cuda.get_device_name(0),
           "shape": {"D": D, "paths": PATHS, "steps": STEPS, "generate_calls": CALLS, "steps_per_call": STEPS // CALLS,
                     "normals_per_call": PATHS * STEPS // CALLS, "noise_bytes_per_call": 4 * PATHS * STEPS // CALLS},
           "reps": a.reps, "warmup": a.warmup, "all_waveforms_finite": finite,
           "host_noise": host, "device_noise": dev,
           "host_over_device": host["median_ms_per_generate"] / dev["median_ms_per_generate"],
           "kernels": kernels}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"generate of {STEPS // CALLS} steps x {PATHS} paths: host noise {host['median_ms_per_generate']:.3f} ms "
          f"(spread {host['spread']:.2f}), device noise {dev['median_ms_per_generate']:.3f} ms (spread {dev['spread']:.2f}), "
          f"ratio {doc['host_over_device']:.2f}")
    for mode, ks in kernels.items():
        print(mode, {k: round(v["ms_per_launch"], 4) for k, v in ks.items()})
    return 0 if finite else 1


if __name__ == "__main__":
    sys.exit(main())
