#!/usr/bin/env python3
"""What the per-clip operand scales of the wide training forward cost: k_fwd_chain16 and k_hy_wide<f16x2> of this tree's library next to
those of a library built from the parent commit.

usage: python scripts/time_wild_clip.py --baseline-lib PATH/libcmps.so [--out profiles/wild_clip_times.json] [--reps 5] [--warmup 2]

The method of scripts/time_eval.py: CMPS_OPT_KERNEL_EVENTS milliseconds per kernel, --warmup repetitions discarded, the median of --reps
kept.  Shape: D = 128, T = 16000, 512 clips, cmps_psi_loss_fwd with save_for_bwd = 1 at the default options (CMPS_WIDE_CHAIN_MFMA,
CMPS_RANK1_DEFAULT).  A process loads one library, so every measurement is a fresh child process (CMPS_LIB), in the order baseline,
change, baseline, change: the two baseline runs give the spread of the session, against which the change is read.  The children also
return the per-clip losses: the change must reproduce the baseline's on ordinary clips (recorded as the largest relative difference).
GATE (recorded, not an error): change <= the slower baseline run, per kernel.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, T, B = 128, 16000, 512
KERNELS = ("k_fwd_chain16", "k_hy_wide<f16x2>")


def worker(reps, warmup):
    import numpy as np
    import torch
    from audio_mps_amd import HParams, PsiCMPS, _capi
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    hp = HParams(minibatch_size=B, bond_dim=D)
    m = PsiCMPS(hp, seed=0, backend=be)
    m.variables["Rx"] *= np.float32(0.5)
    m.variables["Ry"] *= np.float32(0.5)
    audio = be.damped_sine(7, 0, B, T, hp.delta_t)
    be.set_params(m.effective_params(), B, T, train=True)
    ms = {k: [] for k in KERNELS}
    be.kernel_events(True)
    try:
        for rep in range(warmup + reps):
            loss = be.forward(audio, save_for_bwd=True)
            times = be.kernel_times()
            if rep >= warmup:
                for k in KERNELS:
                    ms[k].append(times[k][0])
    finally:
        be.kernel_events(False)
    per = loss.cpu().numpy()
    print("RESULT " + json.dumps({"lib": _capi.LIB_PATH, "ms": ms, "loss": [float(x) for x in per],
                                  "device": torch.cuda.get_device_name(0)}))


def _stats(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "all_ms": list(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-lib", help="libcmps.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wild_clip_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.reps, a.warmup)
        return 0
    if not a.baseline_lib or not os.path.exists(a.baseline_lib):
        ap.error("--baseline-lib must name a library built from the parent commit")
    runs = []
    for name, lib in (("baseline", a.baseline_lib), ("change", None), ("baseline", a.baseline_lib), ("change", None)):
        env = dict(os.environ)
        env.pop("CMPS_LIB", None)
        if lib:
            env["CMPS_LIB"] = os.path.abspath(lib)
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--warmup", str(a.warmup)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
        line = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")]
        if proc.returncode != 0 or not line:
            print(proc.stdout[-4000:])
            return 1                                              # (nothing more is started behind a failed run)
        res = json.loads(line[0][len("RESULT "):])
        runs.append({"which": name, "kernels": {k: _stats(v) for k, v in res["ms"].items()}, "loss": res["loss"], "device": res["device"]})
        print(name, {k: round(v["median_ms"], 3) for k, v in runs[-1]["kernels"].items()})
    import numpy as np
    base, new = [r for r in runs if r["which"] == "baseline"], [r for r in runs if r["which"] == "change"]
    l0, l1 = np.array(base[0]["loss"]), np.array(new[0]["loss"])
    diff = float(np.max(np.abs(l1 - l0) / np.maximum(np.abs(l0), 1.0)))
    summary, gates = {}, {}
    for k in KERNELS:
        b = [r["kernels"][k]["median_ms"] for r in base]
        c = [r["kernels"][k]["median_ms"] for r in new]
        summary[k] = {"baseline_median_ms": b, "change_median_ms": c, "baseline_runs_differ_by": abs(b[0] - b[1]) / min(b),
                      "change_over_baseline": statistics.mean(c) / statistics.mean(b)}
        gates[k] = {"value": min(c), "limit": max(b), "met": bool(min(c) <= max(b))}
    doc = {"what": "CMPS_OPT_KERNEL_EVENTS milliseconds per launch of the wide training forward's kernels (cmps_psi_loss_fwd, save_for_bwd = 1, "
                   "default options): a library built from the parent commit (one operand scale per pair of clips) and this tree's (one per "
                   "clip), fresh processes alternating in one session",
           "device": "MI355X (gfx950); torch.cuda.get_device_name: " + runs[0]["device"],
           "shape": {"D": D, "T": T, "clips": B}, "reps": a.reps, "warmup": a.warmup, "summary": summary, "gates": gates,
           "all_losses_finite": bool(np.all(np.isfinite(l0)) and np.all(np.isfinite(l1))),
           "max_relative_loss_difference_change_vs_baseline": diff,
           "runs": [{"which": r["which"], "kernels": r["kernels"]} for r in runs]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for k, v in summary.items():
        print(f"{k}: baseline {v['baseline_median_ms']} ms, change {v['change_median_ms']} ms, ratio {v['change_over_baseline']:.4f}, "
              f"baseline runs differ by {v['baseline_runs_differ_by']:.4f}; gate met: {gates[k]['met']}")
    print(f"largest relative loss difference change vs baseline: {diff:.3e}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
