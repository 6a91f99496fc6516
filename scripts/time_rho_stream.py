#!/usr/bin/env python3
"""What a segment of the resumable RhoCMPS sampler costs: cmps_rho_stream against cmps_rho_sample_primed on the same job, as one call and
cut into segments, with the existing entries of this tree against the parent's.

usage: python scripts/time_rho_stream.py [--out profiles/rho_stream_segment_times.json] [--reps 7] [--inner 10] [--parent-root DIR]

Shapes (those of scripts/time_rho_sample.py): D = 32, rank 32, 64 paths, P = 1000 teacher-forced + 1000 sampled steps on one shared clip
-- the row-array kernel, both arithmetics (CMPS_OPT_RANK1 default fp16 x 2, and bf16 x 3) -- and the block kernel (CMPS_VARIANT_BLOCK) at
8 paths x (100 + 100) steps.  Clip, noise, output, pred and state records are resident in device memory; HIP events on the launch stream
bracket --inner consecutive runs of one whole job (one cmps_rho_sample call over P + length steps; one cmps_rho_sample_primed call; one
cmps_rho_stream call; the job in segments of 1024 and of 64 steps, state read and written in place), so a segmented time holds the
launch gaps and the state round trips.  Every job is run once untimed and then --reps times; the median (per job), every value and the
spread (max - min) / median go to the JSON file, and the launch boundary as (segmented - one call) / (launches - 1).
--parent-root names a checkout of the parent commit with its library built: its cmps_rho_sample and cmps_rho_sample_primed are timed in
a child process at the same shapes, alternating with nothing else on the device -- the "equal within the run-to-run spread" comparison.
Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                  help="the checkout the package is imported from (the --parent-root child passes the parent's)")
ROOT = os.path.abspath(_pre.parse_known_args()[0].root)
sys.path.insert(0, ROOT)

BLOCK, BF16X3 = 1, 2
# (name, variant, rank1 option, paths, forced, sampled)
SHAPES = [("mfma_f16x2_D32_r32_n64_1000+1000", 0, None, 64, 1000, 1000), ("mfma_bf16x3_D32_r32_n64_1000+1000", 0, BF16X3, 64, 1000, 1000),
          ("block_D32_r32_n8_100+100", BLOCK, None, 8, 100, 100)]
SEGMENTS = [1024, 64]


def time_shape(variant, rank1, n, P, length, reps, inner, entries_only):
    import numpy as np
    import torch
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd.scan import HipScan
    D = rank = 32
    hp = HParams(minibatch_size=n, bond_dim=D, initial_rank=rank, sigma=0.05)
    m = RhoCMPS(hp, seed=2, backend=HipScan(D, variant=variant, rank1=rank1))
    steps = P + length
    be = m._prepare(n, steps + 1, train=False)
    lib, h, dev = be._lib, be._h, be.device
    rng = np.random.default_rng(0)
    noise = torch.from_numpy((0.05 * np.sqrt(hp.delta_t) * rng.standard_normal((n, steps))).astype(np.float32)).to(dev)
    t = np.arange(steps + 1, dtype=np.float32) * np.float32(hp.delta_t)
    clip = torch.from_numpy((0.1 * np.sin(2 * np.pi * 261.6 * t) * np.exp(-t / 0.1)).astype(np.float32)).to(dev)      # one clip, shared
    out = torch.empty((n, steps), dtype=torch.float32, device=dev)
    pred = torch.empty((n, steps), dtype=torch.float32, device=dev)
    stream = be._stream()

    def timed(job):
        job()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                job()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / inner)
        med = statistics.median(ms)
        return {"median_ms": med, "all_ms": ms, "spread": (max(ms) - min(ms)) / med, "us_per_step": 1e3 * med / steps}

    def job_sample():
        assert lib.cmps_rho_sample(h, noise.data_ptr(), n, steps, out.data_ptr(), 0, stream) == 0

    noise_p = noise[:, :length].contiguous()                       # [n][length]: the sampled steps' noise, as the stream jobs cut it

    def job_primed():
        assert lib.cmps_rho_sample_primed(h, clip.data_ptr(), 1, P + 1, noise_p.data_ptr(), n, length, out.data_ptr(), pred.data_ptr(), 0,
                                          stream) == 0

    res = {"cmps_rho_sample": timed(job_sample), "cmps_rho_sample_primed": timed(job_primed)}
    if entries_only:
        return res
    ref_out, ref_pred = out.flatten()[:n * length].view(n, length).clone(), pred.flatten()[:n * P].view(n, P).clone()   # ([n][length], [n][P])
    state = be.rho_stream_state(n)
    st = state.data_ptr()
    res["state_bytes_per_path"] = state.numel() // n

    def segments(seg):
        """(k0, forced, sampled, clip pointer, noise, out, pred) per launch; a segment's noise, out and pred are contiguous arrays of their
        own, as a caller would hold them (built once, outside the timing); the shared clip is read in place"""
        rows = []
        for k0 in range(0, steps, seg):
            k1 = min(k0 + seg, steps)
            f, s = max(min(k1, P) - k0, 0), max(k1 - max(k0, P), 0)
            nz = noise[:, max(k0, P) - P:k1 - P].contiguous() if s else None
            rows.append((k0, f, s, clip.data_ptr() + 4 * k0 if f else None, nz,
                         torch.empty((n, s), dtype=torch.float32, device=dev) if s else None,
                         torch.empty((n, f), dtype=torch.float32, device=dev) if f else None))
        torch.cuda.synchronize()
        return rows

    def job_stream(rows):
        for k0, f, s, cp, nz, o, pr in rows:
            code = lib.cmps_rho_stream(h, st if k0 else None, st, k0, cp, 1, f, nz.data_ptr() if s else None, s, n,
                                       o.data_ptr() if s else None, pr.data_ptr() if f else None, 0, stream)
            assert code == 0, lib.cmps_last_error(h)

    one = segments(steps)
    res["stream_one_call"] = timed(lambda: job_stream(one))
    res["stream_one_call_equals_primed_bitwise"] = bool(torch.equal(one[0][5], ref_out) and torch.equal(one[0][6], ref_pred))
    for seg in SEGMENTS:
        if seg < steps:
            rows = segments(seg)
            r = res[f"stream_segments_of_{seg}"] = timed(lambda: job_stream(rows))
            r["launches"] = len(rows)
            r["us_per_launch_boundary"] = 1e3 * (r["median_ms"] - res["stream_one_call"]["median_ms"]) / (len(rows) - 1)
            r["equals_one_call_bitwise"] = bool(torch.equal(torch.cat([x[5] for x in rows if x[5] is not None], 1), one[0][5])
                                                and torch.equal(torch.cat([x[6] for x in rows if x[6] is not None], 1), one[0][6]))
    return res


def main():
    ap = argparse.ArgumentParser(parents=[_pre], description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rho_stream_segment_times.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--entries-only", action="store_true",
                    help="time cmps_rho_sample and cmps_rho_sample_primed only and print the JSON (what the --parent-root child runs)")
    a = ap.parse_args()
    import torch
    shapes = {}
    for name, variant, rank1, n, P, length in SHAPES:
        shapes[name] = dict(D=32, rank=32, n=n, forced=P, sampled=length, **time_shape(variant, rank1, n, P, length, a.reps, a.inner, a.entries_only))
    if a.entries_only:
        print("JSON " + json.dumps(shapes))
        return 0
    doc = {"what": "device-event time of one job (its launches only; inputs and state resident in device memory), milliseconds per job",
           "device": "MI355X (gfx950); torch.cuda.get_device_name: " + torch.cuda.get_device_name(0), "reps": a.reps,
           "jobs_per_event_pair": a.inner, "shapes": shapes}
    if a.parent_root:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(a.parent_root), "--entries-only",
                               "--reps", str(a.reps), "--inner", str(a.inner)], stdout=subprocess.PIPE, text=True, check=True, timeout=600)
        parent = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("JSON ")][-1][5:])
        for key, row in shapes.items():
            for entry in ("cmps_rho_sample", "cmps_rho_sample_primed"):
                row["parent_" + entry] = parent[key][entry]
                row[entry + "_over_parent"] = row[entry]["median_ms"] / parent[key][entry]["median_ms"]
            row["stream_one_call_over_parent_primed"] = row["stream_one_call"]["median_ms"] / parent[key]["cmps_rho_sample_primed"]["median_ms"]
    for key, row in shapes.items():
        row["stream_one_call_over_primed"] = row["stream_one_call"]["median_ms"] / row["cmps_rho_sample_primed"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for key, row in shapes.items():
        print(key, {k: (round(v["median_ms"], 4) if isinstance(v, dict) else v) for k, v in row.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
