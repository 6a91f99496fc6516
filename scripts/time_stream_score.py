#!/usr/bin/env python3
"""What scoring a followed signal costs: cmps_psi_stream_score against a plain follow (cmps_psi_stream, forced steps only) of the same
steps, and against cmps_psi_loss_fwd on the same clips, in one process.

usage: python scripts/time_stream_score.py [--out profiles/stream_score_times.json] [--reps 7]

Shapes: D = 32, 1024 paths, 16000 steps (the wave kernel) in segments of 16000, 1000 and 100; D = 128, 64 paths, 4000 steps (the wide
kernel) in segments of 4000, 1000 and 100.  One sine clip per path; audio blocks (with their one-sample overlap), nll and the state
records are resident in device memory, pred is not asked for; HIP events on the launch stream bracket the launches of one whole job, so
a segmented time holds the launch gaps and the state round trips.  Every job is run once untimed and then --reps times; the median,
every value and the spread (max - min) / median go to the JSON file, with the ratios scored / followed and scored / forward.  The scored
total of the one-call job is compared with cmps_psi_loss_fwd's loss (max relative difference, recorded).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 1024, 16000, (16000, 1000, 100)), (128, 64, 4000, (4000, 1000, 100))]


def _model(D, n, backend):
    import numpy as np
    from audio_mps_amd import HParams, PsiCMPS
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    m = PsiCMPS(hp, seed=D, backend=backend)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    return m


def time_shape(D, n, steps, segments, reps):
    import numpy as np
    import torch
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    be.set_params(_model(D, n, be).effective_params(), n, steps + 1, train=False)
    lib, h, dev = be._lib, be._h, be.device
    t = np.arange(steps + 1, dtype=np.float64) / 16000.0
    clip = (0.5 * np.sin(2 * np.pi * 261.6 * t[None, :] + np.arange(n)[:, None])).astype(np.float32)
    audio = torch.from_numpy(clip).to(dev)
    stream = be._stream()
    state = be.stream_state(n)
    loss = torch.zeros(n, dtype=torch.float32, device=dev)
    fwd_loss = torch.zeros(n, dtype=torch.float32, device=dev)
    bufs = {}

    def blocks(seg):
        """(k0, steps, audio block [n, steps + 1], nll [n, steps]) per segment, built once outside the timing."""
        if seg not in bufs:
            bufs[seg] = [(k0, min(seg, steps - k0), audio[:, k0:k0 + min(seg, steps - k0) + 1].contiguous(),
                          torch.empty((n, min(seg, steps - k0)), dtype=torch.float32, device=dev)) for k0 in range(0, steps, seg)]
            torch.cuda.synchronize()
        return bufs[seg]

    def job_score(seg):
        st = state.data_ptr()
        for k0, cnt, a, nll in blocks(seg):
            code = lib.cmps_psi_stream_score(h, st if k0 else None, st, k0, a.data_ptr(), n, cnt, n, nll.data_ptr(), loss.data_ptr(), None, stream)
            assert code == 0, lib.cmps_last_error(h)

    def job_follow(seg):
        st = state.data_ptr()
        for k0, cnt, a, _ in blocks(seg):
            code = lib.cmps_psi_stream(h, st if k0 else None, st, k0, a.data_ptr(), n, cnt, None, 0, n, None, None, stream)
            assert code == 0, lib.cmps_last_error(h)

    def job_fwd():
        code = lib.cmps_psi_loss_fwd(h, audio.data_ptr(), n, steps + 1, fwd_loss.data_ptr(), 0, stream)
        assert code == 0, lib.cmps_last_error(h)

    def timed(job):
        job()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            job()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        return {"median_ms": med, "all_ms": ms, "spread": (max(ms) - min(ms)) / med, "us_per_step": 1e3 * med / steps}

    res = {"cmps_psi_loss_fwd": timed(job_fwd)}
    for seg in segments:
        tag = "one_call" if seg >= steps else f"segments_of_{seg}"
        f, s = timed(lambda: job_follow(seg)), timed(lambda: job_score(seg))
        res[f"follow_{tag}"], res[f"score_{tag}"] = f, s
        res[f"score_over_follow_{tag}"] = s["median_ms"] / f["median_ms"]
        res[f"launches_{tag}"] = (steps + seg - 1) // seg
        if seg >= steps:
            lo, fw = loss.cpu().numpy().astype(np.float64), fwd_loss.cpu().numpy().astype(np.float64)
            res["score_total_vs_fwd_max_rel"] = float(np.max(np.abs(lo - fw) / np.maximum(np.abs(fw), 1.0)))
            res["finite"] = bool(np.all(np.isfinite(lo)))
    res["score_one_call_over_loss_fwd"] = res["score_one_call"]["median_ms"] / res["cmps_psi_loss_fwd"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_score_times.json"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    shapes = {}
    for D, n, steps, segments in SHAPES:
        shapes[f"D{D}_n{n}_steps{steps}"] = dict(D=D, n=n, steps=steps, **time_shape(D, n, steps, segments, a.reps))
    doc = {"what": "kernel time of one followed / scored job of forced steps (HIP events around its launches, inputs resident in device "
                   "memory), milliseconds", "device": "MI355X (gfx950); torch.cuda.get_device_name: " + torch.cuda.get_device_name(0),
           "reps": a.reps, "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for key, row in shapes.items():
        print(key, {k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in row.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
