#!/usr/bin/env python3
"""What a segment of the resumable sampler costs: cmps_psi_stream against cmps_psi_sample on the same sampled-only job, as one call and
cut into segments.

usage: python scripts/time_stream.py [--out profiles/stream_segment_times.json] [--reps 7] [--parent-lib PATH]

Shapes: D = 32, 1024 paths, 16000 sampled steps (the wave kernel) and D = 128, 512 paths, 4000 steps (the wide kernel).  Noise, output and
state records are resident in device memory; HIP events on the launch stream bracket the launches of one whole job (one cmps_psi_sample
call; one cmps_psi_stream call; the job in segments of 4096, 1024 and 64 steps, state read and written in place), so a segmented time
holds the launch gaps and the state round trips.  Every job is run once untimed and then --reps times; the median, every value and the
spread (max - min) / median go to the JSON file.  --parent-lib names a libcmps.so built from the parent commit: its cmps_psi_sample is
timed in a child process at the same shapes (through ctypes alone: that library lacks the stream entries the package's binding asks for),
which is the "equal within the run-to-run spread" comparison.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 1024, 16000), (128, 512, 4000)]
SEGMENTS = [4096, 1024, 64]


def _model(D, n, backend):
    import numpy as np
    from audio_mps_amd import HParams, PsiCMPS
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)
    m = PsiCMPS(hp, seed=D, backend=backend)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    return m


class RawLib:
    """cmps_create / cmps_set_params / cmps_psi_sample of a libcmps.so through ctypes alone (the --parent-lib child)."""

    def __init__(self, path, D, n, steps):
        import numpy as np
        import torch                    # first: libcmps binds to the HIP runtime torch has loaded
        c_int, vp = ctypes.c_int, ctypes.c_void_p
        self._lib = lib = ctypes.CDLL(path)
        lib.cmps_create.argtypes = [c_int, ctypes.POINTER(vp)]
        lib.cmps_workspace_bytes.argtypes = [c_int] * 4
        lib.cmps_workspace_bytes.restype = ctypes.c_size_t
        lib.cmps_set_params.argtypes = [vp] * 6 + [ctypes.c_float, ctypes.c_double, ctypes.c_double, c_int, c_int, c_int, vp, ctypes.c_size_t, vp]
        lib.cmps_psi_sample.argtypes = [vp, vp, c_int, c_int, vp, vp]
        lib.cmps_last_error.argtypes = [vp]
        lib.cmps_last_error.restype = ctypes.c_char_p
        self.device = torch.device("cuda:0")
        self._h = vp()
        assert lib.cmps_create(D, ctypes.byref(self._h)) == 0
        p = _model(D, n, object()).effective_params()
        self._keep = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
                      for x in (p.R.real, p.R.imag, p.freqs, p.psi0.real, p.psi0.imag)]
        nbytes = lib.cmps_workspace_bytes(D, n, steps + 1, 0)
        self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        code = lib.cmps_set_params(self._h, *[t.data_ptr() for t in self._keep], float(p.A), float(p.sigma), float(p.delta_t), steps + 1, n, 0,
                                   (self._ws.data_ptr() + 255) // 256 * 256, nbytes, self._stream())
        assert code == 0, lib.cmps_last_error(self._h)

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


def time_shape(D, n, steps, reps, sample_only):
    import torch
    if sample_only:
        be = RawLib(os.environ["CMPS_LIB"], D, n, steps)
    else:
        from audio_mps_amd.scan import HipScan
        be = HipScan(D)
        be.set_params(_model(D, n, be).effective_params(), n, steps + 1, train=False)
    lib, h = be._lib, be._h
    gen = torch.Generator(device="cpu").manual_seed(D)
    std = (0.5 / 16000) ** 0.5                                    # sigma = 1, temp 0.5, delta_t = 1 / 16000
    noise = (std * torch.randn((n, steps), generator=gen)).to(be.device)
    out = torch.empty((n, steps), dtype=torch.float32, device=be.device)
    stream = be._stream()

    def job_sample():
        assert lib.cmps_psi_sample(h, noise.data_ptr(), n, steps, out.data_ptr(), stream) == 0

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

    res = {"cmps_psi_sample": timed(job_sample)}
    if sample_only:
        return res
    # (a segment's noise and out are contiguous [n][cnt] arrays, as a caller would hold them: built once, outside the timing)
    state = be.stream_state(n)
    ref = out.clone()
    res["stream_one_call"] = timed(lambda: job_stream_contig(lib, h, be, state, noise, out, n, steps, steps, stream))
    same = bool(torch.equal(out, ref))
    for seg in SEGMENTS:
        if seg < steps:
            res[f"stream_segments_of_{seg}"] = timed(lambda: job_stream_contig(lib, h, be, state, noise, out, n, steps, seg, stream))
            res[f"stream_segments_of_{seg}"]["launches"] = (steps + seg - 1) // seg
    res["stream_one_call_equals_sample_bitwise"] = same
    return res


_bufs = {}


def job_stream_contig(lib, h, be, state, noise, out, n, steps, seg, stream):
    """The job in segments of `seg` steps on per-segment contiguous noise / out buffers (built once per (shape, seg), outside the timing)."""
    import torch
    key = (n, steps, seg)
    if key not in _bufs:
        _bufs[key] = [(0, steps, noise, out)] if seg >= steps else [
            (k0, min(seg, steps - k0), noise[:, k0:k0 + seg].contiguous(),
             torch.empty((n, min(seg, steps - k0)), dtype=torch.float32, device=be.device)) for k0 in range(0, steps, seg)]
        torch.cuda.synchronize()
    st = state.data_ptr()
    for k0, cnt, nz, o in _bufs[key]:
        code = lib.cmps_psi_stream(h, st if k0 else None, st, k0, None, 1, 0, nz.data_ptr(), cnt, n, o.data_ptr(), None, stream)
        assert code == 0, lib.cmps_last_error(h)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_segment_times.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sample-only", action="store_true", help="time cmps_psi_sample only and print the JSON (what the --parent-lib child runs)")
    a = ap.parse_args()
    import torch
    shapes = {}
    for D, n, steps in SHAPES:
        shapes[f"D{D}_n{n}_steps{steps}"] = dict(D=D, n=n, steps=steps, **time_shape(D, n, steps, a.reps, a.sample_only))
    if a.sample_only:
        print("JSON " + json.dumps(shapes))
        return 0
    doc = {"what": "kernel time of one sampled-only job (HIP events around its launches, inputs resident in device memory), milliseconds",
           "device": "MI355X (gfx950); torch.cuda.get_device_name: " + torch.cuda.get_device_name(0), "reps": a.reps, "shapes": shapes}
    if a.parent_lib:
        env = dict(os.environ, CMPS_LIB=os.path.abspath(a.parent_lib))
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--sample-only", "--reps", str(a.reps)], env=env,
                              stdout=subprocess.PIPE, text=True, check=True, timeout=600)
        parent = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("JSON ")][-1][5:])
        for key, row in shapes.items():
            p = parent[key]["cmps_psi_sample"]
            row["parent_cmps_psi_sample"] = p
            row["stream_one_call_over_parent_sample"] = row["stream_one_call"]["median_ms"] / p["median_ms"]
    for key, row in shapes.items():
        row["stream_one_call_over_sample"] = row["stream_one_call"]["median_ms"] / row["cmps_psi_sample"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for key, row in shapes.items():
        print(key, {k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in row.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
