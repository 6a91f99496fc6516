#!/usr/bin/env python3
"""Worst observed error of the state read-outs (cmps_psi_states, cmps_rho_states) against the f64t32 oracle, per stash layout, next to
the bar of tests/test_gpu_states.py.  Runs every case of tests/_states_ref.py on the GPU, prints one line per case and writes the summary
(usage: states_parity.py [--out profiles/states_parity.json])."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import _states_ref as SR

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "states_parity.json"))
args = ap.parse_args()


def worst(table, layout, entry):
    """Keep, per layout, the case with the largest error / bar."""
    cur = table.setdefault(layout, {"cases": 0, "worst": None})
    cur["cases"] += 1
    if cur["worst"] is None or entry["error"] / entry["bar"] > cur["worst"]["error"] / cur["worst"]["bar"]:
        cur["worst"] = entry


psi, rho, purity = {}, {}, {}
for case in SR.PSI_CASES:
    err = SR.max_abs(SR.run_psi_case(case)["states"], SR.case_reference(case)[0])
    d32 = SR.psi_d32(case)
    print(f"{case.id}: max |hip - f64t32| {err:.3e}  bar {case.bar:.0e}  d32 {d32:.2e}", flush=True)
    worst(psi, case.layout, {"case": case.id, "error": err, "bar": case.bar, "d32": d32})
floor = {}
for variant in SR.FLOOR_VARIANTS:
    out = SR.run_psi(*SR.floor_inputs(), variant=variant)["states"]
    ref = SR.floor_reference()[0]
    floor["block" if variant == SR.BLOCK else "wave16"] = {
        "annihilated_clip_max_abs": float(np.max(np.abs(out[1]))), "other_clips_error": SR.max_abs(out[[0, 2]], ref[[0, 2]]), "bar": SR.PSI_BAR}
for case in SR.RHO_CASES:
    ref, pur_ref, _ = SR.case_reference(case)
    out = SR.run_rho_case(case)
    (bar_rho, bar_pur), (d_rho, d_pur) = SR.rho_bars(case), SR.rho_d32(case)
    e_rho, e_pur = SR.rel_inf(out["rho"], ref), SR.rel_inf(out["purity"], pur_ref)
    print(f"{case.id}: rho {e_rho:.3e} (bar {bar_rho:.2e}, d32 {d_rho:.2e})  purity {e_pur:.3e} (bar {bar_pur:.2e}, d32 {d_pur:.2e})", flush=True)
    worst(rho, case.layout, {"case": case.id, "error": e_rho, "bar": bar_rho, "d32": d_rho})
    worst(purity, case.layout, {"case": case.id, "error": e_pur, "bar": bar_pur, "d32": d_pur})

res = {
    "what": "state read-outs against the f64t32 oracle (float64 on the float32 time grid), worst case per stash layout by error / bar; "
            "d32: the float32 oracle's own distance from f64t32 on that case",
    "device": f"MI355X (gfx950); torch.cuda.get_device_name: {torch.cuda.get_device_name(0)}",
    "pure_state": {"metric": "max |hip - f64t32| over clips, steps and components (unit vectors)", "layouts": psi, "floor_case": floor},
    "rho": {"metric": "max |hip - f64t32| / max |f64t32|; bar max(1e-5, 3 d32)", "layouts": rho},
    "rho_purity": {"metric": "the same for Re tr rho^2", "layouts": purity},
}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res, indent=1))
