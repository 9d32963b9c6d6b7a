#!/usr/bin/env python
"""field_repeat.py [--n 512] [--late 2500] — how many cells repeat each field's bits two steps apart (step n+1 against step n-1).

For each of the six encoded fields: the share of all cells whose bits at step n+1 equal those at step n-1 (compared on the device:
the state is copied device to device into torch tensors, nothing is downloaded), and the share of the step's predicted cells whose
output buffer already held the field (tau3d_store_skip_stats: k_tile_predict's per-field bits, the stores k_fill_z skips).
Two windows: the headline start (impulsive start, clock (0.02, 1e-4), steps 5-25) and the late state (ramped start + --late steps)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluid_sims_amd as f  # noqa: E402
from tests.devstate import FIELDS, hip, snapshot  # noqa: E402,F401


def window(e, H, steps, label):
    shp = (6,) + tuple(e.shape)
    bufs = [torch.empty(shp, dtype=torch.int32, device="cuda") for _ in range(3)]
    snapshot(e, H, bufs[0])           # state n-1
    e.step(1); snapshot(e, H, bufs[1])  # state n
    ncell = bufs[0][0].numel()
    tot_eq = [0] * 6
    tot_held = [0] * 6
    tot_pred = 0
    print(f"# {label}: per step, share of ALL cells with bits(n+1) == bits(n-1) | share of PREDICTED cells whose store was skipped")
    for k in range(steps):
        e.step(1)
        cur = bufs[(k + 2) % 3]
        snapshot(e, H, cur)
        old = bufs[k % 3]
        eq = [int((cur[m] == old[m]).sum().item()) for m in range(6)]
        held, pred = e.store_skip_stats()
        for m in range(6):
            tot_eq[m] += eq[m]; tot_held[m] += held[m]
        tot_pred += pred
        print(f"step {k:3d}  all " + " ".join(f"{FIELDS[m]} {eq[m] / ncell:6.1%}" for m in range(6)) +
              f"  | predicted {pred / ncell:6.1%} of cells: " +
              " ".join(f"{FIELDS[m]} {held[m] / max(pred, 1):6.1%}" for m in range(6)), flush=True)
    print(f"{label} mean over {steps} steps:  all cells " + " ".join(f"{FIELDS[m]} {tot_eq[m] / (ncell * steps):6.1%}" for m in range(6)))
    print(f"{label} mean over {steps} steps:  predicted cells ({tot_pred / (ncell * steps):.1%} of all) " +
          " ".join(f"{FIELDS[m]} {tot_held[m] / max(tot_pred, 1):6.1%}" for m in range(6)))
    nf = sum(1 for m in range(6) if tot_held[m] >= 0.9 * tot_pred and tot_pred > 0)
    print(f"{label}: fields repeating in >= 90 % of predicted cells: {nf}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--late", type=int, default=2500)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    H = hip()
    e = f.Tau3D(a.n)
    e.init(1); e.set_clock(0.02, 1e-4); e.step(5)
    window(e, H, a.steps, "headline")
    e.close()
    e = f.Tau3D(a.n)
    e.init(0); e.step(a.late)
    window(e, H, 5, f"late ({a.late} steps)")
    e.close()


if __name__ == "__main__":
    main()
