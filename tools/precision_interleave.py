#!/usr/bin/env python3
"""KSEG in fp64, mixed and fp32 on one box, interleaved in one process
(DESIGN.md §3.17): one placement-searched state per (precision, replica),
a time-based warm-up, then rounds of `--reps` timed launches per state
round-robin (cloudsc_state_run_span).  Prints one JSON line per state --
median ms per launch, the device memory the state took, its placement -- and
one per precision with the per-field relL1 against reference.h5
(cloudsc_state_validate).

  python tools/precision_interleave.py --ngptot 163840 --nproma 64"""
import argparse
import ctypes as C
import json
import os
import statistics as stt
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dwarf-p-cloudsc_amd"))
import cloudsc_amd as ca  # noqa: E402

CODES = {"fp64": ca.FP64, "mixed": ca.MIXED, "fp32": ca.FP32}


def free_bytes():
    free, total = C.c_size_t(), C.c_size_t()
    ca._hip().hipMemGetInfo(C.byref(free), C.byref(total))
    return free.value


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--precisions", nargs="+", default=["fp64", "mixed", "fp32"])
    p.add_argument("--ngptot", type=int, default=163840)
    p.add_argument("--nproma", type=int, default=64)
    p.add_argument("--replicas", type=int, default=2)
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warm-seconds", type=float, default=3.0)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    ds = ca.load_dataset()
    states = []
    try:
        for rep in range(a.replicas):
            for name in a.precisions:
                before = free_bytes()
                g = ca.GpuState(ds, a.ngptot, a.nproma, CODES[name])
                g.run(ca.VARIANT_KSEG, 1)      # the KSEG workspace is part of the state
                states.append((name, rep, g, before - free_bytes()))
        t0 = time.time()
        while time.time() - t0 < a.warm_seconds:
            for _, _, g, _ in states:
                g.run_span(ca.VARIANT_KSEG, 10)
        res = {(n, r): [] for n, r, _, _ in states}
        for _ in range(a.rounds):
            for n, r, g, _ in states:
                res[(n, r)].append(g.run_span(ca.VARIANT_KSEG, a.reps) / a.reps)
        for n, r, g, mem in states:
            print(json.dumps({"tag": a.tag, "precision": n, "replica": r, "ngptot": a.ngptot, "nproma": a.nproma,
                              "launches": a.rounds * a.reps, "median_ms": round(stt.median(res[(n, r)]), 5),
                              "min_ms": round(min(res[(n, r)]), 5), "device_bytes": mem,
                              "placement": g.placement()}), flush=True)
        for n, r, g, _ in states:
            if r == 0:
                rel = {k: ca.rel_error(s[3], s[4])[0] for (_, k), s in zip(ca.VALIDATED, g.validate())}
                print(json.dumps({"tag": a.tag, "precision": n, "ngptot": a.ngptot,
                                  "rel_l1_vs_reference_h5": {k: float("%.3e" % v) for k, v in rel.items()}}),
                      flush=True)
    finally:
        for _, _, g, _ in states:
            g.close()


if __name__ == "__main__":
    main()
