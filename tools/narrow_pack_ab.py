#!/usr/bin/env python3
"""Narrow NPROMA blocks, packed against unpacked, in one
process: for each NPROMA (8, 16, 32) and precision (fp64, mixed, fp32) ONE
state, on which KSEG runs alternately with narrow_pack(0) (A, the unpacked
kernels) and narrow_pack(1) (B, the packed ones) -- the same buffers, so the
field placement cancels.  After a time-based warm-up of both settings, `--rounds`
rounds of `--reps` timed launches per setting, ABAB; the figure of a setting
is the median over all its launches (30 by default), the spread that of the
A rounds' medians.  An NPROMA 64 state of each precision is the yardstick, and
a KCACHE row (fp64, NPROMA 32) closes the table.  One JSON line per row, then
one per NPROMA with the default the rule gives: packed only if it is faster
than unpacked by more than the A spread in all three precisions.

  python tools/narrow_pack_ab.py > profiles/narrow_pack/kseg_pack_ab.jsonl"""
import argparse
import json
import os
import statistics as stt
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dwarf-p-cloudsc_amd"))
import cloudsc_amd as ca  # noqa: E402

CODES = {"fp64": ca.FP64, "mixed": ca.MIXED, "fp32": ca.FP32}
VARIANTS = {"kseg": ca.VARIANT_KSEG, "kcache": ca.VARIANT_KCACHE}


def ab(g, variant, a):
    """ABAB on one state: ({mode: [ms of every launch]}, {mode: [median of each round]})."""
    t0 = time.time()
    while time.time() - t0 < a.warm_seconds:
        for mode in (0, 1):
            ca.narrow_pack(mode)
            g.run(variant, 10)
    every, rounds = {0: [], 1: []}, {0: [], 1: []}
    for _ in range(a.rounds):
        for mode in (0, 1):
            ca.narrow_pack(mode)
            ms = [float(x) for x in g.run(variant, a.reps)]
            every[mode] += ms
            rounds[mode].append(stt.median(ms))
    return every, rounds


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ngptot", type=int, default=163840)
    p.add_argument("--npromas", type=int, nargs="+", default=[8, 16, 32])
    p.add_argument("--precisions", nargs="+", default=["fp64", "mixed", "fp32"])
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warm-seconds", type=float, default=1.5)
    p.add_argument("--yardstick", type=int, default=64, help="NPROMA of the yardstick states (0 = none)")
    p.add_argument("--kcache", default="fp64:32", help="PRECISION:NPROMA of the KCACHE row ('' = none)")
    a = p.parse_args()
    ds = ca.load_dataset()
    rows = []

    def measure(variant, prec, nproma):
        g = ca.GpuState(ds, a.ngptot, nproma, CODES[prec])
        try:
            every, rounds = ab(g, VARIANTS[variant], a)
        finally:
            g.close()
            ca.narrow_pack(-1)
        ca.narrow_pack(1)
        geo = ca.launch_geometry(CODES[prec], VARIANTS[variant], a.ngptot, nproma, ds.klev)
        ca.narrow_pack(-1)
        una, pk = stt.median(every[0]), stt.median(every[1])
        spread = max(rounds[0]) - min(rounds[0])
        row = {"variant": variant, "precision": prec, "ngptot": a.ngptot, "nproma": nproma, "pack": geo["pack"],
               "launches_per_setting": len(every[0]), "unpacked_ms": round(una, 5), "packed_ms": round(pk, 5),
               "packed_over_unpacked": round(pk / una, 4),
               "unpacked_round_medians_ms": [round(x, 5) for x in rounds[0]],
               "packed_round_medians_ms": [round(x, 5) for x in rounds[1]],
               "unpacked_spread_ms": round(spread, 5), "packed_faster_beyond_spread": bool(una - pk > spread)}
        print(json.dumps(row), flush=True)
        return row

    for nproma in a.npromas:
        for prec in a.precisions:
            rows.append(measure("kseg", prec, nproma))
    yard = {}
    if a.yardstick:
        for prec in a.precisions:
            ca.narrow_pack(-1)
            g = ca.GpuState(ds, a.ngptot, a.yardstick, CODES[prec])
            try:
                t0 = time.time()
                while time.time() - t0 < a.warm_seconds:
                    g.run(ca.VARIANT_KSEG, 10)
                ms = []
                for _ in range(a.rounds):
                    ms += [float(x) for x in g.run(ca.VARIANT_KSEG, a.reps)]
            finally:
                g.close()
            yard[prec] = stt.median(ms)
            at32 = [r for r in rows if r["precision"] == prec and r["nproma"] == 32]
            print(json.dumps({"variant": "kseg", "precision": prec, "ngptot": a.ngptot, "nproma": a.yardstick,
                              "pack": 1, "launches": len(ms), "median_ms": round(yard[prec], 5),
                              "packed_nproma32_over_this": round(at32[0]["packed_ms"] / yard[prec], 4) if at32 else None,
                              "unpacked_nproma32_over_this": round(at32[0]["unpacked_ms"] / yard[prec], 4) if at32 else None}),
                  flush=True)
    if a.kcache:
        prec, nproma = a.kcache.split(":")
        measure("kcache", prec, int(nproma))
    for nproma in a.npromas:
        mine = [r for r in rows if r["nproma"] == nproma]
        print(json.dumps({"nproma": nproma, "default_packed_by_rule": all(r["packed_faster_beyond_spread"] for r in mine),
                          "packed_over_unpacked": {r["precision"]: r["packed_over_unpacked"] for r in mine}}), flush=True)


if __name__ == "__main__":
    main()
