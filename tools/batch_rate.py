#!/usr/bin/env python3
"""One batched launch over N small field sets against N one-shot launches on them, and against one launch on a
single set of all their columns: does cloudsc_gpu_run_batch give an ensemble host the card back?

    python tools/batch_rate.py [--columns 16384] [--nproma 128] [--nsets 1 2 4 8 16] [--rounds 4] [--steps 20]
                               [--out profiles/batch/rate.jsonl]

fp64 for every N, one fp32 line at the largest N.  The sets are cloudsc_fields_alloc sets without the placement
search (33 searches would take longer than the measurement, and all three cases go without), expanded from the data
set, set i from column i * columns on.  Per N three cases, alternated in one process (a, b, c, a, b, c, ...):

  (a) N cloudsc_gpu_run_outputs(KCACHE, ALL) launches on the default stream, one per set: what such a host does today
  (b) one cloudsc_gpu_run_batch over N sets of its own holding the same columns, under the device's parameter set
  (c) one KCACHE launch on a single set of N * columns columns: the ceiling a batch can reach -- a host that owns
      its members' allocations cannot build this set

A run is `steps` back-to-back repetitions of the case between two events after two untimed ones; `rounds` runs per
case after one untimed round; median, minimum and maximum of the ms per repetition.  plude is INOUT and is not
expanded again: (a) and (b) are launched equally often, so their sets stay bit-identical, which the tool checks at
the end of every N (cloudsc_fields_compare of the 21 outputs of every set).  The STREAM copy of the same run goes
first.  One JSON line per record.  Needs an MI355X.

EXPECTATION, written before the first run (nobody had timed a batched launch):
  A KCACHE step fills the card at about 131 k columns (256 CUs x 4 SIMDs x 2 waves x 64 lanes); below that its time
  is the level loop's latency of one wave, 0.95 ms at 16,384 columns against 1.66 ms at 163,840 (README round 6).
  So (a) grows linearly in N, N x 0.95 ms; (c) stays near 0.95 ms up to N = 8 (131 k columns: every wave resident
  at once) and steps up at N = 16 (two rounds of waves); (b) tracks (c): the same waves doing the same work, each
  reading its arguments from a table entry instead of the kernarg segment -- b_over_c between 1.00 and 1.05, and
  b_over_a about 1 / N up to N = 8.  If (b) does not beat (a) the numbers say so and the per-member parameter
  sets remain what the form is for."""
import argparse
import contextlib

import numpy as np

import rate_harness as rh
from rate_harness import ca

EXPECTATION = {"a": "linear in N: N x the one-set time (0.95 ms at 16384 columns, README round 6)",
               "c": "flat up to 131 k columns (N = 8), a step up at N = 16",
               "b_over_c": "1.00 to 1.05", "b_over_a": "about 1 / N up to N = 8",
               "surprise": "b_over_c above 1.15, or b_over_a near 1",
               "why": "see the EXPECTATION paragraph of tools/batch_rate.py (DESIGN 3.31, 10.4)"}
KCACHE = ca.VARIANT_KCACHE


def measure(lib, hip, timer, records, ds, label, prec, columns, nproma, counts, args):
    klev, nmax = ds.klev, max(counts)
    with contextlib.ExitStack() as stack:
        def fields(ngptot, col_offset):
            d = stack.enter_context(contextlib.closing(ca.DeviceFields(ngptot, nproma, klev, prec, place=False)))
            d.expand(ds, col_offset)
            return d
        singles = [fields(columns, i * columns) for i in range(nmax)]
        members = [fields(columns, i * columns) for i in range(nmax)]
        whole = fields(nmax * columns, 0)
        for n in counts:
            batch = stack.enter_context(contextlib.closing(
                ca.Batch(members[:n], prec, ca.OUTPUTS_ALL, columns, nproma, klev)))

            def run_a():
                for d in singles[:n]:
                    ca.gpu_run_outputs(d.f, prec, KCACHE, ca.OUTPUTS_ALL, columns, nproma, klev)

            def run_b():
                batch.run()

            def run_c():     # the first n * columns columns of the big set: a prefix of every array's blocks
                ca.gpu_run_outputs(whole.f, prec, KCACHE, ca.OUTPUTS_ALL, n * columns, nproma, klev)

            ms = rh.alternate(lambda launch: timer.ms_per_launch(launch, args.steps),
                              [("a", run_a), ("b", run_b), ("c", run_c)], args.rounds, 1,
                              rh.launch_check(lib, KCACHE, None))
            differ = sum(v["mismatches"] for s, m in zip(singles[:n], members[:n])
                         for v in m.compare(s, names=ca.selected_outputs(ca.OUTPUTS_ALL)).values())
            a, b, c = (float(np.median(ms[k])) for k in "abc")
            records.emit({"measure": "kcache_batch", "precision": label, "nsets": n, "columns_per_set": columns,
                          "nproma": nproma, "klev": klev, "rounds": args.rounds, "steps": args.steps,
                          "a_single_launches": rh.summary(ms["a"]), "b_batch": rh.summary(ms["b"]),
                          "c_one_set": rh.summary(ms["c"]), "b_over_a": round(b / a, 4), "b_over_c": round(b / c, 4),
                          "a_over_n_ms": round(a / n, 4), "batch_equals_singles": differ == 0,
                          "geometry": ca.batch_launch_geometry(prec, n, columns, nproma, klev)})
            batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=16384, help="columns per set")
    ap.add_argument("--nproma", type=int, default=128)
    ap.add_argument("--nsets", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ds = ca.load_dataset()
    lib, hip, timer, records, _ = rh.begin("batch_rate", ds, EXPECTATION)
    measure(lib, hip, timer, records, ds, "fp64", ca.FP64, args.columns, args.nproma, args.nsets, args)
    measure(lib, hip, timer, records, ds, "fp32", ca.FP32, args.columns, args.nproma, [max(args.nsets)], args)
    records.write(args.out)


if __name__ == "__main__":
    main()
