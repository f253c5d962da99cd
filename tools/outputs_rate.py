#!/usr/bin/env python3
"""KSEG writing only the prognostic outputs against KSEG writing all 21: what does a caller that does not
want the ten diagnostic fluxes gain by not having them written?

    python tools/outputs_rate.py [--ngptot 163840] [--nproma 64] [--rounds 15]
                                 [--out profiles/outputs/outputs_rate.jsonl]

Per precision (fp64, mixed, fp32) one cloudsc_fields_alloc set and one cloudsc_fields_alloc_outputs(
CLOUDSC_OUTPUTS_PROGNOSTIC) set, both with their outputs placed by the library's search and expanded from
the data set.  Three cases, launched alternately in one process (a, b, c, a, b, c, ...), each launch between
its own pair of events:

  (a) cloudsc_gpu_run, KSEG, on the full set: the existing kernel (profiles/outputs/device_assembly.txt
      shows it is the parent's instruction for instruction), the yardstick
  (b) cloudsc_gpu_run_outputs(PROGNOSTIC), KSEG, on the same set: same buffers, same placement -- the
      kernel's own difference
  (c) (b) on the PROGNOSTIC set, whose ten members are NULL and whose placement was searched over the eleven
      allocated outputs: what a caller that allocates through the library gets

after `warmup` untimed rounds; median, minimum and maximum over the rounds.  plude is INOUT and is not
expanded again between launches: every case reads what the launch before it on its set left.  The STREAM
copy of the same run goes first.  One JSON line per record.  Needs an MI355X.

EXPECTATION, written before the first run (nobody had measured any of this):
  The stores per column fall to 0.58 (1,923 of 3,303 values) and the bytes a step moves to 0.80 (44,996 of
  56,036 B per fp64 column).  Two earlier measurements bracket what that buys:
    - the fp64 kernel with ALL its traffic cache-resident ran at 0.95-0.96 of the kernel on HBM (DESIGN
      3.16.4): if traffic as a whole is worth 4-5 %, a fifth of it is worth about 1 %, and even counting
      stores double (they are what stalls on DRAM write credits, 3.12) a few per cent at the most;
    - CLOUDSC_MIXED runs at 0.80 of fp64 at half the bytes (3.17), four times what that floor predicted and
      unexplained: scaled by bytes, 0.80 of the bytes would be worth about 8 %.
  Expected: the first.  (b)/(a) between 0.95 and 0.99 in fp64, the same or closer to 1 for float storage
  (half as many bytes per store, the same instruction count saved), because the mixed result most likely comes
  from something that halving EVERY access changes (cache lines per wave-level access, the loads the level
  loop waits for), which dropping write-only stores does not touch.  The ~26 VGPRs the level loop no longer
  needs change no occupancy (2 waves per SIMD either way, and a third wave was measured and set aside in
  3.16.3).  (c) against (b): within the spread of the rounds; its placement is a different draw of the same
  search, so a difference of up to a few per cent either way would be placement, not the kernel.
  A (b)/(a) below 0.93 would be the surprise and would say that stores cost more than their bytes."""
import argparse
import contextlib
import ctypes as C

import numpy as np

import rate_harness as rh
from rate_harness import ca

EXPECTATION = {"stores_ratio": 0.58, "bytes_ratio": 0.80, "expected": "a few per cent",
               "b_over_a_fp64": "0.95 to 0.99", "b_over_a_float_storage": "the same or closer to 1",
               "c_over_b": "1 within the spread of the rounds and of placements (a few per cent)",
               "surprise": "b_over_a below 0.93",
               "why": "see the EXPECTATION paragraph of tools/outputs_rate.py (DESIGN 3.12, 3.16.4, 3.17)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--nproma", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, nproma = args.ngptot, args.nproma
    ds = ca.load_dataset()
    klev = ds.klev
    lib, hip, timer, records, stream = rh.begin("outputs_rate", ds, EXPECTATION)

    for label, prec in rh.PRECISIONS:
        full = ca.DeviceFields(n, nproma, klev, prec)                                       # 21 outputs, placed
        prog = ca.DeviceFields(n, nproma, klev, prec, outputs=ca.OUTPUTS_PROGNOSTIC)        # eleven, placed
        with contextlib.closing(prog), contextlib.closing(full), \
                rh.kseg_workspace(lib, hip, prec, ca.VARIANT_KSEG, n, nproma, klev) as ws:     # freed: ws, full, prog
            full.expand(ds)
            prog.expand(ds)

            def run_a():
                ca.check(lib.cloudsc_gpu_run(0, None, prec, ca.VARIANT_KSEG, n, nproma, klev, C.byref(full.f), ws))

            def run_b():
                ca.gpu_run_outputs(full.f, prec, ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC, n, nproma, klev, scratch=ws)

            def run_c():
                ca.gpu_run_outputs(prog.f, prec, ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC, n, nproma, klev, scratch=ws)

            ms = rh.alternate(timer.ms, [("a", run_a), ("b", run_b), ("c", run_c)], args.rounds, args.warmup,
                              rh.launch_check(lib, ca.VARIANT_KSEG, ws))
            es = np.dtype(ca.storage_dtype(prec)).itemsize
            rec = {"measure": "kseg_outputs", "precision": label, "ngptot": n, "nproma": nproma, "klev": klev,
                   "rounds": args.rounds, "warmup": args.warmup,
                   "a_all": rh.summary(ms["a"]), "b_prognostic_same_set": rh.summary(ms["b"]),
                   "c_prognostic_own_set": rh.summary(ms["c"]),
                   "column_bytes_all": rh.column_bytes(klev, es, ca.OUTPUTS_ALL),
                   "column_bytes_prognostic": rh.column_bytes(klev, es, ca.OUTPUTS_PROGNOSTIC),
                   "placement_full": full.report.to_dict(), "placement_prognostic": prog.report.to_dict()}
            a, b, c = (float(np.median(ms[k])) for k in "abc")
            rec.update({"b_over_a": round(b / a, 4), "c_over_a": round(c / a, 4), "c_over_b": round(c / b, 4),
                        "a_of_stream_copy": round(rec["column_bytes_all"] * n / (a * 1e-3) / 1e9 / stream, 3),
                        "b_of_stream_copy": round(rec["column_bytes_prognostic"] * n / (b * 1e-3) / 1e9 / stream, 3)})
            records.emit(rec)
    records.write(args.out)


if __name__ == "__main__":
    main()
