#!/usr/bin/env python3
"""KSEG with the four precipitation / enthalpy fluxes at the surface only (CLOUDSC_OUTPUTS_SURFACE) against
the prognostic step that writes their whole profiles (CLOUDSC_OUTPUTS_PROGNOSTIC): how much of the removed
store traffic shows up as time?

    python tools/outputs_surface_rate.py [--ngptot 163840] [--nproma 64] [--rounds 15]
                                         [--out profiles/outputs_surface/outputs_surface_rate.jsonl]

Per precision (fp64, mixed, fp32) one cloudsc_fields_alloc_outputs(PROGNOSTIC) set and one
cloudsc_fields_alloc_outputs(SURFACE) set, both placed by the library's search and expanded from the data
set.  Three cases, launched alternately in one process (a, b, c, a, b, c, ...), each launch between its own
pair of events:

  (a) cloudsc_gpu_run_outputs(PROGNOSTIC), KSEG, on the PROGNOSTIC set: the existing kernel
      (profiles/outputs_surface/device_assembly.txt shows it is the parent's instruction for instruction)
  (b) cloudsc_gpu_run_outputs(SURFACE), KSEG, on that same set's buffers, its four flux members replaced by
      four small scratch arrays [nblocks][nproma]: same buffers, same placement -- the kernel's own difference
  (c) SURFACE on the SURFACE set, whose placement was searched over seven full-size outputs and four small
      ones: what a caller that allocates through the library gets

after `warmup` untimed rounds; median, minimum and maximum over the rounds.  plude is INOUT and is not expanded
again between launches: every case reads what the launch before it on its set left.  The STREAM copy of the
same run goes first.  One JSON line per record.  Needs an MI355X.

EXPECTATION, written before the first run:
  Against the prognostic step the stores per column fall from 1,923 to 1,375 values (4 * klev fewer, 0.715) and
  the bytes a step moves from 44,996 to 40,612 B per fp64 column (0.903).  The prognostic step gained 12.8 % in
  fp64 from dropping ten of fourteen half-level store streams and 19.7 % of the bytes; scaled by bytes these four
  streams are worth about a third of that, 3 to 5 % in fp64, and less for float storage.  No speed-up is
  promised: the bar is that (b) is not slower than (a) beyond the spread of (a)'s own rounds.  (c) against (b)
  is a different draw of the placement search: a few per cent either way would be placement, not the kernel."""
import argparse
import contextlib

import numpy as np

import rate_harness as rh
from rate_harness import ca

EXPECTATION = {"stores_ratio_vs_prognostic": 0.715, "bytes_ratio_vs_prognostic": 0.903,
               "b_over_a_fp64": "0.95 to 0.97", "b_over_a_float_storage": "closer to 1",
               "bar": "b not slower than a beyond the spread of a's rounds; a neutral result is recorded as such",
               "c_over_b": "1 within the spread of the rounds and of placements (a few per cent)"}


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
    lib, hip, timer, records, stream = rh.begin("outputs_surface_rate", ds, EXPECTATION)

    for label, prec in rh.PRECISIONS:
        prog = ca.DeviceFields(n, nproma, klev, prec, outputs=ca.OUTPUTS_PROGNOSTIC)   # eleven outputs, placed
        surf = ca.DeviceFields(n, nproma, klev, prec, outputs=ca.OUTPUTS_SURFACE)      # seven and four small, placed
        with contextlib.closing(surf), contextlib.closing(prog), contextlib.ExitStack() as small, \
                rh.kseg_workspace(lib, hip, prec, ca.VARIANT_KSEG, n, nproma, klev) as ws:     # freed: ws, small, prog, surf
            prog.expand(ds)
            surf.expand(ds)
            # (b): the PROGNOSTIC set's buffers, the four flux members small scratch arrays
            same = ca.fields_subset(prog.f)
            for name in ca.SURFACE_FLUX_FIELDS:
                setattr(same, name, small.enter_context(rh.device_buffer(hip, surf.nbytes(name))).value)

            def run_a():
                ca.gpu_run_outputs(prog.f, prec, ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC, n, nproma, klev, scratch=ws)

            def run_b():
                ca.gpu_run_outputs(same, prec, ca.VARIANT_KSEG, ca.OUTPUTS_SURFACE, n, nproma, klev, scratch=ws)

            def run_c():
                ca.gpu_run_outputs(surf.f, prec, ca.VARIANT_KSEG, ca.OUTPUTS_SURFACE, n, nproma, klev, scratch=ws)

            ms = rh.alternate(timer.ms, [("a", run_a), ("b", run_b), ("c", run_c)], args.rounds, args.warmup,
                              rh.launch_check(lib, ca.VARIANT_KSEG, ws))
            es = np.dtype(ca.storage_dtype(prec)).itemsize
            rec = {"measure": "kseg_outputs_surface", "precision": label, "ngptot": n, "nproma": nproma, "klev": klev,
                   "rounds": args.rounds, "warmup": args.warmup,
                   "a_prognostic": rh.summary(ms["a"]), "b_surface_same_set": rh.summary(ms["b"]),
                   "c_surface_own_set": rh.summary(ms["c"]),
                   "column_bytes_prognostic": rh.column_bytes(klev, es, ca.OUTPUTS_PROGNOSTIC),
                   "column_bytes_surface": rh.column_bytes(klev, es, ca.OUTPUTS_SURFACE),
                   "placement_prognostic": prog.report.to_dict(), "placement_surface": surf.report.to_dict()}
            a, b, c = (float(np.median(ms[k])) for k in "abc")
            spread_a = (float(np.max(ms["a"])) - float(np.min(ms["a"]))) / a
            rec.update({"b_over_a": round(b / a, 4), "c_over_a": round(c / a, 4), "c_over_b": round(c / b, 4),
                        "a_spread": round(spread_a, 4), "b_within_bar": bool(b <= a * (1.0 + spread_a)),
                        "a_of_stream_copy": round(rec["column_bytes_prognostic"] * n / (a * 1e-3) / 1e9 / stream, 3),
                        "b_of_stream_copy": round(rec["column_bytes_surface"] * n / (b * 1e-3) / 1e9 / stream, 3)})
            records.emit(rec)
    records.write(args.out)


if __name__ == "__main__":
    main()
