#!/usr/bin/env python3
"""KSEG on the reference Fortran drivers' packed tendency buffers against KSEG on separate arrays, and
against "unpack, run on separate arrays, pack": which way should a caller whose tendencies live in
BUFFER_TMP / BUFFER_LOC go?

    python tools/tendbuf_rate.py [--ngptot 163840] [--nproma 64] [--rounds 15] [--tend-planes 8]
                                 [--out profiles/tendbuf/tendbuf_rate.jsonl]

Per precision (fp64, mixed, fp32) one cloudsc_fields_alloc set (outputs placed by the library's search),
expanded from the data set, and two plain hipMalloc buffers of `tend_planes` planes per block.  Three cases,
launched alternately in one process (a, b, c, a, b, c, ...), each launch between its own pair of events:

  (a) cloudsc_gpu_run, KSEG, on the set's separate arrays: the existing path, the yardstick
  (b) cloudsc_gpu_run_tendbuf, KSEG, on the set's other members and the two buffers
  (c) unpack BUFFER_TMP into the separate tendency_tmp_* arrays + (a) + pack tendency_loc_* into BUFFER_LOC:
      what a buffer-resident caller pays without (b); one event span over the three launches

after `warmup` untimed rounds; median, minimum and maximum over the rounds.  plude is INOUT and is not
expanded again between launches: every case reads what the launch before it left, the same for all three as
they alternate.  The STREAM copy of the same run goes first.  One JSON line per record.  Needs an MI355X.

EXPECTATION, written before the first run (nobody had measured any of this):
  - (b) against (a): slower, by up to the 16 % that the per-block interleave of the WHOLE field set
    measured, probably by much less since only 16 of the step's ~130 level planes per block
    are interleaved; and BUFFER_LOC is one unplaced allocation where (a)'s outputs are placed (3.12), which
    measured up to ~15 % between placements of all 21 outputs -- 8 of the 2 x 16 output planes here.  A (b)
    equal to (a) within the spread of the rounds would be the good surprise; faster is not expected.
  - (c) against (a): the two conversions move 2 x 2 x 8 planes x 137 x 8 B = 35 KB per fp64 column, 5.7 GB
    at 163,840 columns, at 0.85-1.0 of the STREAM copy (3.19): about 1.0 ms on top of (a)'s ~1.7 ms in
    fp64, half of that for float storage.
  - so (b) should beat (c) clearly, by ~0.7 ms or more in fp64, even if it is 16 % slower than (a)."""
import argparse
import contextlib
import ctypes as C

import numpy as np

import rate_harness as rh
from rate_harness import ca

TMP = [n for n in ca.TENDENCY_FIELDS if "_tmp_" in n]
LOC = [n for n in ca.TENDENCY_FIELDS if "_loc_" in n]
EXPECTATION = {"b_over_a": "1.00 to 1.16, most likely a few percent above 1", "c_minus_a_ms_fp64": "about 1.0",
               "c_minus_a_ms_float_storage": "about 0.5", "b_beats_c": True,
               "why": "see the EXPECTATION paragraph of tools/tendbuf_rate.py (DESIGN 3.12, 3.16.1, 3.19)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--nproma", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tend-planes", type=int, default=ca.TENDBUF_PLANES_MIN)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, nproma, tp = args.ngptot, args.nproma, args.tend_planes
    ds = ca.load_dataset()
    klev = ds.klev
    lib, hip, timer, records, stream = rh.begin("tendbuf_rate", ds, EXPECTATION)

    for label, prec in rh.PRECISIONS:
        df = ca.DeviceFields(n, nproma, klev, prec, tend_planes=tp)     # outputs placed; buffers plain hipMalloc
        with contextlib.closing(df), rh.kseg_workspace(lib, hip, prec, ca.VARIANT_KSEG, n, nproma, klev) as ws:
            sep, buf = df.separate, df.f
            assert hip.hipMemset(df.buffer_tmp, 0, C.c_size_t(df.tendbuf_nbytes())) == 0
            assert hip.hipMemset(df.buffer_loc, 0, C.c_size_t(df.tendbuf_nbytes())) == 0
            df.expand(ds)                                               # the separate arrays
            tmp_sep, tmp_buf = ca.fields_subset(sep, TMP), ca.fields_subset(buf, TMP)
            loc_sep, loc_buf = ca.fields_subset(sep, LOC), ca.fields_subset(buf, LOC)
            ca.convert_fields_tendbuf(tmp_sep, tmp_buf, n, klev, prec, nproma, 0, prec, nproma, tp)   # BUFFER_TMP filled

            def run_a():
                ca.check(lib.cloudsc_gpu_run(0, None, prec, ca.VARIANT_KSEG, n, nproma, klev, C.byref(sep), ws))

            def run_b():
                ca.gpu_run_tendbuf(buf, prec, ca.VARIANT_KSEG, n, nproma, klev, tp, scratch=ws)

            def run_c():
                ca.convert_fields_tendbuf(tmp_buf, tmp_sep, n, klev, prec, nproma, tp, prec, nproma, 0)
                run_a()
                ca.convert_fields_tendbuf(loc_sep, loc_buf, n, klev, prec, nproma, 0, prec, nproma, tp)

            ms = rh.alternate(timer.ms, [("a", run_a), ("b", run_b), ("c", run_c)], args.rounds, args.warmup,
                              rh.launch_check(lib, ca.VARIANT_KSEG, ws))
            es = np.dtype(ca.storage_dtype(prec)).itemsize
            conv_bytes = 2 * 2 * 8 * klev * n * es          # two conversions, read + write, 8 planes each
            rec = {"measure": "kseg_tendbuf", "precision": label, "ngptot": n, "nproma": nproma, "klev": klev,
                   "tend_planes": tp, "rounds": args.rounds, "warmup": args.warmup,
                   "a_plain": rh.summary(ms["a"]), "b_tendbuf": rh.summary(ms["b"]),
                   "c_unpack_run_pack": rh.summary(ms["c"]), "conversion_bytes": conv_bytes}
            a, b, c = (float(np.median(ms[k])) for k in "abc")
            rec.update({"b_over_a": round(b / a, 4), "c_over_a": round(c / a, 4), "c_minus_a_ms": round(c - a, 4),
                        "b_minus_c_ms": round(b - c, 4),
                        "conversions_of_stream_copy": round(conv_bytes / ((c - a) * 1e-3) / 1e9 / stream, 3) if c > a else None})
            records.emit(rec)
    records.write(args.out)


if __name__ == "__main__":
    main()
