#!/usr/bin/env python3
"""The prognostic step on the packed tendency buffers, and the validation of BUFFER_LOC in place: what does a
caller whose tendencies live in BUFFER_TMP / BUFFER_LOC gain from the combined form and from not unpacking?

    python tools/tendbuf_outputs_rate.py [--ngptot 163840] [--nproma 64] [--rounds 15] [--tend-planes 8]
                                         [--out profiles/tendbuf_outputs/rate.jsonl]

Per precision (fp64, mixed, fp32) one cloudsc_fields_alloc set (outputs placed by the library's search),
expanded from the data set, and two plain hipMalloc buffers of `tend_planes` planes per block, BUFFER_TMP
packed from the set's tendency_tmp_*.  Three step cases, launched alternately in one process (a, b, c, a, b,
c, ...), each launch between its own pair of events:

  (a) cloudsc_gpu_run_tendbuf, KSEG, on the set's other members and the two buffers: the parent's kernel
  (b) cloudsc_gpu_run_tendbuf_outputs(PROGNOSTIC) on the same members and buffers: the combined form
  (c) cloudsc_gpu_run_outputs(PROGNOSTIC) on the set's separate arrays: the prognostic form without buffers

after `warmup` untimed rounds; median, minimum and maximum over the rounds.  plude is INOUT and is not
expanded again between launches.  Then two validation cases, alternated the same way, each a host-clock
span from the call to its return (both wait for the stream and write stats[]):

  (v) cloudsc_fields_validate_tendbuf(tend_planes, ALL) on BUFFER_LOC in place
  (u) cloudsc_fields_convert_tendbuf (unpack BUFFER_LOC) + cloudsc_fields_validate on the separate arrays:
      the parent's entry points

The STREAM copy of the same run goes first.  One JSON line per record.  Needs an MI355X.

EXPECTATION, written before the first run (nobody had measured any of this):
  - (b)/(a): the two form bits touch disjoint functions of the level loop, so the prognostic form should buy
    on the buffers what it bought on separate arrays: near 0.87 (fp64), 0.94 (mixed), 0.84
    (fp32).  Within 0.03 of those would confirm it; above 0.97 would say the buffers' stride eats the gain.
  - (b)/(c): the buffers' cost on the prognostic form should be what it was on the full step (3.21):
    1.012-1.014, say 1.00 to 1.03.  BUFFER_LOC is one unplaced allocation, so a few per cent more would be
    placement (3.12), not the kernel.
  - (v) against (u): (u) moves BUFFER_LOC twice more (8 planes x 137 x 8 B read and written per fp64 column:
    2.9 GB at 163,840 columns, ~0.5 ms at the STREAM copy, half for float storage) before validating the
    same bytes; both validations read the 21 outputs once (24,156 B per fp64 column: 4.0 GB, ~0.7 ms at the
    copy rate, and 3.20 measured the comparison at 0.6-0.8 of it).  Expected (v)/(u) about 0.65-0.75, and
    (v) at 0.5-0.8 of the STREAM copy counting the bytes it reads."""
import argparse
import contextlib
import ctypes as C

import numpy as np

import rate_harness as rh
from rate_harness import ca

TMP = [n for n in ca.TENDENCY_FIELDS if "_tmp_" in n]
LOC = [n for n in ca.TENDENCY_FIELDS if "_loc_" in n]
EXPECTATION = {"b_over_a": {"fp64": 0.87, "mixed": 0.94, "fp32": 0.84, "within": 0.03},
               "b_over_c": "1.00 to 1.03 (3.21 measured 1.012-1.014 on the full step)",
               "validate_inplace_over_unpack_validate": "0.65 to 0.75",
               "validate_inplace_of_stream_copy": "0.5 to 0.8",
               "surprise": "b_over_a above 0.97, or b_over_c above 1.05",
               "why": "see the EXPECTATION paragraph of tools/tendbuf_outputs_rate.py (DESIGN 3.20, 3.21, 3.22)"}


def validated_bytes(klev, es):
    """Bytes of one column's 21 validated fields."""
    rows = {"2d": klev, "2dh": klev + 1, "3d": ca.NCLV * klev, "1d": 1}
    return sum(rows[ca.ALL_FIELDS[k]] * es for _, k in ca.VALIDATED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--nproma", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tend-planes", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, nproma, tp = args.ngptot, args.nproma, args.tend_planes
    ds = ca.load_dataset()
    klev = ds.klev
    lib, hip, timer, records, stream = rh.begin("tendbuf_outputs_rate", ds, EXPECTATION)
    keep = []
    ref = ca.make_reference(ds, keep)

    for label, prec in rh.PRECISIONS:
        df = ca.DeviceFields(n, nproma, klev, prec, tend_planes=tp)     # outputs placed; buffers plain hipMalloc
        with contextlib.closing(df), rh.kseg_workspace(lib, hip, prec, ca.VARIANT_KSEG, n, nproma, klev) as ws:
            check = rh.launch_check(lib, ca.VARIANT_KSEG, ws)
            df.expand(ds)                                              # the separate arrays
            ca.convert_fields_tendbuf(ca.fields_subset(df.separate, TMP), ca.fields_subset(df.f, TMP), n, klev, prec,
                                      nproma, 0, prec, nproma, tp)      # BUFFER_TMP filled
            loc_buf, loc_sep = ca.fields_subset(df.f, LOC), ca.fields_subset(df.separate, LOC)

            def run_a():
                ca.gpu_run_tendbuf(df.f, prec, ca.VARIANT_KSEG, n, nproma, klev, tp, scratch=ws)

            def run_b():
                ca.gpu_run_tendbuf_outputs(df.f, prec, ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC, n, nproma, klev, tp,
                                           scratch=ws)

            def run_c():
                ca.gpu_run_outputs(df.separate, prec, ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC, n, nproma, klev,
                                   scratch=ws)

            ms = rh.alternate(timer.ms, [("a", run_a), ("b", run_b), ("c", run_c)], args.rounds, args.warmup, check)
            a, b, c = (float(np.median(ms[k])) for k in "abc")
            records.emit({"measure": "kseg_tendbuf_outputs", "precision": label, "ngptot": n, "nproma": nproma,
                          "klev": klev, "tend_planes": tp, "rounds": args.rounds, "warmup": args.warmup,
                          "a_tendbuf_all": rh.summary(ms["a"]), "b_tendbuf_prognostic": rh.summary(ms["b"]),
                          "c_separate_prognostic": rh.summary(ms["c"]), "b_over_a": round(b / a, 4),
                          "b_over_c": round(b / c, 4), "b_over_a_expected": EXPECTATION["b_over_a"][label],
                          "placement": df.report.to_dict()})

            # all 21 outputs in both places: one full step on the buffers, BUFFER_LOC unpacked once
            run_a()
            check()
            stats_sep = (ca.Stats * len(ca.VALIDATED))()

            def val_inplace():
                ca.validate_fields_tendbuf(df.f, ref, prec, n, nproma, klev, tp, ca.OUTPUTS_ALL)

            def val_unpack():
                ca.convert_fields_tendbuf(loc_buf, loc_sep, n, klev, prec, nproma, tp, prec, nproma, 0)
                ca.check(lib.cloudsc_fields_validate(0, None, prec, n, nproma, klev, 0, C.byref(df.separate),
                                                     C.byref(ref), stats_sep))

            vms = rh.alternate(rh.host_ms, [("v", val_inplace), ("u", val_unpack)], args.rounds, args.warmup)
            v, u = (float(np.median(vms[k])) for k in "vu")
            es = np.dtype(ca.storage_dtype(prec)).itemsize
            vb = validated_bytes(klev, es)
            records.emit({"measure": "validate_tendbuf", "precision": label, "ngptot": n, "nproma": nproma,
                          "klev": klev, "tend_planes": tp, "rounds": args.rounds, "warmup": args.warmup,
                          "v_inplace": rh.summary(vms["v"]), "u_unpack_then_validate": rh.summary(vms["u"]),
                          "v_over_u": round(v / u, 4), "u_minus_v_ms": round(u - v, 4), "validated_column_bytes": vb,
                          "v_of_stream_copy": round(vb * n / (v * 1e-3) / 1e9 / stream, 3)})
    records.write(args.out)


if __name__ == "__main__":
    main()
