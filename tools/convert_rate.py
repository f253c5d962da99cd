#!/usr/bin/env python3
"""Rate of cloudsc_fields_convert against the STREAM copy of the same run, and the cost of
"convert the inputs, run fp64 KSEG at NPROMA 64, convert the outputs back" beside the packed
NPROMA 32 KSEG step of the same process.

    python tools/convert_rate.py [--ngptot 163840] [--reps 20] [--out profiles/fields_convert/convert_rate.jsonl]

Per case the full input set (plude included) and the full output set are converted separately: two
untimed launches, then `reps` launches back to back between two events; moved bytes = bytes read +
bytes written, counted from the shapes (active columns only), over the time of one launch.  One JSON
line per measurement.  Needs an MI355X; there is no CPU form of a rate."""
import argparse
import ctypes as C

import numpy as np

import rate_harness as rh
from rate_harness import ca

INPUTS = list(ca.INPUT_FIELDS) + list(ca.INOUT_FIELDS)
OUTPUTS = [k for _, k in ca.VALIDATED]
PREC = {ca.FP64: "fp64", ca.MIXED: "float-stored"}


def moved_bytes(names, ngptot, klev, sp, dp):
    total = 0
    for n in names:
        rows = int(np.prod(ca.field_shape(ca.ALL_FIELDS[n], klev, 1)))
        es = 8 if n == "ktype" else np.dtype(ca.storage_dtype(sp)).itemsize + np.dtype(ca.storage_dtype(dp)).itemsize
        total += ngptot * rows * es
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.ngptot
    ds = ca.load_dataset()
    klev = ds.klev
    if ca.device_count() < 1:
        raise SystemExit("convert_rate: no HIP device")
    hip = rh.hip_api()
    timer, records = rh.SpanTimer(hip), rh.Records()
    stream = records.stream_copy()

    # (label, src precision, src nproma, dst precision, dst nproma)
    cases = [("fp64 32->64", ca.FP64, 32, ca.FP64, 64), ("fp64 64->64", ca.FP64, 64, ca.FP64, 64),
             ("fp64->float-stored 32->64", ca.FP64, 32, ca.MIXED, 64), ("float->fp64 64->32", ca.MIXED, 64, ca.FP64, 32),
             ("fp64 flat->64", ca.FP64, n, ca.FP64, 64), ("fp64 64->32", ca.FP64, 64, ca.FP64, 32)]
    ms_of = {}
    for label, sp, snp, dp, dnp in cases:
        a = ca.DeviceFields(n, snp, klev, sp, place=False)
        b = ca.DeviceFields(n, dnp, klev, dp, place=False)
        try:
            for name in INPUTS + OUTPUTS[1:]:
                assert hip.hipMemset(C.c_void_p(getattr(a.f, name)), 0x3c, C.c_size_t(a.nbytes(name))) == 0
            for part, names in (("inputs", INPUTS), ("outputs", OUTPUTS)):
                ms = timer.ms_per_launch(lambda: a.convert_to(b, names=names), args.reps)
                nbytes = moved_bytes(names, n, klev, sp, dp)
                gbps = nbytes / (ms * 1e-3) / 1e9
                ms_of[(label, part)] = ms
                records.emit({"measure": "convert", "case": label, "set": part, "ngptot": n, "klev": klev,
                              "src": [PREC[sp], snp], "dst": [PREC[dp], dnp], "moved_bytes": nbytes,
                              "ms": round(ms, 4), "gbps": round(gbps, 1), "of_stream_copy": round(gbps / stream, 3),
                              "reps": args.reps})
        finally:
            a.close()
            b.close()

    # the physics step either way, same process: median of 10 steps after 3
    def kseg_ms(nproma, pack):
        ca.narrow_pack(pack)
        g = ca.GpuState(ds, n, nproma, ca.FP64)
        try:
            g.run(ca.VARIANT_KSEG, 3)
            return float(np.median(g.run(ca.VARIANT_KSEG, 10)))
        finally:
            g.close()
            ca.narrow_pack(-1)

    k64 = kseg_ms(64, -1)
    k32 = kseg_ms(32, 1)
    geo = ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, n, 32, klev)
    t_in, t_out = ms_of[("fp64 32->64", "inputs")], ms_of[("fp64 64->32", "outputs")]
    records.emit({"measure": "reblock_round_trip", "ngptot": n, "convert_inputs_32_to_64_ms": round(t_in, 4),
                  "kseg_fp64_nproma64_ms": round(k64, 4), "convert_outputs_64_to_32_ms": round(t_out, 4),
                  "sum_ms": round(t_in + k64 + t_out, 4), "kseg_fp64_nproma32_packed_ms": round(k32, 4),
                  "nproma32_default_pack": geo["pack"]})
    records.write(args.out)


if __name__ == "__main__":
    main()
