#!/usr/bin/env python3
"""Rate of cloudsc_fields_convert_layout against two baselines of the same process: the plain
cloudsc_fields_convert fp64 64 -> 64 on the same sets (the same bytes, no transpose) and the STREAM copy.

    python tools/fields_layout_rate.py [--ngptot 163840] [--reps 20] [--out profiles/fields_layout/rate.jsonl]
    python tools/fields_layout_rate.py --ab --label lds|naive [--lib build/liblayout_naive.so]

Per case the full input set (plude included) and the full output set are converted separately: two untimed
launches, then `reps` launches back to back between two events; moved bytes = bytes read + bytes written,
counted from the shapes, over the time of one launch.  One JSON line per measurement.

--ab: the two fp64 cases only, for alternating the product library with the form without an LDS tile
(make variant VFLAGS=-DCLOUDSC_LAYOUT_NAIVE OUT=...): four rounds, the order swapped every round, each
process under a time limit of its own, given by the caller, and the processes chained so that a failure ends
the sequence (a process that faulted must not be followed by another on the same card):

    L="timeout -k 10 150 python tools/fields_layout_rate.py --ab --out profiles/fields_layout/rate_ab.jsonl"
    N="--label naive --lib build/liblayout_naive.so"
    $L --label lds && $L $N && $L $N && $L --label lds && $L --label lds && $L $N && $L $N && $L --label lds

The tile ships if its mean is better than the naive form's by more than
the larger of the two ranges over the rounds.

Expectation, written before the first run.  The tile form reads and writes both sides in runs of at
least 64 bytes and moves every byte once: it should reach at least 0.5 of the STREAM copy of the same run
in fp64 in both directions (the project's line), and stay below the plain convert,
whose runs are 512 bytes on both sides.  The naive form strides its LEVELS side by rows * 8 bytes per lane:
a wave's access touches 64 lines for 512 useful bytes, and only the 16 rows of an item reuse a line, so it
should be well under the tile form, by a factor of two or more.  The narrowing and widening cases move
fewer bytes in about the same time per element, so their GB/s should be lower than the fp64 cases'.
Needs an MI355X; there is no CPU form of a rate."""
import argparse
import ctypes as C

import numpy as np

import rate_harness as rh
from convert_rate import INPUTS, OUTPUTS, PREC, moved_bytes
from rate_harness import ca

L, B = ca.LAYOUT_LEVELS, ca.LAYOUT_BLOCKED


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--label", default="lds")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    n = args.ngptot
    ca.gpu_lib(args.lib)
    ds = ca.load_dataset()
    klev = ds.klev
    if ca.device_count() < 1:
        raise SystemExit("fields_layout_rate: no HIP device")
    hip = rh.hip_api()
    timer, records = rh.SpanTimer(hip), rh.Records()
    emit = records.emit

    def sets(sp, sl, snp, dp, dl, dnp):
        a = ca.DeviceFields(n, snp, klev, sp, place=False, layout=sl)
        b = ca.DeviceFields(n, dnp, klev, dp, place=False, layout=dl)
        for name in INPUTS + OUTPUTS[1:]:
            assert hip.hipMemset(C.c_void_p(getattr(a.f, name)), 0x3c, C.c_size_t(a.nbytes(name))) == 0
        return a, b

    def measure(sp, sl, snp, dp, dl, dnp):
        a, b = sets(sp, sl, snp, dp, dl, dnp)
        try:
            out = {}
            for part, names in (("inputs", INPUTS), ("outputs", OUTPUTS)):
                ms = timer.ms_per_launch(lambda: a.convert_to(b, names=names), args.reps)
                nbytes = moved_bytes(names, n, klev, sp, dp)
                out[part] = (ms, nbytes, nbytes / (ms * 1e-3) / 1e9)
            return out
        finally:
            a.close()
            b.close()

    if args.ab:
        rec = {"measure": "layout_ab", "form": args.label, "ngptot": n, "reps": args.reps}
        for label, sl, snp, dl, dnp in (("l2b", L, 0, B, 64), ("b2l", B, 64, L, 0)):
            r = measure(ca.FP64, sl, snp, ca.FP64, dl, dnp)
            for part in ("inputs", "outputs"):
                rec["%s_%s_ms" % (label, part)] = round(r[part][0], 4)
        emit(rec)
    else:
        stream = records.stream_copy()
        plain = measure(ca.FP64, B, 64, ca.FP64, B, 64)
        for part in ("inputs", "outputs"):
            ms, nbytes, gbps = plain[part]
            emit({"measure": "plain_convert", "case": "fp64 B(64)->B(64)", "set": part, "ngptot": n, "klev": klev,
                  "moved_bytes": nbytes, "ms": round(ms, 4), "gbps": round(gbps, 1),
                  "of_stream_copy": round(gbps / stream, 3), "reps": args.reps})
        cases = [("fp64 L->B(64)", ca.FP64, L, 0, ca.FP64, B, 64), ("fp64 B(64)->L", ca.FP64, B, 64, ca.FP64, L, 0),
                 ("fp64 L->float-stored B(64)", ca.FP64, L, 0, ca.MIXED, B, 64),
                 ("float-stored B(64)->fp64 L", ca.MIXED, B, 64, ca.FP64, L, 0),
                 ("fp64 L->B(32)", ca.FP64, L, 0, ca.FP64, B, 32)]
        ms_of = {}
        for label, sp, sl, snp, dp, dl, dnp in cases:
            r = measure(sp, sl, snp, dp, dl, dnp)
            for part in ("inputs", "outputs"):
                ms, nbytes, gbps = r[part]
                ms_of[(label, part)] = ms
                emit({"measure": "convert_layout", "case": label, "set": part, "ngptot": n, "klev": klev,
                      "src": PREC[sp], "dst": PREC[dp], "moved_bytes": nbytes, "ms": round(ms, 4),
                      "gbps": round(gbps, 1), "of_stream_copy": round(gbps / stream, 3),
                      "time_over_plain_convert": round(ms / plain[part][0], 3), "reps": args.reps})
        # does converting pay: the inputs once, the outputs after every step, against the step
        g = ca.GpuState(ds, n, 64, ca.FP64)
        try:
            g.run(ca.VARIANT_KSEG, 3)
            k64 = float(np.median(g.run(ca.VARIANT_KSEG, 10)))
        finally:
            g.close()
        emit({"measure": "levels_round_trip", "ngptot": n,
              "convert_inputs_l2b_ms": round(ms_of[("fp64 L->B(64)", "inputs")], 4),
              "kseg_fp64_nproma64_ms": round(k64, 4),
              "convert_outputs_b2l_ms": round(ms_of[("fp64 B(64)->L", "outputs")], 4)})
    records.write(args.out, append=args.ab)


if __name__ == "__main__":
    main()
