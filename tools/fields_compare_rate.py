#!/usr/bin/env python3
"""Rate of cloudsc_fields_compare and cloudsc_fields_validate against the STREAM copy of the same run,
beside what the same judgement costs without them: 21 downloads plus NumPy, and cloudsc_state_validate.

    python tools/fields_compare_rate.py [--ngptot 163840] [--reps 20] [--out profiles/fields_compare/compare_rate.jsonl]

Expectation, written before the first run: the kernel issues cloudsc_fields_convert's loads and no stores,
so each case should reach at least the fraction of the STREAM copy convert recorded for the same shapes,
0.80-0.93.  A case below 0.5 needs its access pattern explained, or is a negative result.

Per case the full output set of one field set is compared with that of another: two untimed calls, then
`reps` calls between two events on the default stream (each call waits for its own launch, so the span
holds the launches, the result copies and the host's waits).  Bytes read = the elements of both
operands (validate: the set's elements; the 100-column reference stays in the caches), counted from the
shapes, active columns only.  One JSON line per measurement.  Needs an MI355X."""
import argparse
import ctypes as C
import time

import numpy as np

import rate_harness as rh
from rate_harness import ca

OUTPUTS = [k for _, k in ca.VALIDATED]
PREC = {ca.FP64: "fp64", ca.MIXED: "float-stored"}
EXPECTED = [0.80, 0.93]


def read_bytes(names, ngptot, klev, precisions):
    total = 0
    for n in names:
        rows = int(np.prod(ca.field_shape(ca.ALL_FIELDS[n], klev, 1)))
        total += ngptot * rows * sum(np.dtype(ca.storage_dtype(p)).itemsize for p in precisions)
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
        raise SystemExit("fields_compare_rate: no HIP device")
    lib, hip = ca.gpu_lib(), rh.hip_api()
    timer, records = rh.SpanTimer(hip), rh.Records()
    emit = records.emit
    stream = records.stream_copy(expected_of_stream_copy=EXPECTED)

    def fill(df):
        for name in OUTPUTS:
            assert hip.hipMemset(C.c_void_p(getattr(df.f, name)), 0x3c, C.c_size_t(df.nbytes(name))) == 0

    # (label, a precision, a nproma, b precision, b nproma)
    cases = [("fp64 64/64", ca.FP64, 64, ca.FP64, 64), ("fp64 64/32", ca.FP64, 64, ca.FP64, 32),
             ("fp64 64/flat", ca.FP64, 64, ca.FP64, n), ("fp64/float-stored 64/64", ca.FP64, 64, ca.MIXED, 64)]
    for label, ap_, anp, bp, bnp in cases:
        a = ca.DeviceFields(n, anp, klev, ap_, place=False)
        b = ca.DeviceFields(n, bnp, klev, bp, place=False)
        try:
            fill(a)
            fill(b)
            ms = timer.ms_per_launch(lambda: a.compare(b, names=OUTPUTS), args.reps)
            nbytes = read_bytes(OUTPUTS, n, klev, (ap_, bp))
            gbps = nbytes / (ms * 1e-3) / 1e9
            emit({"measure": "compare", "case": label, "set": "outputs", "ngptot": n, "klev": klev,
                  "a": [PREC[ap_], anp], "b": [PREC[bp], bnp], "read_bytes": nbytes, "ms": round(ms, 4),
                  "gbps": round(gbps, 1), "of_stream_copy": round(gbps / stream, 3), "reps": args.reps})
            if label == "fp64 64/64":
                # what the tests do today for one output set: 21 downloads as doubles, then NumPy
                t0 = time.perf_counter()
                x = {k: a.download(k) for k in OUTPUTS}
                t1 = time.perf_counter()
                same = all(np.array_equal(ca.blocks_to_columns(x[k], n), ca.blocks_to_columns(x[k], n)) for k in OUTPUTS)
                t2 = time.perf_counter()
                emit({"measure": "download_and_numpy", "set": "outputs", "ngptot": n, "sets_downloaded": 1,
                      "download_ms": round(1e3 * (t1 - t0), 1), "numpy_equal_ms": round(1e3 * (t2 - t1), 1),
                      "equal": bool(same)})
                del x
        finally:
            a.close()
            b.close()

    # validation: the state's own against cloudsc_fields_validate on the state's fields
    lib.cloudsc_set_placement_search(0)
    g = ca.GpuState(ds, n, 64, ca.FP64)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        f = ca.Fields()
        ca.check(lib.cloudsc_state_fields(g.h, C.byref(f)))
        keep = []
        ref = ca.make_reference(ds, keep)
        st = (ca.Stats * 21)()

        def fields_validate():
            ca.check(lib.cloudsc_fields_validate(0, None, ca.FP64, n, 64, klev, 0, C.byref(f), C.byref(ref), st))
        ms = timer.ms_per_launch(fields_validate, args.reps)
        nbytes = read_bytes(OUTPUTS, n, klev, (ca.FP64,))
        gbps = nbytes / (ms * 1e-3) / 1e9
        emit({"measure": "fields_validate", "ngptot": n, "nproma": 64, "precision": "fp64", "read_bytes": nbytes,
              "ms": round(ms, 4), "gbps": round(gbps, 1), "of_stream_copy": round(gbps / stream, 3), "reps": args.reps})
        got = [(s.minval, s.maxval, s.maxerr, s.errsum, s.refsum) for s in st]
        g.validate()
        t0 = time.perf_counter()
        for _ in range(3):
            want = g.validate()
        state_ms = 1e3 * (time.perf_counter() - t0) / 3
        t0 = time.perf_counter()
        for _ in range(3):
            fields_validate()
        fields_ms = 1e3 * (time.perf_counter() - t0) / 3
        emit({"measure": "validate_wall", "ngptot": n, "state_validate_ms": round(state_ms, 2),
              "fields_validate_ms": round(fields_ms, 2), "same_table": got == [w[:5] for w in want]})
    finally:
        g.close()
        lib.cloudsc_set_placement_search(-1)
    records.write(args.out)


if __name__ == "__main__":
    main()
