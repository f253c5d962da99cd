"""What the step-rate and field-rate tools (tools/*_rate.py) share: the HIP handle, the KSEG workspace, the
event and host clocks, the two round loops, the summaries and the JSON records.  A tool keeps its docstring,
its EXPECTATION, its argument parser, its field sets and step closures and the record it emits; how a launch
is timed, what counts as a round and where the workspace is cleared is decided here, once.
Plain functions and two small classes; nothing here runs at import, so `--help` needs no GPU."""
import contextlib
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dwarf-p-cloudsc_amd"))
import cloudsc_amd as ca  # noqa: E402

PRECISION = {"fp64": ca.FP64, "mixed": ca.MIXED, "fp32": ca.FP32}
PRECISIONS = list(PRECISION.items())
VARIANT = {"kseg": ca.VARIANT_KSEG, "kcache": ca.VARIANT_KCACHE}
OUTPUTS = {"all": ca.OUTPUTS_ALL, "prognostic": ca.OUTPUTS_PROGNOSTIC, "surface": ca.OUTPUTS_SURFACE}


def hip_api():
    """ca._hip() with the prototypes of the calls the tools make beyond the binding's own."""
    hip = ca._hip()
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return hip


def gpu_init(lib, ds):
    """The data set's parameters as device 0's default set (the library keeps its own copy)."""
    p = ca.Params.from_dict(ds.params)
    ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))


@contextlib.contextmanager
def device_buffer(hip, nbytes, fill=None):
    """A plain hipMalloc buffer, freed on the way out whatever happens.  fill: a byte value for the whole
    buffer, or a host array of nbytes to copy in."""
    q = C.c_void_p()
    assert hip.hipMalloc(C.byref(q), C.c_size_t(nbytes)) == 0
    try:
        if isinstance(fill, int):
            assert hip.hipMemset(q, fill, C.c_size_t(nbytes)) == 0
        elif fill is not None:
            assert hip.hipMemcpy(q, fill.ctypes.data, nbytes, 1) == 0
        yield q
    finally:
        hip.hipFree(q)


@contextlib.contextmanager
def kseg_workspace(lib, hip, precision, variant, ngptot, nproma, klev):
    """The variant's workspace with its first 256 bytes (the KSEG queue heads) cleared, freed on the way out;
    a NULL pointer and no allocation where the variant needs none (KCACHE)."""
    nbytes = lib.cloudsc_gpu_scratch_bytes(precision, variant, ngptot, nproma, klev)
    assert nbytes >= 0
    if nbytes == 0:
        yield C.c_void_p()
        return
    with device_buffer(hip, nbytes) as ws:
        assert hip.hipMemset(ws, 0, C.c_size_t(256)) == 0
        yield ws


def launch_check(lib, variant, ws):
    """The call after a launch: cloudsc_gpu_check waits for it and raises on what the kernel flagged."""
    return lambda: ca.check(lib.cloudsc_gpu_check(0, None, variant, ws))


class SpanTimer:
    """Two events on the default stream.  ms: one launch sequence between them, waited for."""

    def __init__(self, hip):
        self.hip = hip
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(self.e0)) == 0 and hip.hipEventCreate(C.byref(self.e1)) == 0

    def _span(self, launch, reps):
        assert self.hip.hipEventRecord(self.e0, None) == 0
        for _ in range(reps):
            launch()
        assert self.hip.hipEventRecord(self.e1, None) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value

    def ms(self, launch):
        return self._span(launch, 1)

    def ms_per_launch(self, launch, reps, warmup=2):
        """`warmup` untimed launches, a device synchronisation, then `reps` launches back to back in one span."""
        for _ in range(warmup):
            launch()
        assert self.hip.hipDeviceSynchronize() == 0
        return self._span(launch, reps) / reps


def host_ms(call):
    """A call on the host clock, from the call to its return: for calls that wait for their own work."""
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def alternate(clock, cases, rounds, warmup, after_launch=None):
    """The cases [(key, launch)] in turn (a, b, c, a, b, c, ...), each timed by clock(launch) -- SpanTimer.ms
    or host_ms -- and followed by after_launch(); the first `warmup` rounds are run the same way and not kept."""
    ms = {key: [] for key, _ in cases}
    for r in range(warmup + rounds):
        for key, launch in cases:
            t = clock(launch)
            if after_launch:
                after_launch()
            if r >= warmup:
                ms[key].append(t)
    return ms


def host_clock_rounds(hip, step, steps, rounds, before_round=None):
    """Per round: before_round() (untimed), then `steps` back-to-back launches between two device
    synchronisations on the host clock.  ms per step of every round."""
    ms = []
    for _ in range(rounds):
        if before_round:
            before_round()
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        hip.hipDeviceSynchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    return ms


def what_rounds(hip, step, o, check, before_round=None):
    """One process of the --what family: o.warmup launches, the check, the host-clock rounds, the check."""
    for _ in range(o.warmup):
        step()
    check()
    ms = host_clock_rounds(hip, step, o.steps, o.rounds, before_round)
    check()
    return ms


def summary(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def column_bytes(klev, es, outputs):
    """Bytes one column moves in a step: every input read once, every selected output written once."""
    read = sum(int(np.prod(ca.field_shape(k, klev, 1))) * (4 if n == "ktype" else es)
               for n, k in {**ca.INPUT_FIELDS, **ca.INOUT_FIELDS}.items())
    read -= 2 * klev * es                   # tendency_tmp_cld, pclv: four of the five species planes are read
    written = sum(int(np.prod(ca.selected_field_shape(n, klev, 1, outputs))) * es for n in ca.selected_outputs(outputs))
    return read + written


def lib_label():
    return "CLOUDSC_AMD_LIB" if os.environ.get("CLOUDSC_AMD_LIB") else "this build"


def what_record(o, ms, keys, **extra):
    """The one line of a --what process: `keys` in their order, from extra or else from the options, then the
    library's stamp, every round's ms per step and their median."""
    rec = {k: extra[k] if k in extra else getattr(o, k) for k in keys}
    rec.update({"lib": lib_label(), "ms_per_step": [round(x, 4) for x in ms],
                "median_ms": round(statistics.median(ms), 4)})
    return rec


class Records:
    """The records of a run: each printed as one JSON line when it is made, all of them written by write()."""

    def __init__(self):
        self.lines = []

    def emit(self, rec):
        self.lines.append(rec)
        print(json.dumps(rec), flush=True)

    def stream_copy(self, **extra):
        """The STREAM copy of this run (4 GiB, 10 repetitions): emitted, and returned in GB/s."""
        gbps = ca.hbm_copy_gbps(0, 4 << 30, 10)
        self.emit({"measure": "stream_copy", "gbps": round(gbps, 1), **extra})
        return gbps

    def write(self, path, append=False):
        """--out: nothing without a path; the directory is made if it is missing."""
        if not path:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a" if append else "w") as fh:
            for rec in self.lines:
                fh.write(json.dumps(rec) + "\n")


def begin(tool, ds, expectation):
    """What an alternating step-rate tool does before its first field set: the device, the events, the
    expectation and STREAM copy records, the parameters.  Returns lib, hip, timer, records, stream GB/s."""
    if ca.device_count() < 1:
        raise SystemExit("%s: no HIP device" % tool)
    lib, hip = ca.gpu_lib(), hip_api()
    timer, rec = SpanTimer(hip), Records()
    rec.emit({"measure": "expectation", **expectation})
    stream = rec.stream_copy()
    gpu_init(lib, ds)
    return lib, hip, timer, rec, stream
