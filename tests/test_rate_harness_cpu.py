"""tools/rate_harness.py without a GPU: a fake HIP handle records every call and hands out scripted elapsed
times, so the order of launches, synchronisations and clock reads -- the measurement procedure the ten
tools/*_rate.py share -- is asserted call by call, as are the workspace's clear and release, the roundings and
the records.  The last tests hold the ten tools to the split: none keeps a copy of a harness piece."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cloudsc_amd as ca
import rate_harness as rh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["tendbuf_rate", "outputs_rate", "outputs_surface_rate", "tendbuf_outputs_rate", "tendbuf_cml_rate",
         "spp_rate", "advance_rate", "convert_rate", "fields_compare_rate", "fields_layout_rate"]


class FakeHip:
    """The HIP calls of the harness: each appends to self.calls and succeeds; events and buffers get
    distinct handles, hipEventElapsedTime hands out the scripted times in turn."""

    def __init__(self, elapsed=()):
        self.calls, self.elapsed, self.handle = [], list(elapsed), 0x1000

    def _new(self, ref):
        self.handle += 0x100
        ref._obj.value = self.handle
        return self.handle

    def hipEventCreate(self, ref):
        self._new(ref)
        return 0

    def hipEventRecord(self, ev, stream):
        assert stream is None
        self.calls.append(("record", ev.value))
        return 0

    def hipEventSynchronize(self, ev):
        self.calls.append(("event_sync", ev.value))
        return 0

    def hipEventElapsedTime(self, ref, e0, e1):
        ref._obj.value = self.elapsed.pop(0)
        self.calls.append(("elapsed", e0.value, e1.value))
        return 0

    def hipDeviceSynchronize(self):
        self.calls.append(("sync",))
        return 0

    def hipMalloc(self, ref, nbytes):
        self.calls.append(("malloc", self._new(ref), nbytes.value))
        return 0

    def hipMemset(self, q, byte, nbytes):
        self.calls.append(("memset", q.value, byte, nbytes.value))
        return 0

    def hipMemcpy(self, q, src, nbytes, kind):
        self.calls.append(("memcpy", q.value, src, nbytes, kind))
        return 0

    def hipFree(self, q):
        self.calls.append(("free", q.value))
        return 0


class FakeLib:
    def __init__(self, scratch_bytes):
        self.scratch_bytes, self.asked = scratch_bytes, []

    def cloudsc_gpu_scratch_bytes(self, *args):
        self.asked.append(args)
        return self.scratch_bytes


def test_alternate_runs_abc_five_times_checks_every_launch_and_keeps_the_last_three():
    log, times = [], iter(range(100, 115))

    def clock(launch):
        launch()
        return next(times)

    cases = [(k, lambda k=k: log.append(k)) for k in "abc"]
    ms = rh.alternate(clock, cases, rounds=3, warmup=2, after_launch=lambda: log.append("check"))
    assert log == ["a", "check", "b", "check", "c", "check"] * 5          # warm-up rounds included
    assert ms == {"a": [106, 109, 112], "b": [107, 110, 113], "c": [108, 111, 114]}
    assert list(ms) == ["a", "b", "c"]


def test_alternate_without_a_check_and_on_the_host_clock(monkeypatch):
    ticks = iter([0.0, 0.001, 1.0, 1.002, 2.0, 2.004, 3.0, 3.008])
    monkeypatch.setattr(rh.time, "perf_counter", lambda: next(ticks))
    log = []
    ms = rh.alternate(rh.host_ms, [("v", lambda: log.append("v")), ("u", lambda: log.append("u"))], rounds=1, warmup=1)
    assert log == ["v", "u", "v", "u"]
    assert ms["v"] == pytest.approx([4.0]) and ms["u"] == pytest.approx([8.0])


def test_span_timer_ms_is_record_launch_record_wait_elapsed_and_nothing_else():
    hip = FakeHip(elapsed=[1.25])
    timer = rh.SpanTimer(hip)
    e0, e1 = timer.e0.value, timer.e1.value
    assert e0 and e1 and e0 != e1 and hip.calls == []
    assert timer.ms(lambda: hip.calls.append(("launch",))) == 1.25
    assert hip.calls == [("record", e0), ("launch",), ("record", e1), ("event_sync", e1), ("elapsed", e0, e1)]


def test_span_timer_ms_per_launch_warms_up_synchronises_and_spans_the_repetitions():
    hip = FakeHip(elapsed=[6.0])
    timer = rh.SpanTimer(hip)
    e0, e1 = timer.e0.value, timer.e1.value
    assert timer.ms_per_launch(lambda: hip.calls.append(("launch",)), reps=3) == 2.0
    assert hip.calls == ([("launch",)] * 2 + [("sync",), ("record", e0)] + [("launch",)] * 3
                         + [("record", e1), ("event_sync", e1), ("elapsed", e0, e1)])


@pytest.mark.parametrize("with_before", [True, False], ids=["before_round", "none"])
def test_host_clock_rounds_keeps_before_round_outside_the_two_synchronisations(monkeypatch, with_before):
    hip = FakeHip()
    ticks = iter([0.0, 0.004, 1.0, 1.010, 2.0, 2.002])

    def clock():
        hip.calls.append(("clock",))
        return next(ticks)

    monkeypatch.setattr(rh.time, "perf_counter", clock)
    before = (lambda: hip.calls.append(("before",))) if with_before else None
    ms = rh.host_clock_rounds(hip, lambda: hip.calls.append(("launch",)), steps=2, rounds=3, before_round=before)
    one = [("sync",), ("clock",), ("launch",), ("launch",), ("sync",), ("clock",)]
    assert hip.calls == ((([("before",)] if with_before else []) + one) * 3)
    assert len(ms) == 3 and ms == pytest.approx([2.0, 5.0, 1.0])           # ms per step of every round


def test_what_rounds_warms_up_checks_measures_and_checks_again():
    hip, log = FakeHip(), []

    class O:
        warmup, steps, rounds = 3, 2, 2

    ms = rh.what_rounds(hip, lambda: log.append("step"), O, lambda: log.append("check"),
                        before_round=lambda: log.append("before"))
    assert log == ["step"] * 3 + ["check"] + ["before", "step", "step"] * 2 + ["check"]
    assert len(ms) == 2


def test_kseg_workspace_clears_256_bytes_and_is_freed_once_when_the_body_raises():
    hip, lib = FakeHip(), FakeLib(1 << 20)
    with pytest.raises(RuntimeError, match="in the body"):
        with rh.kseg_workspace(lib, hip, ca.FP64, ca.VARIANT_KSEG, 8192, 64, 137) as ws:
            q = ws.value
            raise RuntimeError("in the body")
    assert lib.asked == [(ca.FP64, ca.VARIANT_KSEG, 8192, 64, 137)]
    assert hip.calls == [("malloc", q, 1 << 20), ("memset", q, 0, 256), ("free", q)]


def test_kseg_workspace_is_freed_once_on_the_way_out_and_allocates_nothing_for_no_bytes():
    hip = FakeHip()
    with rh.kseg_workspace(FakeLib(4096), hip, ca.FP32, ca.VARIANT_KSEG, 100, 32, 137) as ws:
        q = ws.value
        assert [c[0] for c in hip.calls] == ["malloc", "memset"]
    assert hip.calls[2:] == [("free", q)]
    hip = FakeHip()
    with rh.kseg_workspace(FakeLib(0), hip, ca.FP64, ca.VARIANT_KCACHE, 100, 32, 137) as ws:
        assert ws.value is None                                             # NULL: what KCACHE takes
    assert hip.calls == []
    with pytest.raises(AssertionError):
        with rh.kseg_workspace(FakeLib(-1), hip, 99, ca.VARIANT_KSEG, 100, 32, 137):
            pass
    assert hip.calls == []


def test_device_buffer_fills_as_asked_and_is_freed_once_when_the_body_raises():
    hip = FakeHip()
    with pytest.raises(KeyError):
        with rh.device_buffer(hip, 1000) as q:
            raise KeyError("body")
    assert hip.calls == [("malloc", q.value, 1000), ("free", q.value)]
    hip = FakeHip()
    with rh.device_buffer(hip, 1000, fill=0) as q:
        pass
    assert hip.calls == [("malloc", q.value, 1000), ("memset", q.value, 0, 1000), ("free", q.value)]
    hip, a = FakeHip(), np.arange(5.0)
    with rh.device_buffer(hip, a.nbytes, fill=a) as q:
        pass
    assert hip.calls == [("malloc", q.value, 40), ("memcpy", q.value, a.ctypes.data, 40, 1), ("free", q.value)]


def test_launch_check_calls_cloudsc_gpu_check_on_the_workspace_and_raises_on_its_code(monkeypatch):
    seen = []

    class Lib:
        def cloudsc_gpu_check(self, *args):
            seen.append(args)
            return 7

    monkeypatch.setattr(rh.ca, "check", lambda rc: seen.append(("check", rc)))
    rh.launch_check(Lib(), ca.VARIANT_KSEG, "ws")()
    assert seen == [(0, None, ca.VARIANT_KSEG, "ws"), ("check", 7)]


def test_summary_rounds_to_four_places_and_takes_the_median_of_an_even_count():
    assert rh.summary([1.00004, 3.00006, 2.0, 4.123456]) == {"median_ms": 2.5, "min_ms": 1.0, "max_ms": 4.1235}
    assert rh.summary([0.12344, 0.12348]) == {"median_ms": 0.1235, "min_ms": 0.1234, "max_ms": 0.1235}
    assert all(type(v) is float for v in rh.summary(np.array([1.0, 2.0], dtype=np.float32)).values())


def test_what_record_and_lib_label(monkeypatch):
    class O:
        what, precision, ngptot, nproma, steps, rounds, outputs = "a", "fp64", 8192, 64, 2, 2, "all"

    keys = ("what", "precision", "outputs", "ngptot", "nproma", "steps", "rounds", "finite")
    monkeypatch.delenv("CLOUDSC_AMD_LIB", raising=False)
    assert rh.lib_label() == "this build"
    rec = rh.what_record(O, [1.00004, 3.00006, 2.0, 4.123456], keys, finite=True)
    assert rec == {"what": "a", "precision": "fp64", "outputs": "all", "ngptot": 8192, "nproma": 64, "steps": 2,
                   "rounds": 2, "finite": True, "lib": "this build", "ms_per_step": [1.0, 3.0001, 2.0, 4.1235],
                   "median_ms": 2.5}
    assert list(rec) == list(keys) + ["lib", "ms_per_step", "median_ms"]   # the order the profiles' lines have
    monkeypatch.setenv("CLOUDSC_AMD_LIB", "/somewhere/libcloudsc_amd.so")
    assert rh.lib_label() == "CLOUDSC_AMD_LIB" and rh.what_record(O, [1.0], keys[:2])["lib"] == "CLOUDSC_AMD_LIB"
    monkeypatch.setenv("CLOUDSC_AMD_LIB", "")
    assert rh.lib_label() == "this build"


def test_records_print_each_line_as_made_and_write_the_same_lines(tmp_path, capsys, monkeypatch):
    asked = []
    monkeypatch.setattr(rh.ca, "hbm_copy_gbps", lambda *a: asked.append(a) or 5123.456)
    records = rh.Records()
    records.emit({"measure": "expectation", "b_over_a": "about 1"})
    assert capsys.readouterr().out == '{"measure": "expectation", "b_over_a": "about 1"}\n'       # at once
    assert records.stream_copy() == 5123.456 and asked == [(0, 4 << 30, 10)]
    records.emit({"measure": "x", "ms": 1.5, "ok": True, "none": None})
    printed = capsys.readouterr().out.splitlines()
    assert json.loads(printed[0]) == {"measure": "stream_copy", "gbps": 5123.5}
    out = tmp_path / "not" / "there" / "rate.jsonl"
    records.write(str(out))
    lines = out.read_text().splitlines()
    assert lines[1:] == printed and len(lines) == 3 and [json.loads(x)["measure"] for x in lines] == [
        "expectation", "stream_copy", "x"]
    records.write(str(out))                                                 # --out overwrites
    assert out.read_text().splitlines() == lines
    records.write(str(out), append=True)                                    # fields_layout_rate.py --ab appends
    assert out.read_text().splitlines() == lines + lines
    records.write(None)                                                     # no --out: nothing
    assert rh.Records().stream_copy(expected=[0.8, 0.93]) == 5123.456
    assert json.loads(capsys.readouterr().out) == {"measure": "stream_copy", "gbps": 5123.5, "expected": [0.8, 0.93]}


def _profile_record(path, measure, precision):
    with open(os.path.join(REPO, "profiles", path)) as fh:
        recs = [json.loads(x) for x in fh]
    return next(r for r in recs if r.get("measure") == measure and r.get("precision") == precision)


def test_column_bytes_are_the_committed_profiles():
    rec = _profile_record("outputs/outputs_rate.jsonl", "kseg_outputs", "fp64")
    assert rec["klev"] == 137
    assert rh.column_bytes(137, 8, ca.OUTPUTS_ALL) == rec["column_bytes_all"] == 56036
    assert rh.column_bytes(137, 8, ca.OUTPUTS_PROGNOSTIC) == rec["column_bytes_prognostic"] == 44996
    surf = _profile_record("outputs_surface/outputs_surface_rate.jsonl", "kseg_outputs_surface", "fp32")
    assert rh.column_bytes(137, 4, ca.OUTPUTS_PROGNOSTIC) == surf["column_bytes_prognostic"]
    assert rh.column_bytes(137, 4, ca.OUTPUTS_SURFACE) == surf["column_bytes_surface"]


def test_the_option_tables():
    assert rh.PRECISIONS == [("fp64", ca.FP64), ("mixed", ca.MIXED), ("fp32", ca.FP32)]
    assert rh.PRECISION == dict(rh.PRECISIONS)
    assert rh.VARIANT == {"kseg": ca.VARIANT_KSEG, "kcache": ca.VARIANT_KCACHE}
    assert rh.OUTPUTS["all"] == ca.OUTPUTS_ALL and rh.OUTPUTS["surface"] == ca.OUTPUTS_SURFACE


HARNESS_PIECES = re.compile(r"hipEventCreate|\.argtypes|def summary|def emit|class SpanTimer|class Timer|"
                            r"hipDeviceSynchronize|hipMalloc\(|hipFree\(|cloudsc_gpu_scratch_bytes|hbm_copy_gbps|"
                            r"def column_bytes|os\.environ")


@pytest.mark.parametrize("tool", TOOLS)
def test_a_rate_tool_keeps_no_copy_of_a_harness_piece(tool):
    with open(os.path.join(REPO, "tools", tool + ".py")) as fh:
        text = fh.read()
    assert HARNESS_PIECES.findall(text) == []
    assert ("perf_counter" in text) == (tool == "fields_compare_rate")     # its spans around downloads and NumPy
    assert "rate_harness" in text


@pytest.mark.parametrize("tool", TOOLS)
def test_a_rate_tool_prints_its_help_without_a_gpu(tool):
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", tool + ".py"), "--help"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: %s.py" % tool) and "--ngptot" in r.stdout
