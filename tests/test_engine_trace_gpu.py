"""The engine launches what tests/golden/engine_backward_trace.json says: every call into the library of two forward /
backward passes of the small graphs of tests/engine_trace.py, under every setting listed there, call by call with its
arguments.  The fixture was written from the engine before its backward routing moved into dspnet_amd/backward_route.py
(tests/golden/make_engine_backward_trace_golden.py); it is regenerated only by a change that means to alter what is
launched.  The default setting of each toy is compared line by line, every other case by the sha256 of its lines, with the
per-function call counts printed first where they differ."""
import json
import os

import pytest

import engine_trace as T

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_backward_trace.json")) as _f:
    GOLDEN = json.load(_f)
ROWS = {(r["graph"], r["setting"]): r for r in GOLDEN["cases"]}


def test_fixture_covers_the_cases_and_the_recorded_functions():
    assert sorted(ROWS) == sorted(T.cases())
    assert GOLDEN["recorded"] == T.recorded_functions(), "functional.py gained or lost an entry the recorder wraps: regenerate"


@pytest.mark.parametrize("graph,setting", T.cases(), ids=lambda v: v)
def test_launch_sequence_is_the_recorded_one(gpu_device, graph, setting):
    row = ROWS[(graph, setting)]
    lines = T.trace(graph, setting, gpu_device, pointers=GOLDEN["pointers"])
    assert T.call_counts(lines) == row["counts"]
    for i, (got, want) in enumerate(zip(lines, row.get("lines", ()))):
        assert got == want, "call %d" % i
    assert len(lines) == row["calls"] + lines.count("-- pass") and T.digest(lines) == row["sha256"]
    assert T.EXPECT.get((graph, setting), set()) <= T.routes_seen(lines)
