"""Writes engine_backward_trace.json: what the engine launches, call by call, in two forward / backward passes of the small
graphs of tests/engine_trace.py under every setting listed there (tests/test_engine_trace_gpu.py replays it case by case).
SELF-GENERATED on the GPU, from the engine whose routing is to be pinned, with the DSPN_* knobs unset; regenerate it only in a
change that means to alter what is launched.

Every case is traced twice and the two traces must agree: first with the tensors' pointer numbers (@k); if those turn out not
to repeat, without them, which the file then says ("pointers": false).  The full line list is stored for the default setting of
each toy; every other case stores the sha256 of its joined lines and its per-function call counts.  The maker refuses a fixture
in which a route a case is there for does not occur (engine_trace.EXPECT / FORBID).

    python tests/golden/make_engine_backward_trace_golden.py [--dump DIR]      # DIR: every full trace, one file per case"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "engine_backward_trace.json"))
    args = ap.parse_args()
    assert not [k for k in os.environ if k.startswith("DSPN_") and k != "DSPN_LIB"], "unset the DSPN_* knobs"
    import torch
    import engine_trace as T
    dev = torch.device("cuda", 0)
    cases = T.cases()
    pointers = True
    traces = {}
    for graph, setting in cases:
        a = T.trace(graph, setting, dev, pointers)
        if pointers and a != T.trace(graph, setting, dev, True):
            print("pointer numbers do not repeat (%s, %s): recording without them" % (graph, setting))
            pointers = False
            break
        traces[(graph, setting)] = a
    if not pointers:
        traces = {}
        for graph, setting in cases:
            a = T.trace(graph, setting, dev, False)
            assert a == T.trace(graph, setting, dev, False), ("the trace does not repeat", graph, setting)
            traces[(graph, setting)] = a
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for (graph, setting), lines in traces.items():
            with open(os.path.join(args.dump, "%s.%s.txt" % (graph, setting)), "w") as f:
                f.write("\n".join(lines) + "\n")
    missing, everywhere = [], set()
    for key, lines in traces.items():
        seen = T.routes_seen(lines)
        everywhere |= seen
        missing += [(key, "missing", r) for r in sorted(T.EXPECT.get(key, set()) - seen)]
        missing += [(key, "unexpected", r) for r in sorted(T.FORBID.get(key, set()) & seen)]
    for r in ("sums-only", "addend", "compact", "parked", "pooled", "fallback", "second stream", "recomputed apply", "planes",
              "parameters only", "input-sum gradient", "branch stream"):
        if r not in everywhere:
            missing.append(("any case", "missing", r))
    rows = []
    for (graph, setting), lines in traces.items():
        row = {"graph": graph, "setting": setting, "calls": len([ln for ln in lines if not ln.startswith("--")]),
               "sha256": T.digest(lines), "counts": T.call_counts(lines)}
        if setting == "defaults" and graph in T.TOYS:
            row["lines"] = lines
        rows.append(row)
    with open(args.out, "w") as f:
        f.write("{\"pointers\": %s,\n \"recorded\": %s,\n \"cases\": [\n" % (json.dumps(pointers), json.dumps(T.recorded_functions())))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print(len(rows), "cases,", sum(r["calls"] for r in rows), "calls, pointers", pointers, "->", os.path.getsize(args.out), "bytes")
    assert not missing, ("written, but not fit to commit: a route a case is there for does not occur", missing)


if __name__ == "__main__":
    main()
