#!/usr/bin/env python3
"""Generates tests/golden/stitch_fingerprints.json: what the speculation scheduler (gr_lora_amd/csrc/lora_stitch.hpp) did on a fixed list of
CPU-simulated workloads (tests/host_sim/stitch_sim.cpp; the list is tests/test_stitch_sim.py's fingerprint_workloads).  Per workload: frames,
header positions, the stream of every frame, the sim's counters and its FNV-1a hash over every call the scheduler made.

Each workload's frames are checked against the serial oracle before anything is written.  Regenerate only when the scheduler is meant to
take other paths; a refactor must leave the file as it is.  Run from the repo root:  python tests/golden/make_stitch_fingerprints.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import test_stitch_sim as T  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    O.build()
    sim = T.load_sim()
    out = T.fingerprints(sim)
    for name, (iq, kw) in T.fingerprint_workloads().items():
        got = out[name]
        for i, (off, n) in enumerate(kw.get("streams") or [(0, iq.size)]):
            o = O.Oracle(sf=kw["sf"], cr=kw.get("ctor_cr", 4), demod=kw.get("demod", 2), reduced_rate=kw.get("reduced", False))
            o.run(iq[off:off + n])
            mine = [(f, p) for f, p, s in zip(got["frames"], got["header_pos"], got["stats"]["stream"]) if s == i]
            assert mine == [(f.hex(), p) for f, p in zip(o.frames(), o.frame_positions())], (name, i)
        print("%-44s %3d frames  %s" % (name, len(got["frames"]), got["stats"]))
    with open(os.path.join(HERE, "stitch_fingerprints.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
