#!/usr/bin/env python3
"""Record tests/golden/unit_trace.json: what the layer units of module.py launch and compute, on one MI355X.

    python tests/golden/make_unit_trace.py [--out FILE] [--force]

The fixture pins the tree of the commit it was recorded on -- the parent of the commit that gave the four unit classes one
forward and one backward -- and tests/test_gpu_unit_trace.py holds every later tree to it.  It is therefore made ONCE and
committed; re-recording it with the tree under test would make that test compare the tree with itself, so an existing file is
only replaced with --force (a deliberate change of a launch sequence, recorded on the commit before it).  Cases, inputs, the
proxy and the digests are the functions of the test module; nothing here draws a random number.

Every case runs twice on fresh models.  The traces must be equal; a case whose digests differ between the two runs keeps its
trace and is stored without digests (and is named on the way out).  Distinct entries and distinct per-step sequences are
stored once: "entries" is the table, "sequences" the per-step index lists into it, a case's "steps" index into those."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import torch
    import sggan_amd
    from tests import test_gpu_unit_trace as T
    assert torch.cuda.is_available(), "the recorder needs the GPU"
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else T.FIXTURE
    if os.path.exists(dst) and "--force" not in sys.argv:
        sys.exit(f"{dst} exists: it is recorded once (see the docstring)")
    entries, sequences, cases = {}, {}, {}
    for case in T.CASES:
        t0 = time.time()
        steps, digests = T.run_case(sggan_amd, case)
        again, digests2 = T.run_case(sggan_amd, case)
        assert T.first_difference(case, again, steps) is None, T.first_difference(case, again, steps)
        if digests != digests2:
            print(f"{case}: digests differ between two runs ({[k for k in digests if digests[k] != digests2[k]]}): stored without")
            digests = None
        ids = []
        for step in steps:
            seq = tuple(entries.setdefault(json.dumps(e, separators=(",", ":")), len(entries)) for e in step)
            ids.append(sequences.setdefault(seq, len(sequences)))
        cases[case] = {"steps": ids, "digests": digests}
        pair2 = sorted({e[4] for step in steps for e in step if e[0] == "sgg_conv2d_bwd_weight_pair2"})
        print(f"{case}: {[len(s) for s in steps]} calls, steps {ids}, wgrad_pair2 statuses {pair2}, {(time.time() - t0) / 2:.2f} s per run", flush=True)
    head = {"rocm": torch.version.hip, "device": torch.cuda.get_device_name(0), "library": sggan_amd.lib().sgg_version(),
            "entry": "[symbol, conv descriptor fields or null, scalar arguments, NULL flag per pointer argument, status]",
            "digest": "sha256 of the tensor's bytes after step 2"}
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:                              # one entry, sequence and case per line
        line = lambda o: json.dumps(o, separators=(",", ":"))
        f.write("{\n" + "".join(f"{json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()))
        f.write('"entries": [\n' + ",\n".join(entries) + "\n],\n")
        f.write('"sequences": [\n' + ",\n".join(line(list(s)) for s in sequences) + "\n],\n")
        f.write('"cases": {\n' + ",\n".join(f"{json.dumps(k)}: {line(v)}" for k, v in cases.items()) + "\n}\n}\n")
    with open(dst) as f:
        back = json.load(f)
    for case in T.CASES:                                   # what was written reads back as what was run
        assert len(T.recorded_steps(back, case)) == T.STEPS
    print(f"wrote {dst}: {len(cases)} cases, {len(entries)} distinct entries, {len(sequences)} distinct step sequences, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
