#!/usr/bin/env python3
"""Record tests/golden/adam_bits.json: what the Adam entry points compute, as SHA-256 digests, on one MI355X.

    python tests/golden/make_adam_bits.py [--out FILE] [--force]

The fixture pins the library of the commit it was recorded on -- the parent of the commit that moved the family to
csrc/adam.hip -- and tests/test_gpu_adam_bits.py holds every later library to it.  It is therefore made ONCE and committed;
re-recording it with the library under test would make that test compare the library with itself, so an existing file is
only replaced with --force (a deliberate change of the arithmetic, recorded on the commit before it).  Paths, sizes, inputs
and the digest are the functions of the test module; nothing here draws a random number."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import torch
    import sggan_amd
    import sggan_amd.kernels as K
    from tests import test_gpu_adam_bits as T
    assert torch.cuda.is_available(), "the recorder needs the GPU"
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else T.FIXTURE
    if os.path.exists(dst) and "--force" not in sys.argv:
        sys.exit(f"{dst} exists: it is recorded once (see the docstring)")
    digests = {path: {str(n): T.run_path(K, path, n) for n in T.SIZES} for path in T.PATHS}
    again = {path: {str(n): T.run_path(K, path, n) for n in T.SIZES} for path in T.PATHS}
    assert digests == again, "two runs gave different bits"
    out = {"rocm": torch.version.hip, "device": torch.cuda.get_device_name(0), "library": sggan_amd.lib().sgg_version(),
           "digest": "sha256 of the tensor's bytes after steps 1, 2, 3", "digests": digests}
    with open(dst, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {dst}: {len(T.PATHS)} paths x {len(T.SIZES)} sizes")


if __name__ == "__main__":
    main()
