"""Per-kernel resource usage of one csrc file: the file recompiled with the build's flags and
-Rpass-analysis=kernel-resource-usage (the method of tests/test_build_resources.py), the remarks parsed.  Shared by the CPU
tests that hold kernels to register, LDS and occupancy figures (test_lr_schedule_cpu.py, test_grad_guard_cpu.py,
test_ema_cpu.py)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PATS = (("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("vgpr", r" VGPRs: (\d+)"))


def kernel_resource_usage(source, tmp_path):
    """{mangled kernel name: {"vspill", "sspill", "scratch", "occ", "lds", "vgpr"}} of csrc/<source>; skips without hipcc."""
    sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, source), "-o", str(tmp_path / source.replace(".hip", ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        for key, pat in _PATS:
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    return usage


def the_kernel(usage, frag):
    """The one kernel whose name contains ``frag``."""
    hits = [v for k, v in usage.items() if frag in k]
    assert len(hits) == 1, f"kernel {frag}: {len(hits)} matches in the build"
    return hits[0]
