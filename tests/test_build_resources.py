"""Build-time guard for the register-bound GEMM kernels (CPU only: hipcc cross-compiles without a GPU).

The 8-wave kernels run at 2 waves/SIMD, i.e. a 256-VGPR budget they use almost completely; a source change that tips
one of them into scratch spills costs 2-5x at run time without failing any numerical test (seen while developing the
all-taps weight-gradient kernel).  This test recompiles the conv sources of build.SOURCES (conv.hip, conv_halo3.hip, conv_wgrad.hip)
with -Rpass-analysis=kernel-resource-usage and requires zero VGPR spills and the expected occupancy for the production configurations, and one owner file per kernel.
"""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))

# mangled-name fragments of the kernels that must not spill (production tile configurations)
MUST_NOT_SPILL = [
    # conv3x3_halo_gemm_kernel<MODE, FOLD, STATS, PAIR, SRC>: a fragment up to PAIR covers every SRC of it the library dispatches
    "conv3x3_halo_gemm_kernelILi0ELb0ELi0ELb0E",               # 3x3 forward, halo resident
    "conv3x3_halo_gemm_kernelILi0ELb0ELi1ELb0E",               # ... with the norm-statistics epilogue
    "conv3x3_halo_gemm_kernelILi0ELb0ELi0ELb1E",               # ... on a stacked pair of networks
    "conv3x3_halo_gemm_kernelILi0ELb0ELi1ELb1E",               # ... both (the roofline kernel of the cycle step)
    "conv3x3_halo_gemm_kernelILi1ELb0ELi0ELb0E",               # 3x3 data gradient, zero padding
    "conv3x3_halo_gemm_kernelILi1ELb1ELi0ELb0E",               # 3x3 data gradient, REFLECT fold
    "conv3x3_halo_gemm_kernelILi1ELb0ELi0ELb1E", "conv3x3_halo_gemm_kernelILi1ELb1ELi0ELb1E",   # ... paired
    # (<DGRAD, *, STATS=2>: the data gradient with the norm-backward sums in its epilogue -- opt-in (fuse_in_bwd), off by default, measured
    # "no gain" at the step's launch size in round 3 -- sat at 249-250 VGPRs then; the kernel body as round 4 restructured it (a tile loop
    # that runs once, the main loop as a lambda) spills 29 (FOLD: 38) VGPRs, 112 (124) bytes of scratch.  Without that structure both build
    # with 0 spills at 249 / 250 VGPRs, but that form changes the code of all 16 instantiations and waits for a timing against this one.
    # Numerically tested (test_conv_dgrad_norm_bwd_epilogue), not guarded here.)
    "conv3x3_wgrad_halo_kernel",                               # 3x3 weight gradient, all taps per block
    "conv3x3_wgrad_halo_s2_kernel",                            # the same for stride 2
    "deconv_s2_halo_kernel",                                   # stride-2 data gradient / Conv2DTranspose forward
    "conv_wgrad_glds_kernelIDF16bLb0E", "conv_wgrad_glds_kernelIDF16bLb1E",
    "conv_gemm_glds_kernelIDF16bLi0ELi256ELi256ELi2ELi8ELi128ELi2E",
    "conv_gemm_glds_kernelIDF16bLi1ELi256ELi256ELi2ELi8ELi128ELi2E",
    "conv_gemm_glds_kernelIDF16bLi0ELi256ELi128ELi4ELi8ELi128ELi3E",
]
# small-tile configurations: only spills are checked
NO_SPILL_ONLY = ["conv_gemm_glds_kernelIDF16bLi0ELi128ELi128ELi2ELi8ELi128ELi2E", "conv_gemm_glds_kernelIDF16bLi1ELi128ELi128ELi2ELi8ELi128ELi2E"]


def test_gemm_kernels_do_not_spill(tmp_path):
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    srcs = [s for s in B.SOURCES if s.startswith("conv")]
    assert "conv.hip" in srcs and len(srcs) > 1, srcs
    with ThreadPoolExecutor(max_workers=min(16, len(srcs))) as ex:
        runs = list(ex.map(lambda s: subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, s), "-o", str(tmp_path / (s + ".o")),
                                                     "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True), srcs))
    owner = {}
    for s, r in zip(srcs, runs):
        assert r.returncode == 0, f"{s}: {r.stderr[-2000:]}"
        for n in re.findall(r"Function Name: (\S+)", r.stderr):
            assert owner.setdefault(n, s) == s, f"device function {n} is built by {owner[n]} and by {s}"
    merged = "\n".join(r.stderr for r in runs)
    # remarks come in blocks: "Function Name: X", ..., "VGPRs Spill: N", ..., "Occupancy [waves/SIMD]: M"
    usage, name = {}, None
    for line in merged.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        for key, pat in (("spill", r"VGPRs Spill: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    assert usage, "no kernel-resource-usage remarks parsed"
    for frag in MUST_NOT_SPILL + NO_SPILL_ONLY:
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, f"kernel {frag} not found in the build"
        for k, v in hits.items():
            assert v.get("spill") == 0, f"{k} spills {v.get('spill')} VGPRs"
            if frag in MUST_NOT_SPILL:
                assert v.get("occ", 0) >= 2, f"{k} occupancy {v.get('occ')} waves/SIMD"
