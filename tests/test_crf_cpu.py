"""metric.dense_crf without a GPU: the float64 oracle (tests/crf_oracle.py) stated twice and pinned to itself, known answers
that follow from the definition, the C-ABI declarations, the register budget of csrc/crf.hip, and the two numbers the GPU
tests lean on -- the f32 error of the formula itself (eps32, committed as tests/golden/crf_eps32.json) and the share of
near-tie pixels that the label comparison may leave out."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests import crf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))

EXPORTS = ("sgg_dense_crf_workspace_bytes", "sgg_dense_crf")


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_matrix_and_loop_statements_agree(name):
    img, probs = O.case_inputs(name)
    assert np.abs(O.dense_crf_loop(img, probs) - O.case_q64(name)).max() <= 1e-12


def _softmax_neg_unary(probs):
    U = O.unary_from_softmax(probs).astype(np.float64)
    e = np.exp(-U - (-U).max(axis=0))
    return (e / e.sum(axis=0)).reshape(probs.shape)


@pytest.mark.parametrize("crf", [O.dense_crf_matrix, O.dense_crf_loop])
def test_known_answers(crf):
    """Exact consequences of the definition; the bounds are float64 rounding of a C-term softmax (C <= 34: 1e-14), not
    measurements."""
    img, probs = O.case_inputs("smooth3")
    q0 = _softmax_neg_unary(probs)
    # no pairwise weight: every step recomputes softmax(-U + 0)
    assert np.abs(crf(img, probs, pos_w=0, bi_w=0) - q0).max() <= 1e-14
    # no steps: Q_0
    assert np.abs(crf(img, probs, max_iter=0) - q0).max() <= 1e-14
    # the marginals of a pixel sum to one
    assert np.abs(crf(img, probs).sum(axis=0) - 1.0).max() <= 1e-14
    # a constant image with a constant unary: every class receives the same message, Q stays uniform
    flat = np.full((6, 9, 3), 77, dtype=np.uint8)
    q = crf(flat, np.full((4, 6, 9), 0.25, dtype=np.float32))
    assert np.abs(q - 0.25).max() <= 1e-14
    # one-hot probabilities: the unary holds exactly 0 and -log(1e-5)
    _, onehot = O.case_inputs("tiny34")
    U = O.unary_from_softmax(onehot)
    assert U.dtype == np.float32 and U.shape == (34, 240)
    assert set(np.unique(U).tolist()) == {0.0, float(np.float32(-np.log(1e-5)))}
    assert np.array_equal(U == 0, onehot.reshape(34, -1) == 1)


def test_exports_declared_in_header_abi_and_library():
    src = open(os.path.join(ROOT, "include", "sggan.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert os.path.exists(A.LIB_PATH), "run `python __graft_entry__.py build` first"
    L = ctypes.CDLL(A.LIB_PATH)
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in A.SIGNATURES, name
        assert hasattr(L, name), f"{name} not exported by libsggan.so"
    assert len(A.SIGNATURES["sgg_dense_crf"][1]) == 16 and len(A.SIGNATURES["sgg_dense_crf_workspace_bytes"][1]) == 3
    decl = re.search(r"int\s+sgg_dense_crf\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert len(decl.split(",")) == 16
    for word in ("max_iter", "pos_w", "pos_xy_std", "bi_w", "bi_xy_std", "bi_rgb_std", "ws_bytes", "stream"):      # run-time arguments
        assert re.search(r"\b" + word + r"\b", decl), word


def test_host_side_argument_checks_without_gpu():
    """Everything sgg_dense_crf refuses before it launches: answered from the host, no device needed."""
    L = A.lib()
    need = L.sgg_dense_crf_workspace_bytes(33, 47, 34)
    assert need > 0 and need % 256 == 0
    assert L.sgg_dense_crf_workspace_bytes(33, 47, 3) < need                         # sized by the padded channel count
    assert L.sgg_dense_crf_workspace_bytes(33, 47, 34) == L.sgg_dense_crf_workspace_bytes(33, 47, 40)
    assert L.sgg_dense_crf_workspace_bytes(0, 47, 3) == 0 and L.sgg_dense_crf_workspace_bytes(33, 47, 41) == 0
    call = lambda img, p, u, out, ws, nbytes, it=10, sxy=1.0: L.sgg_dense_crf(img, p, u, 33, 47, 34, it, 3.0, sxy, 4.0, 67.0, 3.0, out, ws,
                                                                             nbytes, None)
    x = ctypes.c_void_p(4096)                                                        # never dereferenced by a refused call
    assert call(None, x, None, x, x, need) == A.EINVAL
    assert call(x, x, x, x, x, need) == A.EINVAL and call(x, None, None, x, x, need) == A.EINVAL     # exactly one of probs / unary
    assert call(x, x, None, x, x, need, it=-1) == A.EINVAL and call(x, x, None, x, x, need, sxy=0.0) == A.EINVAL
    assert call(x, x, None, x, x, need - 1) == A.EWORKSPACE and call(x, x, None, x, None, need) == A.EWORKSPACE
    assert L.sgg_dense_crf(x, x, None, 33, 47, 41, 10, 3.0, 1.0, 4.0, 67.0, 3.0, x, x, need, None) == A.EUNSUPPORTED


def test_crf_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    assert "crf.hip" in B.SOURCES
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "crf.hip"), "-o", str(tmp_path / "crf.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        for key, pat in (("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    kernels = {k: v for k, v in usage.items() if "crf_" in k}
    # prep, the normaliser pass, and per padded channel count 8..40 one pair kernel and one softmax kernel
    assert len(kernels) == 12 and sum("crf_pair_kernel" in k for k in kernels) == 6, sorted(kernels)
    for k, v in kernels.items():
        assert v == {"vspill": 0, "sspill": 0, "scratch": 0}, (k, v)


def test_eps32_fixture_is_the_measured_f32_error_of_the_formula():
    """eps32 = max |Q_float32 - Q_float64| of the matrix statement over the shared inputs.  The committed number is what the
    GPU bound multiplies; re-measured here it may move with the summation order of the installed BLAS (a different split of
    the N-term dot products), which changes individual roundings but not their scale -- so the check is a factor of 4 either
    way, far inside the margin factor of 8 the GPU test grants on top of it."""
    with open(O.GOLDEN) as f:
        g = json.load(f)
    assert set(g["per_case"]) == set(O.CASES) and g["eps32"] == max(g["per_case"].values())
    now = O.measured_eps32()
    print("eps32 committed", g["eps32"], "measured", now)
    assert g["eps32"] / 4 <= max(now.values()) <= g["eps32"] * 4
    assert 2.0 ** -24 < g["eps32"] < 1e-4          # no better than one rounding of a value near 1, no worse than 10 steps can make it


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_near_tie_share_of_the_oracle_is_under_the_cap(name):
    """Pixels whose float64 top-two margin is under 16 eps32 are left out of the GPU label comparison; they must be at most
    1 % of an input (an input over the cap gets another seed, the cap stays)."""
    share = float((O.top2_margin(O.case_q64(name)) < 16 * O.golden_eps32()).mean())
    print(name, "near-tie share", share)
    assert share <= 0.01
