"""tests/golden/unit_trace.json pins nothing where it never goes: every configuration of tests/test_gpu_unit_trace.py must be in
it with both steps, and across them every launch the layer units of module.py can make must occur at least once with status 0
(sgg_conv2d_bwd_weight_pair2 with whatever it answered -- its fallback launches are pinned behind it).  Reads the JSON only."""
import json

from tests.test_gpu_unit_trace import CASES, FIXTURE, STEPS, recorded_steps

NORM = ["sgg_instnorm_" + d + form for d, forms in (("fwd", ("", "_partial", "_skip", "_pair", "_partial_pair", "_skip_pair")),
                                                    ("bwd", ("", "_partial", "_skip", "_pair", "_skip_pair", "_mixed"))) for form in forms]
SYMBOLS = ["sgg_conv2d_fwd", "sgg_conv2d_fwd_stats", "sgg_conv2d_fwd_stats_pair", "sgg_conv2d_fwd_group2",
           "sgg_deconv2d_fwd", "sgg_deconv2d_fwd_stats", "sgg_deconv2d_fwd_group2",
           "sgg_conv2d_bwd_data", "sgg_conv2d_bwd_data_stats", "sgg_conv2d_bwd_data_mixed", "sgg_conv2d_bwd_data_pair", "sgg_conv2d_bwd_data_group2",
           "sgg_deconv2d_bwd_data", "sgg_deconv2d_bwd_data_group2",
           "sgg_conv2d_bwd_weight", "sgg_conv2d_bwd_weight_pair", "sgg_conv2d_bwd_weight_group2", "sgg_deconv2d_bwd_weight", "sgg_deconv2d_bwd_weight_group2",
           "sgg_bias_grad", "sgg_bias_grad_group2", "sgg_instnorm_finalize", "sgg_dropout"] + NORM


def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_configuration_is_recorded_with_both_steps():
    rec = _recorded()
    assert rec["rocm"] and set(rec["cases"]) == set(CASES)
    for case in CASES:
        steps = recorded_steps(rec, case)
        assert len(steps) == STEPS and all(steps), case
        digests = rec["cases"][case]["digests"]
        assert digests is None or all(len(d) == 64 for d in digests.values()), case
        assert all(len(e) == 5 and (e[1] is None or len(e[1]) == 14) for step in steps for e in step), case


def test_every_launch_of_the_units_occurs_with_status_ok():
    rec = _recorded()
    used = [rec["entries"][i] for case in CASES for s in rec["cases"][case]["steps"] for i in rec["sequences"][s]]
    ok = {e[0] for e in used if e[4] == 0}
    assert not [s for s in SYMBOLS if s not in ok]
    assert any(e[0] == "sgg_conv2d_bwd_weight_pair2" for e in used)
    # sgg_deconv2d_fwd_stats of one network (nsplit 0, no second weight set) and of the stacked pair: its scalars are (nsplit, ws_bytes),
    # its pointers (x, w, bias, w2, bias2, y, partial, ws, stream)
    forms = {(e[2][0] > 0, e[3][3] == "0") for e in used if e[0] == "sgg_deconv2d_fwd_stats" and e[4] == 0}
    assert forms == {(False, False), (True, True)}
