"""not-gpu: the launch plans of the glue kernels.  For every shape of the sweep (tests/glue_cases.py) avsep_glue_plan — the
function the launchers themselves take their form and grid from — answers the form and grid written in the table, the loops
a row claims are really taken twice, no tensor reaches the size limit, and the seeds of the pooling rows give no window whose
fp32 winner differs from the float64 one."""
import ctypes

import pytest
import torch

import glue_cases as S
import glueref as G


def _lib():
    import avsep_amd
    return avsep_amd.lib.load()


@pytest.mark.parametrize("row", S.SWEEP, ids=lambda r: f"{r[0]}-{S.case_id(r)}")
def test_plan_of_every_sweep_shape(row):
    kernel, op, dims, aux, form, grid, twice, _ = row
    got = S.plan(_lib(), op, dims, aux)
    assert got == (form, grid), (row, got)
    lp = S.loops(op, dims, aux, form, grid)
    for name in twice:
        assert lp[name] > 1 and (name == "terms" or lp[name] != int(lp[name])), (row, lp)     # twice, the last pass ragged
    assert S.largest_tensor(op, dims, aux) < S.SIZE_LIMIT, row


def test_every_form_of_every_launcher_is_in_the_sweep():
    forms = {}
    for r in S.SWEEP:
        forms.setdefault(r[1], set()).add(r[4])
    assert forms["bn_bwd_apply"] == forms["affine_act"] == {"vec4", "scalar"}
    assert forms["affine_act_bwd"] == {"v4", "v1"}
    assert forms["maxpool_fwd"] == {"fwd4", "generic"}
    assert forms["maxpool_bn_relu_bwd_apply"] == {"apply4", "pair", "apply1"}
    for op in ("b16_affine_act", "b16_affine_act_bwd", "b16_bn_bwd_apply", "b16_maxpool_fwd", "b16_maxpool_bwd_stats",
               "b16_maxpool_bwd_apply"):
        assert forms[op] == {"slot", "slot,images"}, op
    taken = {(r[1], n) for r in S.SWEEP for n in r[6]}
    for want in [("channel_stats", "terms"), ("bn_bwd_apply", "x"), ("affine_act", "x"), ("affine_act_bwd", "terms"),
                 ("maxpool_fwd", "x"), ("maxpool_bwd", "x"), ("maxpool_bn_relu_bwd_stats", "terms"),
                 ("maxpool_bn_relu_bwd_apply", "x"), ("temporal_mean_fwd", "x"), ("temporal_mean_bwd", "x"), ("sgd", "x"),
                 ("space_to_depth2", "x"), ("space_to_depth2", "planes"), ("f32_to_b16", "x"), ("b16_to_f32", "x"),
                 ("bn_bwd_apply_to_b16", "x"), ("b16_affine_act", "slots"), ("b16_affine_act", "images")]:
        assert want in taken, want
    # the flush of channel_stats: 64 terms on a thread
    assert max(S.loops(r[1], r[2], r[3], r[4], r[5])["terms"] for r in S.cases("channel_stats")) == 64


def test_plan_query_refuses_what_the_launchers_refuse():
    L = _lib()
    form, grid = ctypes.create_string_buffer(64), (ctypes.c_int32 * 3)()
    bad = [("no_such_op", 1, 16, 4, 4, 0), ("affine_act", 0, 3, 4, 4, 0), ("affine_act", 1, 65536, 4, 4, 0),
           ("b16_affine_act", 1, 24, 4, 4, 0), ("space_to_depth2", 1, 3, 5, 4, 16), ("space_to_depth2", 1, 3, 4, 4, 8),
           ("b16_space_to_depth2", 1, 5, 4, 4, 0), ("affine_act_bwd", 70000, 1, 256, 256, 0)]
    for op, *a in bad:
        assert L.avsep_glue_plan(op.encode(), *a, form, 64, grid) == -1, op
    assert L.avsep_glue_plan(b"affine_act", 1, 1, 4, 4, 0, form, 8, grid) == -1          # buffer too small
    assert L.avsep_glue_plan(b"affine_act", 1, 1, 4, 4, 0, None, 64, grid) == -1


@pytest.mark.parametrize("row", [r for r in S.SWEEP if r[1] in ("maxpool_fwd", "b16_maxpool_fwd") and r[2][1] < 65536],
                         ids=lambda r: f"{r[0]}-{S.case_id(r)}")
def test_pool_seeds_have_no_window_the_reference_itself_cannot_decide(row):
    import glue_inputs as I
    for act in (0, 1, 2):
        x, sc, sh = I.pool_operands(row, act)
        assert torch.equal(G.maxpool(x, sc, sh, act, exact=True)["tap"], G.maxpool(x, sc, sh, act, exact=False)["tap"]), (row, act)
