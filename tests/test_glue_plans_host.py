"""not-gpu: the launch plans of the glue kernels.  For every shape of the sweep (tests/glue_cases.py) avsep_glue_plan — the
function the launchers themselves take their form and grid from — answers the form and grid written in the table, the loops
a row claims are really taken twice, no tensor reaches the size limit, and the seeds of the pooling rows give no window whose
fp32 winner differs from the float64 one."""
import ctypes

import pytest
import torch

import glue_cases as S
import glueref as G
from recipes import lib as _lib


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


# The decoder glue (ReLU + bilinear x2 of the skip concat and its transpose): (op, low-res (N, C, H, W) with C = C0 + C1, aux,
# form, grid), None for a shape the launcher refuses.  Every grid is the launcher's arithmetic done by hand, in the comment.
# fp32 (aux = 1: a source is an [N, C] broadcast vector), pair forms need a power-of-two 4 <= W <= 128 and H >= 2:
#   pair     (ceil((H + 1) * W/2 / 256), gy = min(planes, 32768), ceil(planes / gy)), planes = N * C
#   fwd4     W >= 8: (ceil(W/2 / 2^l), ceil(2H / (256 >> l)), planes), 2^l = the power of two >= W/2 within 4 .. 64
#   generic  (ceil(2W / 2^l), ceil(2H / (256 >> l)), planes), 2^l = the power of two >= 2W within 4 .. 256
#   sweep    pair shape, H >= 8, chunks = ceil(H / 8), tp = chunks * W/2 threads per plane: "sweep,planes" when tp <= 64 and
#            chunks is a power of two: (1, groups, 1) with groups = ceil(planes / (256 / tp)) <= 32768; else (ceil(tp / 256), gy, gz)
#   tile     (tiles of 8 x 32, C, min(ceil(4096 / (C * tiles)), N)); C <= 65535
# B16 (aux = C0): forward = the slot grid of glue_cases.py over the 4HW hi-res positions; backward (tiles of 8 x 16, C/16, gz),
#   gz = N until tiles * C/16 * N > 8192, then 8192 / (tiles * C/16)
DECODER = [
    ("relu_up2x_fwd", (2, 3, 5, 8), 0, "pair", (1, 6, 1)),                 # ceil(6 * 4 / 256) = 1; 6 planes
    ("relu_up2x_fwd", (64, 1024, 16, 16), 0, "pair", (1, 32768, 2)),       # ceil(17 * 8 / 256) = 1; 65536 planes over y and z
    ("relu_up2x_fwd", (2, 3, 5, 12), 0, "fwd4", (1, 1, 6)),                # W/2 = 6 -> 8 columns x 32 rows: ceil(6/8), ceil(10/32)
    ("relu_up2x_fwd", (1, 2, 40, 96), 0, "fwd4", (1, 20, 2)),              # W/2 = 48 -> 64 columns x 4 rows: ceil(48/64), ceil(80/4)
    ("relu_up2x_fwd", (2, 3, 5, 6), 0, "generic", (1, 1, 6)),              # 2W = 12 -> 16 columns x 16 rows: ceil(12/16), ceil(10/16)
    ("relu_up2x_fwd", (2, 3, 1, 8), 0, "fwd4", (1, 1, 6)),                 # H = 1: no pair form; 4 columns x 64 rows
    ("relu_up2x_fwd", (2, 3, 5, 8), 1, "generic", (1, 1, 6)),              # a broadcast source: 2W = 16 -> 16 x 16
    ("relu_up2x_fwd", (1, 1, 32768, 4), 0, None, None),                    # 2H > 65535
    ("relu_up2x_fwd", (65536, 32768, 2, 2), 0, None, None),                # 2^31 planes
    ("relu_up2x_bwd", (2, 3, 8, 8), 0, "sweep,planes", (1, 1, 1)),         # tp = 1 * 4: 64 planes per workgroup, 6 planes
    ("relu_up2x_bwd", (64, 1024, 16, 16), 0, "sweep,planes", (1, 4096, 1)),    # tp = 2 * 8 = 16: ceil(65536 / 16)
    ("relu_up2x_bwd", (1, 65536, 8, 8), 0, "sweep,planes", (1, 1024, 1)),  # C > 65535 is no obstacle here: ceil(65536 / 64)
    ("relu_up2x_bwd", (2, 3, 24, 8), 0, "sweep", (1, 6, 1)),               # chunks = 3: no power of two; tp = 12
    ("relu_up2x_bwd", (2, 3, 5, 8), 0, "tile", (1, 3, 2)),                 # H < 8; one tile; min(ceil(4096 / 3), 2)
    ("relu_up2x_bwd", (2, 3, 8, 8), 1, "tile", (1, 3, 2)),                 # a broadcast source
    ("relu_up2x_bwd", (3, 5, 9, 33), 0, "tile", (4, 5, 3)),                # 2 x 2 tiles; min(ceil(4096 / 20), 3)
    ("relu_up2x_bwd", (1, 65536, 5, 8), 0, None, None),                    # C > 65535 on the tile path
    ("b16_relu_up2x_fwd", (2, 32, 5, 8), 16, "slot", (2, 2, 2)),           # 320 slots: ceil(320 / 256) = 2
    ("b16_relu_up2x_fwd", (1, 16, 3, 3), 16, "slot", (1, 1, 1)),           # C1 = 0
    ("b16_relu_up2x_fwd", (1300, 32, 5, 10), 16, "slot,images", (2, 2, 1024)),     # 2 * 2 * 1300 > 4096: gz = 4096 / 4
    ("b16_relu_up2x_fwd", (2, 32, 5, 8), 8, None, None),                   # C0 % 16 != 0
    ("b16_relu_up2x_fwd", (2, 40, 5, 8), 16, None, None),                  # C1 % 16 != 0
    ("b16_relu_up2x_fwd", (65536, 32, 5, 8), 16, None, None),              # N > 65535
    ("b16_relu_up2x_bwd", (2, 32, 5, 8), 16, "tile", (1, 2, 2)),           # one tile, two blocks, two images
    ("b16_relu_up2x_bwd", (1300, 32, 20, 40), 16, "tile", (9, 2, 455)),    # 3 x 3 tiles; 18 * 1300 > 8192: gz = 8192 / 18
    ("b16_relu_up2x_bwd", (2, 32, 5, 8), 8, None, None),                   # C0 % 16 != 0
    ("b16_relu_up2x_bwd", (2, 40, 5, 8), 16, None, None),                  # C1 % 16 != 0
    ("b16_relu_up2x_bwd", (65536, 32, 5, 8), 16, None, None),              # N > 65535
]


@pytest.mark.parametrize("row", DECODER, ids=lambda r: f"{r[0]}-{'x'.join(map(str, r[1]))}-{r[2]}")
def test_plan_of_the_decoder_glue(row):
    op, dims, aux, form, grid = row
    buf, g = ctypes.create_string_buffer(64), (ctypes.c_int32 * 3)()
    rc = _lib().avsep_glue_plan(op.encode(), *dims, aux, buf, 64, g)
    if form is None:
        assert rc == -1, row
    else:
        assert (rc, buf.value.decode(), tuple(g)) == (0, form, grid), (row, rc, buf.value, tuple(g))


def test_every_form_of_the_decoder_glue_is_pinned():
    forms = {}
    for op, _, _, form, _ in DECODER:
        forms.setdefault(op, set()).add(form)
    assert forms == {"relu_up2x_fwd": {"pair", "fwd4", "generic", None}, "relu_up2x_bwd": {"sweep,planes", "sweep", "tile", None},
                     "b16_relu_up2x_fwd": {"slot", "slot,images", None}, "b16_relu_up2x_bwd": {"tile", None}}


@pytest.mark.parametrize("row", [r for r in S.SWEEP if r[1] in ("maxpool_fwd", "b16_maxpool_fwd") and r[2][1] < 65536],
                         ids=lambda r: f"{r[0]}-{S.case_id(r)}")
def test_pool_seeds_have_no_window_the_reference_itself_cannot_decide(row):
    import glue_inputs as I
    for act in (0, 1, 2):
        x, sc, sh = I.pool_operands(row, act)
        assert torch.equal(G.maxpool(x, sc, sh, act, exact=True)["tap"], G.maxpool(x, sc, sh, act, exact=False)["tap"]), (row, act)
