"""The sweep of the glue-kernel tests: per kernel the shapes that reach every launch form, every capped loop at least twice
and the edges, with the form and grid avsep_glue_plan must answer for each (tests/test_glue_plans_host.py pins them on the
host, tests/test_gpu_glue_forms.py runs them).  A plain module: no test lives here.

A row: (kernel, plan op, (N, C, H, W), aux, form, grid, loops that must be taken twice, what the shape is for).
(N, C, H, W) and aux mean what include/avsep.h says for the op: temporal mean (B, C, H, W) with aux = T, sgd n = N*C*H*W,
space_to_depth2 aux = Cp, the pools' planes are N*C.

Forms and thresholds (csrc/ops.hip, csrc/b16.hip), 256-thread workgroups throughout:
  channel_stats      "chunks"  grid (C, min(ceil(2048/C), ceil(N*HW/4096))): a chunk is a slice of the (n, hw) range that may
                     start inside an image; fp32 partial sums are flushed to fp64 every 64 terms
  bn_bwd_apply       "vec4" (HW % 4 == 0) | "scalar"; grid (min(ceil(HW/1024), 64), C, N)
  affine_act         "vec4" | "scalar"; grid (min(ceil(HW/1024 | HW/256), 64), C, N)
  affine_act_bwd     "v4" (HW % 4 == 0) | "v1"; grid (C, min(ceil(2048/C), ceil(N*HW/2048)))
  maxpool_fwd        "fwd4" (W % 8 == 0, H even, N*C <= 65535): grid (ceil(Ho*Wo/4/256), N*C) | "generic": min(.., 65536) flat
  maxpool_bwd        "gather": min(ceil(N*C*H*W/256), 65536) flat
  maxpool_bn_relu_bwd_stats   "plane": grid (C, N), a workgroup walks its pooled plane in steps of 256
  maxpool_bn_relu_bwd_apply   "apply4" (W % 4 == 0) | "pair" (W even), both N*C <= 65535 and grid (min(.., 64), N*C) |
                     "apply1": min(.., 262144) flat
  temporal_mean_*    "flat": min(.., 65536);   sgd "flat": min(.., 16384)
  space_to_depth2    "planes": grid (min(ceil(Hs*Ws/256), 16), min(N*Cp, 65535))
  f32_to_b16, b16_to_f32, bn_bwd_apply_to_b16   "position": grid (min(ceil(HW/256), 64), C/16, N)
  the B16 elementwise kernels, pools and channel sum   "slot": grid (gx = min(ceil(2*HW/256), 32), C/16, N) |
                     "slot,images": gz = 4096 / (gx * C/16) < N once gx * C/16 * N > 4096 (image-stride loop)
  b16_space_to_depth2   "flat": min(.., 262144)
  relu_up2x_fwd      "pair" | "fwd4" | "generic";   relu_up2x_bwd   "sweep,planes" | "sweep" | "tile"
  b16_relu_up2x_fwd  "slot" | "slot,images";        b16_relu_up2x_bwd   "tile"
                     (the decoder glue: no sweep rows here yet; form and grid are pinned by DECODER in test_glue_plans_host.py)
A launcher accepts or refuses a shape, and picks form and grid, in its *_plan function alone; avsep_glue_plan looks the op up in
one table and calls that function, so a refusal here is the launcher's.

Not reached (the size limit of a test's largest tensor is 2^25 elements):
  channel_stats, a flush followed by a remainder (>= 65 terms on a thread): needs 2048 * 16385 = 33 556 480 elements
      (the issue's [2, 1024, 130, 130] has 34 611 200); the flush itself fires at [1, 2048, 127, 127], 64 terms on thread 0
  maxpool_bn_relu_bwd_apply "apply1", 262144-workgroup cap: needs 2^26 + 1 = 67 108 865 elements
  b16_space_to_depth2, 262144-workgroup cap: needs 2^26 + 1 slots = 536 870 920 bf16 elements
  maxpool_fwd "generic", 65536-workgroup cap on maps larger than 1x1: needs 4 * (2^24 + 1) = 67 108 868 input elements
      (reached with 1x1 maps, 16 778 216 planes; maxpool_bwd is run on the same planes)
  temporal_mean_fwd 65536-workgroup cap with T >= 2: needs 2 * (2^24 + 1) = 33 554 434 elements (reached with T = 1)
"""
import ctypes

from recipes import cdiv, out_hw

BIG = 2 ** 24 + 1000
SIZE_LIMIT = 2 ** 25

SWEEP = [
    ("channel_stats", "channel_stats", (3, 5, 37, 41), 0, "chunks", (5, 2, 1), ("terms",), "two chunks, the boundary inside image 1"),
    ("channel_stats", "channel_stats", (1, 2, 1, 3), 0, "chunks", (2, 1, 1), (), "N = 1, one chunk, 3 live threads"),
    ("channel_stats", "channel_stats", (1, 2048, 127, 127), 0, "chunks", (2048, 1, 1), ("terms",), "64 terms on thread 0: the fp32 -> fp64 flush fires"),
    ("bn_bwd_apply", "bn_bwd_apply", (2, 3, 5, 8), 0, "vec4", (1, 3, 2), (), "HW % 4 == 0"),
    ("bn_bwd_apply", "bn_bwd_apply", (2, 3, 3, 7), 0, "scalar", (1, 3, 2), (), "HW % 4 == 1"),
    ("bn_bwd_apply", "bn_bwd_apply", (2, 3, 2, 11), 0, "scalar", (1, 3, 2), (), "HW % 4 == 2"),
    ("bn_bwd_apply", "bn_bwd_apply", (1, 2, 3, 5), 0, "scalar", (1, 2, 1), (), "HW % 4 == 3, N = 1"),
    ("bn_bwd_apply", "bn_bwd_apply", (1, 2, 13, 79), 0, "scalar", (2, 2, 1), ("x",), "HW = 1027: scalar form, three passes"),
    ("bn_bwd_apply", "bn_bwd_apply", (1, 1, 116, 569), 0, "vec4", (64, 1, 1), ("x",), "HW = 66004: 64-workgroup cap, ragged second pass"),
    ("bn_bwd_apply_to_b16", "bn_bwd_apply_to_b16", (1, 16, 5, 7), 0, "position", (1, 1, 1), (), "N = 1, C = 16"),
    ("bn_bwd_apply_to_b16", "bn_bwd_apply_to_b16", (3, 48, 9, 14), 0, "position", (1, 3, 3), (), "C = 48"),
    ("bn_bwd_apply_to_b16", "bn_bwd_apply_to_b16", (1, 16, 125, 132), 0, "position", (64, 1, 1), ("x",), "HW = 16500: 64-workgroup cap"),
    ("affine_act", "affine_act", (2, 3, 5, 8), 0, "vec4", (1, 3, 2), (), "HW % 4 == 0"),
    ("affine_act", "affine_act", (2, 3, 3, 7), 0, "scalar", (1, 3, 2), (), "HW % 4 == 1"),
    ("affine_act", "affine_act", (2, 3, 2, 11), 0, "scalar", (1, 3, 2), (), "HW % 4 == 2"),
    ("affine_act", "affine_act", (1, 2, 3, 5), 0, "scalar", (1, 2, 1), (), "HW % 4 == 3, N = 1"),
    ("affine_act", "affine_act", (1, 1, 116, 569), 0, "vec4", (64, 1, 1), ("x",), "HW = 66004: vector form past the cap"),
    ("affine_act", "affine_act", (1, 2, 29, 569), 0, "scalar", (64, 2, 1), ("x",), "HW = 16501: scalar form past the cap"),
    ("affine_act_bwd", "affine_act_bwd", (2, 3, 5, 8), 0, "v4", (3, 1, 1), (), "HW % 4 == 0"),
    ("affine_act_bwd", "affine_act_bwd", (2, 3, 3, 7), 0, "v1", (3, 1, 1), (), "HW % 4 == 1"),
    ("affine_act_bwd", "affine_act_bwd", (2, 3, 2, 11), 0, "v1", (3, 1, 1), (), "HW % 4 == 2"),
    ("affine_act_bwd", "affine_act_bwd", (1, 2, 3, 5), 0, "v1", (2, 1, 1), (), "HW % 4 == 3, N = 1"),
    ("affine_act_bwd", "affine_act_bwd", (5, 3, 7, 143), 0, "v1", (3, 3, 1), ("terms",), "HW = 1001: three chunks, none aligned to an image"),
    ("affine_act_bwd", "affine_act_bwd", (5, 3, 4, 251), 0, "v4", (3, 3, 1), ("terms",), "HW = 1004: the same in the vector form"),
    ("maxpool_fwd", "maxpool_fwd", (2, 3, 6, 16), 0, "fwd4", (1, 6, 1), (), "W % 8 == 0, even H"),
    ("maxpool_fwd", "maxpool_fwd", (1, 2, 40, 112), 0, "fwd4", (2, 2, 1), (), "fwd4, two workgroups per plane, the second ragged"),
    ("maxpool_fwd", "maxpool_fwd", (1, 2, 5, 8), 0, "generic", (1, 1, 1), (), "W % 8 == 0 but odd H"),
    ("maxpool_fwd", "maxpool_fwd", (2, 3, 7, 10), 0, "generic", (1, 1, 1), (), "W % 4 == 2, partial last window row"),
    ("maxpool_fwd", "maxpool_fwd", (2, 3, 5, 7), 0, "generic", (1, 1, 1), (), "odd W, partial last window row and column"),
    ("maxpool_fwd", "maxpool_fwd", (1, 2, 1, 9), 0, "generic", (1, 1, 1), (), "H = 1"),
    ("maxpool_fwd", "maxpool_fwd", (2, 2, 6, 1), 0, "generic", (1, 1, 1), (), "W = 1"),
    ("maxpool_fwd", "maxpool_fwd", (1, 3, 2, 2), 0, "generic", (1, 1, 1), (), "H = W = 2"),
    ("maxpool_fwd", "maxpool_fwd", (1, 65539, 4, 8), 0, "generic", (2049, 1, 1), (), "N*C > 65535: the scalar fallback"),
    ("maxpool_fwd", "maxpool_fwd", (1, BIG, 1, 1), 0, "generic", (65536, 1, 1), ("x",), "65536-workgroup cap (1x1 maps keep it under the size limit)"),
    ("maxpool_bwd", "maxpool_bwd", (2, 3, 6, 16), 0, "gather", (3, 1, 1), (), ""),
    ("maxpool_bwd", "maxpool_bwd", (2, 3, 5, 7), 0, "gather", (1, 1, 1), (), "odd sizes"),
    ("maxpool_bwd", "maxpool_bwd", (1, 2, 1, 9), 0, "gather", (1, 1, 1), (), "H = 1"),
    ("maxpool_bwd", "maxpool_bwd", (2, 2, 6, 1), 0, "gather", (1, 1, 1), (), "W = 1"),
    ("maxpool_bwd", "maxpool_bwd", (1, 65539, 4, 8), 0, "gather", (8193, 1, 1), (), "N*C > 65535"),
    ("maxpool_bwd", "maxpool_bwd", (1, BIG, 1, 1), 0, "gather", (65536, 1, 1), ("x",), "65536-workgroup cap"),
    ("maxpool_bn_relu_bwd_stats", "maxpool_bn_relu_bwd_stats", (2, 3, 6, 16), 0, "plane", (3, 2, 1), (), ""),
    ("maxpool_bn_relu_bwd_stats", "maxpool_bn_relu_bwd_stats", (2, 3, 5, 7), 0, "plane", (3, 2, 1), (), "odd sizes"),
    ("maxpool_bn_relu_bwd_stats", "maxpool_bn_relu_bwd_stats", (2, 3, 40, 30), 0, "plane", (3, 2, 1), ("terms",), "Ho*Wo = 300: second pass of 44"),
    ("maxpool_bn_relu_bwd_stats", "maxpool_bn_relu_bwd_stats", (1, 65539, 4, 8), 0, "plane", (65539, 1, 1), (), "65539 channels"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (2, 3, 6, 16), 0, "apply4", (1, 6, 1), (), "W % 4 == 0"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (2, 3, 5, 12), 0, "apply4", (1, 6, 1), (), "W % 4 == 0, odd H"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (1, 1, 129, 512), 0, "apply4", (64, 1, 1), ("x",), "apply4 past the 64-workgroup cap"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (2, 3, 5, 10), 0, "pair", (1, 6, 1), (), "W % 4 == 2"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (1, 3, 2, 2), 0, "pair", (1, 3, 1), (), "H = W = 2"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (1, 1, 128, 258), 0, "pair", (64, 1, 1), ("x",), "pair form past the cap"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (2, 3, 5, 7), 0, "apply1", (1, 1, 1), (), "odd W"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (1, 2, 1, 9), 0, "apply1", (1, 1, 1), (), "H = 1"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (2, 2, 6, 1), 0, "apply1", (1, 1, 1), (), "W = 1"),
    ("maxpool_bn_relu_bwd_apply", "maxpool_bn_relu_bwd_apply", (1, 65539, 4, 8), 0, "apply1", (8193, 1, 1), (), "N*C > 65535: the scalar fallback"),
    ("temporal_mean", "temporal_mean_fwd", (2, 3, 5, 7), 3, "flat", (1, 1, 1), (), "B = 2, T = 3"),
    ("temporal_mean", "temporal_mean_fwd", (1, 2, 3, 3), 4, "flat", (1, 1, 1), (), "B = 1, T = 4"),
    ("temporal_mean", "temporal_mean_fwd", (1, 1, 8, 2097277), 1, "flat", (65536, 1, 1), ("x",), "65536-workgroup cap (T = 1 keeps the input under the size limit)"),
    ("temporal_mean_bwd", "temporal_mean_bwd", (2, 3, 5, 7), 3, "flat", (3, 1, 1), (), "B = 2, T = 3"),
    ("temporal_mean_bwd", "temporal_mean_bwd", (1, 2, 3, 3), 4, "flat", (1, 1, 1), (), "B = 1, T = 4"),
    ("temporal_mean_bwd", "temporal_mean_bwd", (1, 1, 4, 2097277), 2, "flat", (65536, 1, 1), ("x",), "65536-workgroup cap"),
    ("sgd_momentum_", "sgd", (1, 1, 1, 1000), 0, "flat", (4, 1, 1), (), "n = 1000"),
    ("sgd_momentum_", "sgd", (1, 1, 1, 4195304), 0, "flat", (16384, 1, 1), ("x",), "16384-workgroup cap"),
    ("space_to_depth2", "space_to_depth2", (2, 3, 6, 8), 16, "planes", (1, 32, 1), (), "Cp = 16 > 4C: four dead planes per image"),
    ("space_to_depth2", "space_to_depth2", (1, 3, 4, 4), 12, "planes", (1, 12, 1), (), "Cp = 4C, N = 1"),
    ("space_to_depth2", "space_to_depth2", (1, 1, 124, 124), 4, "planes", (16, 4, 1), ("x",), "65 x 65 output plane: 16-workgroup cap"),
    ("space_to_depth2", "space_to_depth2", (16385, 1, 2, 2), 4, "planes", (1, 65535, 1), ("planes",), "65540 planes: the plane loop"),
    ("to_b16", "f32_to_b16", (1, 16, 5, 7), 0, "position", (1, 1, 1), (), "N = 1, C = 16"),
    ("to_b16", "f32_to_b16", (3, 48, 9, 14), 0, "position", (1, 3, 3), (), "C = 48"),
    ("to_b16", "f32_to_b16", (1, 16, 125, 132), 0, "position", (64, 1, 1), ("x",), "HW = 16500: 64-workgroup cap"),
    ("to_f32", "b16_to_f32", (1, 16, 5, 7), 0, "position", (1, 1, 1), (), "N = 1, C = 16"),
    ("to_f32", "b16_to_f32", (3, 48, 9, 14), 0, "position", (1, 3, 3), (), "C = 48"),
    ("to_f32", "b16_to_f32", (1, 16, 125, 132), 0, "position", (64, 1, 1), ("x",), "HW = 16500: 64-workgroup cap"),
    ("b16_affine_act", "b16_affine_act", (1, 16, 5, 7), 0, "slot", (1, 1, 1), (), "N = 1, C = 16"),
    ("b16_affine_act", "b16_affine_act", (3, 48, 9, 14), 0, "slot", (1, 3, 3), (), "C = 48"),
    ("b16_affine_act", "b16_affine_act", (1, 16, 50, 83), 0, "slot", (32, 1, 1), ("slots",), "HW = 4150: 32-workgroup cap, ragged second pass"),
    ("b16_affine_act", "b16_affine_act", (1300, 32, 10, 20), 0, "slot,images", (2, 2, 1024), ("images",), "gz = 1024 < N: one or two images per workgroup"),
    ("b16_affine_act_bwd", "b16_affine_act_bwd", (1, 16, 5, 7), 0, "slot", (1, 1, 1), (), "N = 1, C = 16"),
    ("b16_affine_act_bwd", "b16_affine_act_bwd", (3, 48, 9, 14), 0, "slot", (1, 3, 3), (), "C = 48"),
    ("b16_affine_act_bwd", "b16_affine_act_bwd", (1, 16, 50, 83), 0, "slot", (32, 1, 1), ("slots",), "HW = 4150: 32-workgroup cap, ragged second pass"),
    ("b16_affine_act_bwd", "b16_affine_act_bwd", (1300, 32, 10, 20), 0, "slot,images", (2, 2, 1024), ("images",), "gz = 1024 < N: one or two images per workgroup"),
    ("b16_bn_bwd_apply", "b16_bn_bwd_apply", (1, 16, 5, 7), 0, "slot", (1, 1, 1), (), "N = 1, C = 16"),
    ("b16_bn_bwd_apply", "b16_bn_bwd_apply", (3, 48, 9, 14), 0, "slot", (1, 3, 3), (), "C = 48"),
    ("b16_bn_bwd_apply", "b16_bn_bwd_apply", (1, 16, 50, 83), 0, "slot", (32, 1, 1), ("slots",), "HW = 4150: 32-workgroup cap, ragged second pass"),
    ("b16_bn_bwd_apply", "b16_bn_bwd_apply", (1300, 32, 10, 20), 0, "slot,images", (2, 2, 1024), ("images",), "gz = 1024 < N: one or two images per workgroup"),
    ("b16_maxpool", "b16_maxpool_fwd", (1, 16, 5, 7), 0, "slot", (1, 1, 1), (), "N = 1, C = 16, odd sizes"),
    ("b16_maxpool", "b16_maxpool_fwd", (3, 48, 6, 16), 0, "slot", (1, 3, 3), (), "C = 48"),
    ("b16_maxpool", "b16_maxpool_fwd", (1, 16, 1, 9), 0, "slot", (1, 1, 1), (), "H = 1"),
    ("b16_maxpool", "b16_maxpool_fwd", (2, 16, 6, 1), 0, "slot", (1, 1, 2), (), "W = 1"),
    ("b16_maxpool", "b16_maxpool_fwd", (1, 16, 2, 2), 0, "slot", (1, 1, 1), (), "H = W = 2"),
    ("b16_maxpool", "b16_maxpool_fwd", (1, 16, 100, 165), 0, "slot", (32, 1, 1), ("slots",), "Ho*Wo = 4150"),
    ("b16_maxpool", "b16_maxpool_fwd", (2100, 32, 4, 4), 0, "slot,images", (1, 2, 2048), ("images",), "gz = 2048 < N"),
    ("b16_maxpool_bwd_stats", "b16_maxpool_bwd_stats", (1, 16, 5, 7), 0, "slot", (1, 1, 1), (), "N = 1, C = 16, odd sizes"),
    ("b16_maxpool_bwd_stats", "b16_maxpool_bwd_stats", (3, 48, 6, 16), 0, "slot", (1, 3, 3), (), "C = 48"),
    ("b16_maxpool_bwd_stats", "b16_maxpool_bwd_stats", (1, 16, 100, 165), 0, "slot", (32, 1, 1), ("slots",), "Ho*Wo = 4150"),
    ("b16_maxpool_bwd_stats", "b16_maxpool_bwd_stats", (2100, 32, 4, 4), 0, "slot,images", (1, 2, 2048), ("images",), "gz = 2048 < N"),
    ("b16_maxpool_bwd_apply", "b16_maxpool_bwd_apply", (1, 16, 5, 7), 0, "slot", (1, 1, 1), (), "N = 1, C = 16, odd sizes"),
    ("b16_maxpool_bwd_apply", "b16_maxpool_bwd_apply", (3, 48, 6, 16), 0, "slot", (1, 3, 3), (), "C = 48"),
    ("b16_maxpool_bwd_apply", "b16_maxpool_bwd_apply", (1, 16, 1, 9), 0, "slot", (1, 1, 1), (), "H = 1"),
    ("b16_maxpool_bwd_apply", "b16_maxpool_bwd_apply", (2, 16, 6, 1), 0, "slot", (1, 1, 2), (), "W = 1"),
    ("b16_maxpool_bwd_apply", "b16_maxpool_bwd_apply", (1, 16, 50, 83), 0, "slot", (32, 1, 1), ("slots",), "H*W = 4150"),
    ("b16_maxpool_bwd_apply", "b16_maxpool_bwd_apply", (2100, 32, 4, 4), 0, "slot,images", (1, 2, 2048), ("images",), "gz = 2048 < N"),
    ("b16_channel_sum", "b16_channel_sum", (2, 16, 9, 14), 0, "slot", (1, 1, 2), (), "dbias of a 16 -> 16 3x3 conv's B16 weight gradient"),
    ("b16_channel_sum", "b16_channel_sum", (3, 48, 9, 14), 0, "slot", (1, 3, 3), (), "C = 48"),
    ("b16_channel_sum", "b16_channel_sum", (1, 16, 50, 83), 0, "slot", (32, 1, 1), ("slots",), "N = 1, HW = 4150"),
    ("b16_channel_sum", "b16_channel_sum", (1300, 32, 10, 20), 0, "slot,images", (2, 2, 1024), ("images",), "gz = 1024 < N"),
    ("b16_space_to_depth2", "b16_space_to_depth2", (2, 3, 6, 8), 0, "flat", (1, 1, 1), (), "C = 3: four dead channels"),
    ("b16_space_to_depth2", "b16_space_to_depth2", (1, 1, 2, 4), 0, "flat", (1, 1, 1), (), "C = 1, N = 1"),
    ("b16_space_to_depth2", "b16_space_to_depth2", (3, 4, 20, 20), 0, "flat", (4, 1, 1), (), "C = 4: all 16 channels live, four workgroups, the last ragged"),
]

KERNELS = sorted({r[0] for r in SWEEP})


def cases(kernel):
    return [r for r in SWEEP if r[0] == kernel]


def case_id(r):
    return "x".join(str(d) for d in r[2]) + (f"-{r[3]}" if r[3] else "")


def plan(L, op, dims, aux=0):
    """(form, grid) avsep_glue_plan answers; L = the loaded library."""
    form = ctypes.create_string_buffer(64)
    grid = (ctypes.c_int32 * 3)()
    rc = L.avsep_glue_plan(op.encode(), *dims, aux, form, 64, grid)
    assert rc == 0, (op, dims, aux, rc)
    return form.value.decode(), tuple(grid)


def loops(op, dims, aux, form, grid):
    """extent / (what one pass of the launched grid covers) for every capped loop of the op's kernel: > 1 means the loop body
    runs at least twice on some thread (grid * 256 * V < extent).  "terms": per-thread terms of a chunked or per-plane sum."""
    N, C, H, W = dims
    HW, gx, gy, gz = H * W, grid[0], grid[1], grid[2]
    Ho, Wo = out_hw(H), out_hw(W)
    if op == "channel_stats":
        return {"terms": cdiv(cdiv(N * HW, gy), 256)}
    if op in ("bn_bwd_apply", "affine_act"):
        return {"x": (HW // 4 if form == "vec4" else HW) / (gx * 256)}
    if op == "affine_act_bwd":
        return {"terms": cdiv(cdiv(N * (HW // 4 if form == "v4" else HW), gy), 256)}
    if op == "maxpool_fwd":
        return {"x": 1.0 if form == "fwd4" else N * C * Ho * Wo / (gx * 256)}
    if op == "maxpool_bwd":
        return {"x": N * C * HW / (gx * 256)}
    if op == "maxpool_bn_relu_bwd_stats":
        return {"terms": cdiv(Ho * Wo, 256)}
    if op == "maxpool_bn_relu_bwd_apply":
        return {"x": {"apply4": HW // 4, "pair": HW // 2, "apply1": N * C * HW}[form] / (gx * 256)}
    if op == "temporal_mean_fwd":
        return {"x": N * C * HW / (gx * 256)}
    if op == "temporal_mean_bwd":
        return {"x": N * aux * C * HW / (gx * 256)}
    if op == "sgd":
        return {"x": N * C * HW / (gx * 256)}
    if op == "space_to_depth2":
        return {"x": (H // 2 + 3) * (W // 2 + 3) / (gx * 256), "planes": N * aux / gy}
    if op in ("f32_to_b16", "b16_to_f32", "bn_bwd_apply_to_b16"):
        return {"x": HW / (gx * 256)}
    if op == "b16_space_to_depth2":
        return {"x": N * (H // 2 + 3) * (W // 2 + 3) * 2 / (gx * 256)}
    ext = Ho * Wo if op in ("b16_maxpool_fwd", "b16_maxpool_bwd_stats") else HW
    return {"slots": 2 * ext / (gx * 256), "images": N / gz, "terms": cdiv(2 * ext, gx * 256) * cdiv(N, gz)}


def largest_tensor(op, dims, aux):
    N, C, H, W = dims
    n = N * C * H * W
    if op in ("temporal_mean_fwd", "temporal_mean_bwd"):
        n *= aux
    if op == "space_to_depth2":
        n = max(n, N * aux * (H // 2 + 3) * (W // 2 + 3))
    if op == "b16_space_to_depth2":
        n = max(n, N * 16 * (H // 2 + 3) * (W // 2 + 3))
    return n
