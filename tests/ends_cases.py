"""The rows of the step-end kernel tests (tests/test_endsref.py checks them on the host, tests/test_gpu_step_ends.py runs them)
and their operands, drawn on the CPU from a seed that is a function of the row alone.  A plain module: no test lives here.

A row is a dict: "op" (the launcher group), the sizes and switches of the call, and "note": the form or edge it reaches.
Forms and thresholds (csrc/ops.hip, fusion.hip, fusion_n.hip, attention.hip), 256-thread workgroups throughout:
  mask_loss_fwd / _bwd   grid (min(ceil(FT / 1024), 64), B): a thread loops once FT > 256 * gx; S = 1..4; `c != 0.f` skips a term
  prepare / warp         grid (Fout, B) / (Hout, BC); a thread loops over t in steps of 256
  innerprod_fwd          grid (min(ceil(HW / 256), 256), B), K * 4 bytes of LDS, K <= 8192
  innerprod_bwd          grid (K, B), a workgroup strides HW by 256; dsnd optional, scale optional
  innerprod_nosum        "vec4" (HW % 4 == 0) | "scalar"; grid (min(ceil(HW / 1024), 64), B * K)
  innerprod_pixelwise    grid (ceil(HW / 128), B); 32-row tiles of P; LDS K * (roundup(P, 32) + 1) * 4, opt-in above 64 KB
  sdr_sums               grid (min(ceil(L / 2048), 64), R)
  fusion_av_fwd / _bwd   one workgroup per sample / (B, parts), parts = 4 (B < 128), 2 (B < 256), 1, clamped to Dc; LDS
                         (4 Dc + 10 HW + 44) * 4, opt-in above 64 KB, rejected above 160 KB
  fusion_n_av_*          one workgroup per sample, C = 2..4, LDS (D + 2 C C HW + C HW + 61) * 4
  attmodel_infer_*       one workgroup per sample, S <= 4, K <= 128, HW <= 4096

Not reached under the size limit of 2^25 elements per tensor: nothing in this list; the 160 KB rejections need no launch and
are checked on the host (tests/test_endsref.py).
"""
import itertools
import math
import zlib

import torch

import endsref as E

SIZE_LIMIT = 2 ** 25
F32 = torch.float32


def case_id(row):
    return row["id"]


def gen(row, salt=""):
    return torch.Generator().manual_seed(zlib.crc32(f"{row['op']}-{row['id']}-{salt}".encode()))


def _r(op, id, note, **kw):
    return dict(op=op, id=id, note=note, **kw)


A, Ls = {"none": 0, "relu": 1, "sigmoid": 3, "tanh": 4, "softmax": 5}, {"bce": 0, "l1": 1, "l2": 2}
_COEF = ("identity", "full", "perm", "zeros")
_WEIGHT = (None, "shared", "target")

ROWS = []
# ---- mask loss: every activation x loss the model can build, [B, S, FT] = [2, 2, 30] ------------------------------------
_n = 0
for _loss in ("bce", "l1", "l2"):
    for _act in (("sigmoid", "softmax", "none") if _loss == "bce" else ("none", "relu", "sigmoid", "tanh", "softmax")):
        ROWS.append(_r("mask_loss", f"{_act}-{_loss}-2x2x30", f"base sweep, coef {_COEF[_n % 4]}, weight {_WEIGHT[_n % 3]}",
                       B=2, S=2, FT=30, act=_act, loss=_loss, coef=_COEF[_n % 4], weight=_WEIGHT[_n % 3], targets="binary"))
        _n += 1
ROWS += [
    _r("mask_loss", "S1-sigmoid-bce-1027", "S = 1, FT = 1027: four strided iterations, the last ragged; per-target weights",
       B=2, S=1, FT=1027, act="sigmoid", loss="bce", coef="full", weight="target", targets="binary"),
    _r("mask_loss", "S3-softmax-l2-1027", "S = 3, a permutation matrix that differs per sample, shared weights",
       B=3, S=3, FT=1027, act="softmax", loss="l2", coef="perm", weight="shared", targets="binary"),
    _r("mask_loss", "S4-softmax-bce-1027", "S = 4, full coef, per-target weights",
       B=2, S=4, FT=1027, act="softmax", loss="bce", coef="full", weight="target", targets="binary"),
    _r("mask_loss", "S4-tanh-l1-1027", "S = 4, coef with exact zeros (the c != 0.f skip), no weights",
       B=2, S=4, FT=1027, act="tanh", loss="l1", coef="zeros", weight=None, targets="binary"),
    _r("mask_loss", "S3-sigmoid-bce-1027", "S = 3, PIT's off-diagonal permutation coef, per-target weights",
       B=3, S=3, FT=1027, act="sigmoid", loss="bce", coef="perm", weight="target", targets="binary"),
    _r("mask_loss", "cap-sigmoid-bce-65541", "FT = 64 * 1024 + 5: the grid cap of 64, every thread loops (5 terms on the first)",
       B=1, S=2, FT=64 * 1024 + 5, act="sigmoid", loss="bce", coef="perm", weight="shared", targets="binary"),
    _r("mask_loss", "saturating-sigmoid-bce", "logits in +-30: pred == 1.0f, the log clamp -100 (forward only, sums staged on pred)",
       B=2, S=2, FT=300, act="sigmoid", loss="bce", coef="identity", weight="shared", targets="binary", scale=30.0, fwd_only=True),
    _r("mask_loss", "ratio-relu-l1", "ratio targets in [0, 5], L1 under the margin rule", B=2, S=2, FT=300, act="relu", loss="l1",
       coef="full", weight="target", targets="ratio"),
    _r("mask_loss", "ratio-sigmoid-l1", "ratio targets, L1 sign behind an inexact activation", B=2, S=2, FT=300, act="sigmoid",
       loss="l1", coef="full", weight="shared", targets="ratio01"),
    _r("mask_loss", "ratio-none-l2", "ratio targets in [0, 5], L2", B=2, S=3, FT=300, act="none", loss="l2", coef="zeros",
       weight="shared", targets="ratio"),
]
# ---- prepare and warp -------------------------------------------------------------------------------------------------------
ROWS += [
    _r("prepare", "S1-warp64to256-T255-w-bin", "S = 1, log-frequency warp 64 -> 256, weighted, binary masks (margin rule on the warped values)",
       S=1, B=2, Fin=64, T=255, Fout=256, warp=1, weighted=1, binary=1, mix="sum"),
    _r("prepare", "S2-warp33to20-T257-ratio-x8", "S = 2, warp 33 -> 20 (down), T = 257: the stride loop; sources up to 8x the mixture: clamp at 5",
       S=2, B=2, Fin=33, T=257, Fout=20, warp=1, weighted=0, binary=0, mix="x8"),
    _r("prepare", "S3-nowarp7-T600-span-ratio", "S = 3, no warp, T = 600 (three passes); mixtures 1e-12 .. e^11: both clamps of the weight",
       S=3, B=2, Fin=7, T=600, Fout=7, warp=0, weighted=1, binary=0, mix="span"),
    _r("prepare", "S4-nowarp7-T1-zero-bin", "S = 4, T = 1, a silent mixture (log(1e-10)), binary masks", S=4, B=3, Fin=7, T=1, Fout=7,
       warp=0, weighted=1, binary=1, mix="zero"),
    _r("prepare", "S2-warp64to256-T600-span-bin", "warp on, T = 600, mixtures over both clamps of the weight, binary masks",
       S=2, B=1, Fin=64, T=600, Fout=256, warp=1, weighted=1, binary=1, mix="span"),
    _r("prepare", "S2-nowarp7-T255-zero-ratio", "a zero mixture under the ratio mask (clamp at 5 / 0), unweighted", S=2, B=2, Fin=7,
       T=255, Fout=7, warp=0, weighted=0, binary=0, mix="zero"),
    _r("prepare", "S4-warp33to20-T1-bin", "S = 4, T = 1 with the warp (linspace of one point)", S=4, B=2, Fin=33, T=1, Fout=20, warp=1,
       weighted=1, binary=1, mix="sum"),
    _r("warp", "unwarp-256to512-W300", "avsep_warp, warp = 0 (the un-warp), 256 -> 512, Wout = 300: two passes over t",
       BC=3, Hin=256, Win=300, Hout=512, Wout=300, warp=0),
    _r("warp", "warp-512to256-W300", "avsep_warp, warp = 1, 512 -> 256, Win = 37 -> Wout = 300", BC=2, Hin=512, Win=37, Hout=256,
       Wout=300, warp=1),
]
# ---- synthesizer ------------------------------------------------------------------------------------------------------------
ROWS += [
    _r("innerprod_fwd", "K1-HW1", "K = 1, HW = 1", B=2, K=1, HW=1, scale=True, bias=True),
    _r("innerprod_fwd", "K3-HW255", "K = 3, HW = 255: one ragged workgroup; no scale (Bias)", B=2, K=3, HW=255, scale=False, bias=True),
    _r("innerprod_fwd", "K32-HW257", "K = 32, HW = 257: two workgroups; no bias", B=2, K=32, HW=257, scale=True, bias=False),
    _r("innerprod_fwd", "K8192-HW257", "K = 8192: the LDS limit of the launcher", B=1, K=8192, HW=257, scale=True, bias=True),
    _r("innerprod_fwd", "K3-HW65836", "HW = 65536 + 300: the grid cap of 256, a second ragged pass", B=1, K=3, HW=65836, scale=True, bias=True),
    _r("innerprod_bwd", "HW1", "HW = 1", B=2, K=5, HW=1, scale=True, dsnd=True),
    _r("innerprod_bwd", "HW63-noscale", "HW = 63: one wave short; scale == NULL (Bias)", B=2, K=5, HW=63, scale=False, dsnd=True),
    _r("innerprod_bwd", "HW64-nodsnd", "HW = 64; dsnd == NULL", B=2, K=5, HW=64, scale=True, dsnd=False),
    _r("innerprod_bwd", "HW257-noscale-nodsnd", "HW = 257: a second, ragged pass; both null", B=3, K=4, HW=257, scale=False, dsnd=False),
    _r("innerprod_bwd", "HW5000", "HW = 5000: 20 passes", B=2, K=5, HW=5000, scale=True, dsnd=True),
] + [_r("innerprod_nosum", f"HW{hw}", f"HW % 4 == {hw % 4}" + (": vec4" if hw % 4 == 0 else ": scalar"), B=2, K=3, HW=hw, scale=hw != 9, bias=hw != 10)
     for hw in (8, 9, 10, 11)] + [
    _r("innerprod_nosum", "HW262152", "HW = 64 * 1024 * 4 + 8: the vec4 loop past the grid cap", B=1, K=2, HW=64 * 1024 * 4 + 8, scale=True, bias=True),
    _r("innerprod_nosum", "HW16387", "HW = 64 * 256 + 3: the scalar loop, four passes", B=1, K=2, HW=64 * 256 + 3, scale=True, bias=True),
    _r("innerprod_pixelwise", "K2-P1-HW1", "K = 2, P = 1, HW = 1", B=2, K=2, P=1, HW=1, scale=True, bias=True),
    _r("innerprod_pixelwise", "K34-P31-HW127", "P = 31, HW = 127: both one short of a tile", B=2, K=34, P=31, HW=127, scale=True, bias=False),
    _r("innerprod_pixelwise", "K2-P33-HW128", "P = 33: a second tile of one row; HW = 128 exactly; no scale", B=1, K=2, P=33, HW=128, scale=False, bias=True),
    _r("innerprod_pixelwise", "K34-P196-HW129", "P = 196 (14 x 14), HW = 129: a second workgroup of one position", B=2, K=34, P=196, HW=129, scale=True, bias=True),
    _r("innerprod_pixelwise", "K128-P128-HW129", "(K, P) = (128, 128): 66 048 B of LDS, the opt-in above 64 KB", B=1, K=128, P=128, HW=129, scale=True, bias=True),
] + [_r("sdr_sums", f"L{L}", note, R=3, L=L, pad=pad) for L, pad, note in (
    (1, 0, "L = 1"), (2047, 5, "L = 2047, row strides larger than L"), (2049, 0, "L = 2049: a second workgroup of one sample"),
    (64 * 2048 + 777, 3, "L = 64 * 2048 + 777: the grid cap, strided rows"))]
# ---- fusion (two sources) -----------------------------------------------------------------------------------------------------
_KN = ("hidsep", "sel", "mixvis")
_AN = ("cos", "sig")


def _fav(id, note, B, Dc, HW, FT, kind, att, dmaps=True, dmatch=True, null=None, special=None, vscale=0.1):
    return _r("fusion_av", id, note, B=B, Dc=Dc, HW=HW, FT=FT, kind=kind, att=att, dmaps=dmaps, dmatch=dmatch, null=null,
              special=special, vscale=vscale)


ROWS += [_fav(f"{_KN[k]}-{_AN[a]}-3x32x20x4", "base sweep" + ("" if (k + a) % 2 else ", dmaps null") + (", dmatch null (scale only)" if k == a else ""),
              3, 32, 20, 4, k, a, dmaps=bool((k + a) % 2), dmatch=k != a) for k in range(3) for a in range(2)]
ROWS += [
    _fav("parts2-B128-Dc8", "B = 128: parts = 2", 128, 8, 20, 4, 0, 0),
    _fav("parts1-B256-Dc8", "B = 256: parts = 1", 256, 8, 20, 4, 0, 1),
    _fav("Dc10-slices", "Dc = 10 over 4 parts: slices of 2, 3, 2, 3 channels", 3, 10, 20, 4, 1, 0),
    _fav("Dc3-clamped", "Dc = 3: parts clamped to 3", 3, 3, 20, 4, 2, 0, vscale=0.3),
    _fav("Dc1-clamped", "Dc = 1: parts clamped to 1", 3, 1, 20, 4, 0, 1, vscale=1.0),
    _fav("HW1", "HW = 1", 3, 16, 1, 4, 0, 1),
    _fav("HW63", "HW = 63", 3, 16, 63, 5, 1, 0),
    _fav("HW65", "HW = 65: a second lane pass of one", 3, 16, 65, 4, 2, 1),
    _fav("HW196", "HW = 196", 2, 16, 196, 4, 0, 0),
    _fav("HW300", "HW = 300: a second thread pass", 2, 16, 300, 3, 2, 0),
    _fav("lds-HW1640-Dc16", "HW = 41 * 40, Dc = 16: 66 032 B of LDS, the opt-in above 64 KB", 2, 16, 1640, 4, 0, 0),
    _fav("null-dx", "dx == NULL", 3, 32, 20, 4, 0, 0, null="dx"),
    _fav("null-dv0", "dv0 == NULL", 3, 32, 20, 4, 1, 1, null="dv0"),
    _fav("null-dv1", "dv1 == NULL", 3, 32, 20, 4, 0, 1, null="dv1"),
    _fav("eps-zero-position", "cos: one visual position all zero (nv == 0: both epsilon branches of dv)", 3, 16, 20, 4, 0, 0, special="zero_v"),
    _fav("eps-zero-audio", "cos: the pooled vector of audio block 1 all zero (na == 0)", 3, 16, 20, 4, 1, 0, special="zero_a"),
    _fav("eps-mixvis-zero-selected", "cos MixVis: the selected visual vector is zero (nu == 0)", 3, 16, 20, 4, 2, 0, special="zero_sel"),
    _fav("tie-columns-hidsep", "two bitwise equal columns of v0 carry the maximum of map (0, 0): the first wins", 3, 16, 20, 4, 0, 0, special="tie_cols"),
    _fav("tie-columns-sel", "the same under CoLoc_Sel, where the arg-max selects the vector", 3, 16, 20, 4, 1, 0, special="tie_cols"),
    _fav("tie-zero-channel", "a channel of v0 zero everywhere: v * att == 0, index 0 wins", 3, 16, 20, 4, 0, 1, special="zero_channel"),
    _fav("tie-equal-maps", "v1 == v0 bit for bit: equal permutation scores, best must be 0", 3, 16, 20, 4, 0, 0, special="equal_maps"),
    _r("fusion_ao", "B3-Dc16", "mixed draws", B=3, Dc=16, FT=4, draws=(1, 0, 1)),
    _r("fusion_ao", "B4-Dc33-allzero", "every draw 0: the one_hot width quirk, both slots take block 1", B=4, Dc=33, FT=7, draws=(0, 0, 0, 0)),
    _r("fusion_ao", "B2-Dc300", "Dc = 300: 2 Dc > 256, a second thread pass", B=2, Dc=300, FT=3, draws=(0, 1)),
]


# ---- fusion for C sources ------------------------------------------------------------------------------------------------------
def _fn(id, note, B, C, D, HW, FT, att, dmatch=True, special=None, vscale=0.1):
    return _r("fusion_n_av", id, note, B=B, C=C, D=D, HW=HW, FT=FT, att=att, dmatch=dmatch, special=special, vscale=vscale)


ROWS += [
    _fn("C2-D64-HW20-cos", "C = 2: bit for bit fusion.hip's kind 0", 2, 2, 64, 20, 4, 0),
    _fn("C3-D66-HW20-cos", "C = 3, D = 66", 2, 3, 66, 20, 4, 0),
    _fn("C4-D64-HW196-sig", "C = 4, HW = 196, dmatch null", 2, 4, 64, 196, 3, 1, dmatch=False),
    _fn("C3-D3-HW1-sig", "D = C: one channel per block, HW = 1", 2, 3, 3, 1, 4, 1, vscale=1.0),
    _fn("C4-D66-HW20-sig", "C = 4, D = 66: a remainder of two channels", 2, 4, 66, 20, 4, 1),
    _fn("C4-D512-HW20-cos", "D = 512", 1, 4, 512, 20, 3, 0),
    _fn("C2-D66-HW1-cos", "C = 2, HW = 1", 2, 2, 66, 1, 4, 0, vscale=0.3),
    _fn("lds-C4-HW600", "C = 4, HW = 600: 86 908 B of LDS, the opt-in above 64 KB", 1, 4, 66, 600, 3, 1),
    _fn("eps-zero-position", "cos: one visual position all zero", 2, 3, 48, 20, 4, 0, special="zero_v"),
    _fn("eps-zero-audio", "cos: audio block 1 pooled to zero", 2, 3, 48, 20, 4, 0, special="zero_a"),
    _fn("tie-columns", "two bitwise equal columns of v0 carry the maximum of map (0, 0)", 2, 3, 48, 20, 4, 0, special="tie_cols"),
    _fn("tie-zero-channel", "a channel of v0 zero everywhere: index 0 wins", 2, 3, 48, 20, 4, 1, special="zero_channel"),
    _fn("tie-equal-maps", "C = 2, v1 == v0 bit for bit: the two scores are the same two terms, best must be 0 (for C > 2 the sums differ in their order: no exact tie)",
        2, 2, 66, 20, 4, 0, special="equal_maps"),
] + [_r("fusion_n_ao", f"C{C}-D{D}", f"every permutation index of C = {C} as a draw" + (", a remainder" if D % C else ""), C=C, D=D, FT=FT,
        B=math.factorial(C)) for C, D, FT in ((2, 2, 3), (3, 66, 5), (4, 64, 4), (4, 512, 2), (3, 64, 3))]


# ---- attention -------------------------------------------------------------------------------------------------------------------
def _att(id, note, B, S, K, HW, att, dmaps=True, dmatch=True, special=None):
    return _r("attention", id, note, B=B, S=S, K=K, HW=HW, att=att, dmaps=dmaps, dmatch=dmatch, special=special)


ROWS += [
    _att("S1-K7-HW1-sig", "S = 1, HW = 1", 2, 1, 7, 1, 1),
    _att("S2-K128-HW63-cos", "S = 2, K = 128, HW = 63; dmaps null", 2, 2, 128, 63, 0, dmaps=False),
    _att("S4-K7-HW257-cos", "S = 4, K = 7, HW = 257: a second thread pass; dmatch null", 2, 4, 7, 257, 0, dmatch=False),
    _att("S2-K1-HW63-sig", "K = 1; both null", 2, 2, 1, 63, 1, dmaps=False, dmatch=False),
    _att("S4-K128-HW4096-sig", "the limit shape: 67 KB / 151 KB of LDS", 1, 4, 128, 4096, 1),
    _att("S4-K128-HW4096-cos", "the limit shape, cos", 1, 4, 128, 4096, 0),
    _att("zero-query-cos", "cos: a zero query (na == 0)", 2, 2, 16, 63, 0, special="zero_a"),
    _att("zero-position-cos", "cos: a zero visual position (nv == 0)", 2, 2, 16, 63, 0, special="zero_v"),
]


def cases(op):
    return [r for r in ROWS if r["op"] == op]


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _randn(g, *shape):
    return torch.randn(shape, generator=g)


def _rand(g, *shape):
    return torch.rand(shape, generator=g)


def coef_matrix(row, g):
    B, S, FT = row["B"], row["S"], row["FT"]
    kind = row["coef"]
    if kind == "identity":
        return (torch.eye(S)[None].expand(B, S, S) / (B * S * FT)).contiguous()
    if kind == "perm":                      # what PIT sends: the permutation matrix of sample b, a different one per sample
        perms = list(itertools.permutations(range(S)))
        c = torch.zeros(B, S, S)
        for b in range(B):
            for i, j in enumerate(perms[(b + 1) % len(perms)]):
                c[b, i, j] = 1.0 / (B * S * FT)
        return c
    c = _randn(g, B, S, S)
    if kind == "zeros":
        c = c * (_rand(g, B, S, S) > 0.5)
    return c


def mask_loss_inputs(row):
    """(logits [B, S, FT], gt [S, B, FT], weight, coef [B, S, S]) with every L1 sign and BCE floor decidable."""
    g = gen(row)
    B, S, FT, act, loss = row["B"], row["S"], row["FT"], A[row["act"]], Ls[row["loss"]]
    if act == 0 and loss == 0:
        logits = _rand(g, B, S, FT) * 0.96 + 0.02           # no activation before BCE: the inputs are probabilities
    elif "scale" in row:
        logits = (_rand(g, B, S, FT) * 2 - 1) * row["scale"]
    else:
        logits = _randn(g, B, S, FT) * 3
    t = row["targets"]
    gt = (_rand(g, S, B, FT) > 0.5).float() if t == "binary" else _rand(g, S, B, FT) * (5.0 if t == "ratio" else 1.0)
    weight = {None: None, "shared": _rand(g, B, FT) + 0.1, "target": _rand(g, S, B, FT) + 0.1}[row["weight"]]
    coef = coef_matrix(row, g)
    if not row.get("fwd_only"):
        for _ in range(8):
            bad = mask_loss_undecided(logits, gt, weight, coef, act, loss)
            if not bool(bad.any()):
                break
            logits = torch.where(bad, logits * 0.5 + 0.11, logits)       # out of the saturation, off the target
        else:
            raise AssertionError("mask_loss_inputs did not converge")
    return logits, gt, weight, coef


def mask_loss_undecided(logits, gt, weight, coef, act, loss):
    _, _, margins = E.mask_loss_bwd(logits, gt, weight, coef, act, loss)
    bad = torch.zeros(logits.shape, dtype=torch.bool)
    for m, s in margins.values():
        bad |= ~E.decided(m, s)
    return bad


def prepare_inputs(row):
    """(mag_mix [B, Fin, T], mags [S, B, Fin, T]).  Without the warp the binary masks are made decidable here; with it the
    interpolated values cannot be resampled and the test excludes what the reference proves undecidable."""
    g = gen(row)
    S, B, Fin, T = row["S"], row["B"], row["Fin"], row["T"]
    mags = _randn(g, S, B, Fin, T).abs()
    kind = row["mix"]
    if kind == "sum":
        mix = mags.sum(0) * (0.5 + _rand(g, B, Fin, T))
    elif kind == "x8":
        mix = mags.amax(0) / (8.0 * _rand(g, B, Fin, T)).clamp_min(0.05)
    elif kind == "span":
        mix = torch.exp(math.log(1e-12) + _rand(g, B, Fin, T) * (11.0 - math.log(1e-12)))
    else:
        mags = mags * (_rand(g, S, B, Fin, T) > 0.1)        # silent sources too: the ratio mask's lower clamp
        mix = mags.sum(0) * (_rand(g, B, Fin, T) > 0.3)
    if row["binary"] and not row["warp"]:
        for _ in range(8):
            m, s = E.prepare(mix, mags, 0, row["weighted"], 1, row["Fout"])["gt_margin"]
            bad = ~E.decided(m, s)
            if not bool(bad.any()):
                break
            mags = torch.where(bad, mags * 1.5 + 1e-3, mags)
        else:
            raise AssertionError("prepare_inputs did not converge")
    return mix.contiguous(), mags.contiguous()


def warp_inputs(row):
    return _randn(gen(row), row["BC"], row["Hin"], row["Win"])


def innerprod_inputs(row):
    """(img [B, K] or imgs [B, K, P], snd [B, K, HW], scale [K] | None, bias [1] | None, dz [B, HW])."""
    g = gen(row)
    B, Kc, HW = row["B"], row["K"], row["HW"]
    img = _randn(g, B, Kc, row["P"]) if "P" in row else _randn(g, B, Kc)
    snd = _randn(g, B, Kc, HW)
    scale = (_rand(g, Kc) + 0.5) * (torch.randint(0, 2, (Kc,), generator=g) * 2 - 1).float() if row["scale"] else None
    bias = _randn(g, 1) if row.get("bias", True) else None
    return img, snd, scale, bias, _randn(g, B, HW)


def sdr_inputs(row):
    """(est, ref) [R, L] views of [R, L + pad] buffers."""
    g = gen(row)
    R_, L, pad = row["R"], row["L"], row["pad"]
    return _randn(g, R_, L + pad)[:, :L], (_randn(g, R_, L + 2 * pad) * 0.7)[:, :L]


def _fusion_draw(row, g, C, Ka, D, special):
    B, Dc, HW, FT, att = row["B"], D // Ka if "Dc" not in row else row["Dc"], row["HW"], row["FT"], row["att"]
    x = _randn(g, B, D, FT)
    vs = [_randn(g, B, Dc, HW) * row["vscale"] for _ in range(C)]
    h1, h2 = (HW // 3, HW // 3 + 5) if HW > 8 else (0, 0)
    if special == "zero_a":
        x[:, Dc:2 * Dc] = 0.0
    if special == "zero_v":
        vs[0][:, :, h1] = 0.0
    if special == "zero_channel":
        vs[0][:, 1] = 0.0
    if special == "equal_maps":
        vs = [vs[0]] + [vs[0].clone() for _ in range(C - 1)]
    a0 = x.amax(2)[:, :Dc]                                  # the pooled audio block 0
    if special == "tie_cols":                               # cos(a_0, column) == 1, the same bits at h1 and h2
        vs[0][:, :, h1] = a0 * 0.25
        vs[0][:, :, h2] = a0 * 0.25
    if special == "zero_sel":                               # every cosine negative but at one zero position
        x = x.abs()
        vs[0] = -vs[0].abs() - 0.01
        vs[0][:, :, h1] = 0.0
    return x, vs


def _undecided(f):
    return any(not bool(E.decided(m, s).all()) for m, s in f.margins.values())


def fusion_av_inputs(row):
    """(x [B, 2 Dc, FT], vs (one map for MixVis, else two), dfeat [B, 2 Dc], dmaps [B, 2, HW] | None, dmatch [1] | None, prefill
    of dx): the first seed whose decisions are all decidable."""
    kind = row["kind"]
    for salt in range(8):
        g = gen(row, str(salt))
        x, vs = _fusion_draw(row, g, 1 if kind == 2 else 2, 2, 2 * row["Dc"], row["special"])
        if not _undecided(E.fusion_fwd(x, vs, kind, row["att"])):
            B, D, HW = row["B"], 2 * row["Dc"], row["HW"]
            return (x, vs, _randn(g, B, D), _randn(g, B, 2, HW) if row["dmaps"] else None, _randn(g, 1) if row["dmatch"] else None,
                    _randn(g, B, D, row["FT"]))
    raise AssertionError(f"no decidable draw for {row['id']}")


def fusion_n_inputs(row):
    """(x [B, D, FT], vs C maps [B, D // C, HW], dfeat [B, D], dmatch [1] | None, prefill of dx)."""
    C, D = row["C"], row["D"]
    for salt in range(8):
        g = gen(row, str(salt))
        r = dict(row, Dc=D // C)
        x, vs = _fusion_draw(r, g, C, C, D, row["special"])
        if not _undecided(E.fusion_fwd(x, vs, 0, row["att"])):
            return x, vs, _randn(g, row["B"], D), _randn(g, 1) if row["dmatch"] else None, _randn(g, row["B"], D, row["FT"])
    raise AssertionError(f"no decidable draw for {row['id']}")


def fusion_ao_inputs(row):
    """(x [B, D, FT], draws, dfeat [B, D], prefill of dx)."""
    g = gen(row)
    if row["op"] == "fusion_ao":
        B, D = row["B"], 2 * row["Dc"]
        draws = torch.tensor(row["draws"], dtype=torch.uint8)
    else:
        B, D = row["B"], row["D"]
        draws = torch.arange(B, dtype=torch.int32)
    return _randn(g, B, D, row["FT"]), draws, _randn(g, B, D), _randn(g, B, D, row["FT"])


def attention_inputs(row):
    """(a [B, S, K], mix [B, K, HW], dctx [B, S, K], dmaps | None, dmatch [B] | None) with the clamp decidable."""
    B, S, Kc, HW = row["B"], row["S"], row["K"], row["HW"]
    for salt in range(8):
        g = gen(row, str(salt))
        a, mix = _randn(g, B, S, Kc), _randn(g, B, Kc, HW)
        if row["special"] == "zero_a":
            a[:, 1] = 0.0
        if row["special"] == "zero_v":
            mix[:, :, HW // 2] = 0.0
        if not _undecided(E.attention_fwd(a, mix, row["att"])):
            return a, mix, _randn(g, B, S, Kc), _randn(g, B, S, HW) if row["dmaps"] else None, _randn(g, B) if row["dmatch"] else None
    raise AssertionError(f"no decidable draw for {row['id']}")


def largest_tensor(row):
    """Elements of the largest tensor of a row."""
    r = row
    return {"mask_loss": lambda: r["B"] * r["S"] * r["S"] * r["FT"],
            "prepare": lambda: r["S"] * r["B"] * max(r["Fin"], r["Fout"]) * r["T"],
            "warp": lambda: r["BC"] * max(r["Hin"] * r["Win"], r["Hout"] * r["Wout"]),
            "innerprod_fwd": lambda: r["B"] * r["K"] * r["HW"], "innerprod_bwd": lambda: r["B"] * r["K"] * r["HW"],
            "innerprod_nosum": lambda: r["B"] * r["K"] * r["HW"],
            "innerprod_pixelwise": lambda: r["B"] * max(r["K"], r["P"]) * r["HW"],
            "sdr_sums": lambda: r["R"] * (r["L"] + 2 * r["pad"]),
            "fusion_av": lambda: r["B"] * r["Dc"] * max(2 * r["FT"], r["HW"]), "fusion_ao": lambda: r["B"] * 2 * r["Dc"] * r["FT"],
            "fusion_n_av": lambda: r["B"] * max(r["D"] * r["FT"], r["D"] // r["C"] * r["HW"], r["C"] * r["C"] * r["HW"]),
            "fusion_n_ao": lambda: r["B"] * r["D"] * r["FT"],
            "attention": lambda: r["B"] * max(r["S"], r["K"]) * r["HW"]}[r["op"]]()


# ---- what a row must give: name -> (ref, absref, k, unit); "=name" -> an integer output that must be equal --------------------
def _to(dev, *ts):
    return [None if t is None else ([u.to(dev) for u in t] if isinstance(t, (list, tuple)) else t.to(dev)) for t in ts]


def expected(row, inp, dev="cpu", pred=None):
    """The references of every output of a row on `dev`.  `pred`: the kernel's own activated predictions for the staged loss
    sums (the host tests pass none: the float64 activation rounded to fp32 stands in).  Values are (ref, absref, k, unit);
    names starting with "=" are integer outputs; "excluded:<name>" is a mask of elements the gate may skip."""
    U, op = E.U, row["op"]
    if op == "mask_loss":
        logits, gt, weight, coef = _to(dev, *inp)
        act, loss = A[row["act"]], Ls[row["loss"]]
        p, pu = E.activation(logits, act)
        out = {"pred": (p, pu, E.K["mask_loss.pred"], U)}
        s, su = E.mask_loss_sums(p.float() if pred is None else pred, gt, weight, loss)
        out["sums"] = (s, su, E.K["mask_loss.sums"], U)
        if not row.get("fwd_only"):
            g, gu, _ = E.mask_loss_bwd(logits, gt, weight, coef, act, loss)
            out["dlogits"] = (g, gu, 1, U)
        return out
    if op == "prepare":
        mix, mags = _to(dev, *inp)
        r = E.prepare(mix, mags, row["warp"], row["weighted"], row["binary"], row["Fout"])
        out = {n: (r[n][0], r[n][1], E.K["prepare"], U) for n in ("mag_mix", "mags", "log_mag_mix", "weight", "gt")}
        if row["binary"]:
            m, s = r["gt_margin"]
            out["excluded:gt"] = m <= U * s          # only what the reference itself proves undecidable
        return out
    if op == "warp":
        (x,) = _to(dev, inp)
        ref, units = E.warp(x, row["Hout"], row["Wout"], row["warp"])
        return {"y": (ref, units, E.K["warp"], U)}
    if op in ("innerprod_fwd", "innerprod_nosum", "innerprod_pixelwise"):
        img, snd, scale, bias, _ = _to(dev, *inp)
        fn = {"innerprod_fwd": E.innerprod_fwd, "innerprod_nosum": E.innerprod_nosum, "innerprod_pixelwise": E.innerprod_pixelwise}[op]
        k = E.K[op](row["K"]) if op != "innerprod_nosum" else E.K[op]
        return {"z": (*fn(img, snd, scale, bias), k, U)}
    if op == "innerprod_bwd":
        img, snd, scale, _, dz = _to(dev, *inp)
        r = E.innerprod_bwd(img, snd, scale, dz)
        HW, B = row["HW"], row["B"]
        out = {"r": (*r["r"], E.K["innerprod_bwd.r"](HW), U), "dimg": (*r["dimg"], E.K["innerprod_bwd.dimg"](HW), U),
               "dbias": (*r["dbias"], E.K["innerprod_bwd.dbias"], U)}
        if row["dsnd"]:
            out["dsnd"] = (*r["dsnd"], E.K["innerprod_bwd.dsnd"], U)
        if row["scale"]:
            out["dscale"] = (*r["dscale"], E.K["innerprod_bwd.dscale"](HW, B), U)
        return out
    if op == "sdr_sums":
        ref, a = E.sdr_sums(*inp)
        return {"sums": (ref.to(dev), a.to(dev), E.K["sdr_sums"](row["L"]), 2.0 ** -53)}
    if op in ("fusion_av", "fusion_n_av"):
        if op == "fusion_av":
            x, vs, dfeat, dmaps, dmatch, prefill = _to(dev, *inp)
            kind, C, B = row["kind"], 2, row["B"]
            Dc, HW, att = row["Dc"], row["HW"], row["att"]
            kb = E.K["fusion_av_bwd"](Dc, HW, att)
            km = E.K["fusion_av.match"](Dc, HW, att, kind)
        else:
            x, vs, dfeat, dmatch, prefill = _to(dev, *inp)
            dmaps, kind, C, B = None, 0, row["C"], row["B"]
            Dc, HW, att = row["D"] // C, row["HW"], row["att"]
            kb = E.K["fusion_n_av_bwd"](Dc, HW, att, C)
            km = E.K["fusion_n.match"](Dc, att, C)
        f = E.fusion_fwd(x, vs, kind, att, grad=True)
        kmap = E.K["fusion.maps"](Dc, att)
        out = {"a_pool": (f.a_pool.detach(), f.a_pool.detach().abs(), 0, U), "=pool_idx": f.pool_idx, "=sel_idx": f.sel, "=best": f.best,
               "att_maps": (f.att_maps.detach(), f.att_mapsa, kmap, U), "match_part": (f.match.detach(), f.matcha, km, U),
               "feat": (f.feat.detach(), f.feata, E.K["fusion.feat"](Dc, att, kind), U)}
        dm = (float(dmatch[0]) if dmatch is not None else 1.0) * E.f32(1.0 / B)
        g = E.fusion_bwd(f, dfeat, dmaps, dm)
        pre = E.take(prefill.to(E.F64), f.pool_idx)
        out["dx"] = (pre + g["dx"][0], pre.abs() / kb + g["dx"][1], kb, U)
        out["dv"] = (g["dv"][0], g["dv"][1], kb, U)
        return out
    if op in ("fusion_ao", "fusion_n_ao"):
        x, draws, dfeat, prefill = _to(dev, *inp)
        C = 2 if op == "fusion_ao" else row["C"]
        all_zero = op == "fusion_ao" and max(row["draws"]) == 0
        feat, pool_idx, src = E.fusion_ao(x, draws, C, all_zero)
        g, ga = E.fusion_ao_bwd(src, dfeat)
        pre = E.take(prefill.to(E.F64), pool_idx)
        return {"feat": (feat, feat.abs(), E.K["fusion_ao.feat"], U), "=pool_idx": pool_idx,
                "dx": (pre + g, pre.abs() + ga, E.K["fusion_ao.dx"], U)}
    if op == "attention":
        a, mix, dctx, dmaps, dmatch = _to(dev, *inp)
        S, Kc, HW, att = row["S"], row["K"], row["HW"], row["att"]
        f = E.attention_fwd(a, mix, att, grad=True)
        g = E.attention_bwd(f, dctx, dmaps, dmatch)
        kb = E.K["att_bwd"](Kc, HW, att, S)
        return {"maps_raw": (f.m.detach(), f.ma, E.K["att.maps"](Kc, att), U), "maps": (f.mc.detach(), f.ma, E.K["att.maps"](Kc, att), U),
                "match": (f.match.detach(), f.matcha, E.K["att.match"](Kc, HW, att, S), U),
                "ctx": (f.ctx.detach(), f.ctxa, E.K["att.ctx"](Kc, HW, att), U),
                "da": (*g["da"], kb, U), "dmix": (*g["dmix"], kb, U)}
    raise ValueError(op)


INPUTS = {"mask_loss": mask_loss_inputs, "prepare": prepare_inputs, "warp": warp_inputs, "innerprod_fwd": innerprod_inputs,
          "innerprod_bwd": innerprod_inputs, "innerprod_nosum": innerprod_inputs, "innerprod_pixelwise": innerprod_inputs,
          "sdr_sums": sdr_inputs, "fusion_av": fusion_av_inputs, "fusion_n_av": fusion_n_inputs, "fusion_ao": fusion_ao_inputs,
          "fusion_n_ao": fusion_ao_inputs, "attention": attention_inputs}
OPS = tuple(INPUTS)


def inputs(row):
    return INPUTS[row["op"]](row)
