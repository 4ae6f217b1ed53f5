"""Float64 reference of one `kernels.Conv` call, and an error gate that accounts for the conditioning of every element.

reference(cv, mode, operands) recomputes, in float64 with torch on the operands' device, what one call of Conv.fwd / dgrad /
dgrad_act / dgrad_up2x / wgrad must return (include/avsep.h semantics), together with `absref`: the same linear operation
applied to the absolute values of its operands — the sum of |term| behind every output element.  check(out, ref, absref, tau)
then asks |out - ref| <= tau * absref of EVERY element: unlike max|d| / max|ref| it sees a wrong small element (a border row,
a masked pixel) and it is not fooled by cancellation (the weight-gradient sums).

`cv` is a kernels.Conv or a Geometry (host tests): N, Cin, H, W, Cout, KH, KW, Ho, Wo and d.stride / pad / dil / C0 / act0 /
act1 / up2x.  `operands` is a dict:
  x0, x1, sc0, sh0, sc1, sh1   the sources of the virtual input (fp32 NCHW or B16 images [N, C/16, H, W, 16])
  w, bias                      OIHW fp32 weight (the tensor the call's packed image was built from) and bias (or None)
  dy                           the cotangent (dgrad*, wgrad)
  stats                        True: fwd accumulated the per-channel (sum y, sum y^2)
  bf16                         the call runs a bf16 kernel: operands rounded as the bf16 kernels stage them
  dgrad_act: y, scale, shift, residual, res_scale, res_shift, dz2, add, mean, invstd, act, bstats (bool)
  dgrad_up2x: mean1, invstd1, bstats1 (bool), g0_acc (the accumulated g0 BEFORE the call, or None)
  want_bias                    wgrad: dbias requested
"""
import types

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LRELU02 = 0, 1, 2
F64 = torch.float64
LRELU_SLOPE = float(torch.tensor(0.2, dtype=torch.float32))     # the kernels' 0.2f

# ---- the gate's tolerances, shared by test_gpu_benched_conv_calls.py (where they were measured) and test_gpu_conv_variants.py
WINOGRAD = ("wino4_kernel", "wino_kernel", "winow4_kernel", "winow_kernel")
CEIL_DIRECT, CEIL_WINO = 2e-5, 1.2e-4
# tau per (family, precision): 4x the measured worst ratio, at most the ceiling; families not listed take their ceiling
TAU = {
    ("conv3x3_kernel", "f32"): 2.7e-6,       # fwd 6.52e-7, dgrad 6.26e-7
    ("convbf_kernel", "bf16"): CEIL_DIRECT,  # fwd 1.99e-5, dgrad 1.99e-5: B16 outputs, the half-ulp rounding term dominates
    ("head_fwd_kernel", "f32"): 3.9e-6,      # 9.55e-7
    ("head_fwd_kernel", "bf16"): 3.9e-6,     # 9.68e-7
    ("head_dgrad_kernel", "f32"): CEIL_DIRECT,   # dgrad_up2x 1.86e-5
    ("head_dgrad_kernel", "bf16"): CEIL_DIRECT,  # dgrad_up2x 1.86e-5
    ("head_wgrad_kernel", "f32"): 3.8e-6,    # 9.46e-7
    ("head_wgrad_kernel", "bf16"): 3.8e-6,   # 9.31e-7
    ("igemm_kernel<fwd>", "f32"): 1.7e-6,    # 4.14e-7
    ("igemm_kernel<fwd>", "bf16"): 1.7e-6,   # 4.23e-7
    ("igemm_kernel<dgrad>", "f32"): 8.0e-6,  # 1.98e-6
    ("igemm_kernel<dgrad>", "bf16"): 7.1e-6, # 1.75e-6
    ("igemm_kernel<wgrad>", "f32"): 4.4e-6,  # 1.10e-6
    ("igemm_kernel<wgrad>", "bf16"): 6.6e-8, # 1.64e-8
    ("smallci_dgrad", "f32"): 2.1e-6,        # 5.23e-7
    ("smallci_dgrad", "bf16"): 2.2e-6,       # 5.33e-7
    ("smallci_wgrad_kernel", "f32"): 6.5e-8, # 1.61e-8
    ("wgrad3x3_kernel", "f32"): 1.2e-7,      # 2.80e-8
    ("wgrad3x3_kernel", "bf16"): 2.5e-6,     # 6.18e-7
    ("wgrad4d_kernel", "f32"): 1.9e-6,       # 4.76e-7
    ("wgrad4d_kernel", "bf16"): 1.5e-6,      # 3.61e-7
    ("wgradb_kernel", "bf16"): 4.2e-6,       # 1.04e-6
    ("wino4_kernel", "f32"): 7.3e-5,         # fwd 3.42e-6, dgrad 1.64e-5, dgrad_act 1.80e-5 (tile absref)
    ("wino_kernel", "f32"): 6.2e-7,          # fwd 1.41e-7, dgrad 1.54e-7 (tile absref)
    ("winow4_kernel", "f32"): 5.7e-5,        # wgrad 1.41e-5 (tile absref)
}


def tau_of(family, prec):
    return TAU.get((family, prec), CEIL_WINO if family in WINOGRAD else CEIL_DIRECT)


# Per (variant string, precision) entries of the variant gate (test_gpu_conv_variants.py) alone; the benched gate keeps TAU.
# Same rule: 4x the measured worst ratio, at most the ceiling.  Both are N = 1 weight gradients that sum a few hundred
# products in an fp32 MFMA accumulator.  Their benched entries were measured on sums of 10^4 ... 10^6 terms of either sign,
# where |ref| << absref and the roundings of the partial sums average out; over a short sum an element whose terms mostly
# share a sign has |ref| ~ absref, and ONE rounding of an fp32 result of that size is already 2^-24 = 5.96e-8 of absref, which
# is 0.9 / 0.5 of the two benched values.  The misses were 1.5 and 2.4 times 2^-24 at elements of |ref| = 0.17 absref (6 and 13
# ulps of the result, i.e. 0.8 and 1.6 ulps at the partial sums' size), and the same kernel on the same operands sits at
# 7.4e-8 / 1.7e-7 under the other precision's entry: rounding.  A dropped or misplaced term would be ~absref / K = 1e-3.
VARIANT_TAU = {
    ("igemm_kernel<wgrad>", "bf16"): 3.6e-7,   # 8.86e-8: layer2.1x1s2 at N = 1 (K = 784), f32 kernel under AVSEP_ALGO_NO_BF16_KERNELS
    ("wgrad3x3_kernel", "f32"): 5.8e-7,        # 1.44e-7: ragged18x30 at N = 1 (K = 540)
}


def tau_of_variant(variant, prec):
    return VARIANT_TAU.get((variant, prec), tau_of(variant.split(":")[0], prec))


class Geometry:
    """The geometry a Conv descriptor carries, for host tests that cannot build a kernels.Conv."""

    def __init__(self, N, Cin, H, W, Cout, k, stride=1, pad=0, dil=1, C0=None, act0=0, act1=0, up2x=False):
        kh, kw = (k, k) if isinstance(k, int) else k
        self.N, self.Cin, self.H, self.W, self.Cout, self.KH, self.KW = N, Cin, H, W, Cout, kh, kw
        self.Ho = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1
        self.Wo = (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
        self.d = types.SimpleNamespace(stride=stride, pad=pad, dil=dil, C0=Cin if C0 is None else C0, act0=act0, act1=act1,
                                       up2x=int(up2x))


def nchw(t):
    """fp32 NCHW view of an activation in either storage format (B16 -> fp32 is exact)."""
    if t is None:
        return None
    if t.dtype == torch.bfloat16:
        N, CB, H, W, _ = t.shape
        return t.float().permute(0, 1, 4, 2, 3).reshape(N, CB * 16, H, W)
    return t.float()


def bf16(t):
    """Round to bfloat16 (nearest even), returned in the input's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def fmaf(a, s, h):
    """fp32 fmaf(a, s, h) per channel: the float64 product is exact, the sum is rounded once to float32."""
    return (a.to(F64) * s.to(F64).view(1, -1, 1, 1) + h.to(F64).view(1, -1, 1, 1)).float()


def act_fwd(v, act):
    """The kernels' activation on fp32 values (fmaxf(v, slope * v))."""
    if act == ACT_RELU:
        return torch.clamp_min(v, 0.0)
    if act == ACT_LRELU02:
        return torch.where(v > 0, v, v * torch.tensor(0.2, dtype=torch.float32))
    return v


def act_grad(pre, act):
    if act == ACT_RELU:
        return (pre > 0).to(F64)
    if act == ACT_LRELU02:
        return torch.where(pre > 0, 1.0, LRELU_SLOPE).to(F64)
    return torch.ones_like(pre, dtype=F64)


def up2x(v):
    return F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=True)


def up2x_adjoint(g, h, w):
    """Transpose of bilinear x2 (align_corners=True) from [.., 2h, 2w] back to [.., h, w]."""
    z = torch.zeros(g.shape[0], g.shape[1], h, w, dtype=g.dtype, device=g.device, requires_grad=True)
    with torch.enable_grad():
        out = up2x(z)
        return torch.autograd.grad(out, z, g)[0]


def _sources(cv, op):
    """The activated sources (fp32 values, as the kernel stages them) and their pre-activations."""
    d = cv.d
    out = []
    for i, (x, sc, sh, act) in enumerate(((op.get("x0"), op.get("sc0"), op.get("sh0"), d.act0),
                                          (op.get("x1"), op.get("sc1"), op.get("sh1"), d.act1))):
        if x is None:
            continue
        x = nchw(x)
        if op.get("bf16"):
            x = bf16(x)                                  # a bf16 kernel (and the grid pack) stages the B16 image of the source
        pre = fmaf(x, sc, sh) if sc is not None else x
        v = act_fwd(pre, act)
        if op.get("bf16"):
            v = bf16(v)                                  # ... and rounds the activated value on its way into LDS
        out.append((v, pre))
    return out


def virtual_input(cv, op, absolute=False):
    """The convolution's virtual input in float64: concat of act_i(sc_i * x_i + sh_i), bilinear x2 with up2x."""
    vs = [v.to(F64) for v, _ in _sources(cv, op)]
    v = torch.cat(vs, 1) if len(vs) > 1 else vs[0]
    if absolute:
        v = v.abs()
    return up2x(v) if cv.d.up2x else v


def _w(op):
    w = op["w"].to(F64)
    return bf16(w) if op.get("bf16") else w


def _dy(op):
    dy = nchw(op["dy"]).to(F64)
    return bf16(dy) if op.get("bf16") else dy


def _conv(cv, v, w, b=None):
    return F.conv2d(v, w, b, cv.d.stride, cv.d.pad, cv.d.dil)


def _conv_t(cv, dy, w):
    """Gradient wrt the [N, Cin, H, W] virtual input of conv(., w) given dy."""
    shape = (cv.N, cv.Cin, cv.H, cv.W)
    return torch.ops.aten.convolution_backward(dy, torch.empty(shape, dtype=F64, device=dy.device), w, None,
                                               [cv.d.stride] * 2, [cv.d.pad] * 2, [cv.d.dil] * 2, False, [0, 0], 1,
                                               [True, False, False])[0]


def _conv_w(cv, dy, v):
    return torch.ops.aten.convolution_backward(dy, v, torch.empty((cv.Cout, cv.Cin, cv.KH, cv.KW), dtype=F64, device=dy.device),
                                               None, [cv.d.stride] * 2, [cv.d.pad] * 2, [cv.d.dil] * 2, False, [0, 0], 1,
                                               [False, True, False])[1]


def _chan(t):
    return t.sum((0, 2, 3))


def reference(cv, mode, operands):
    """{name: (ref, absref)} of every output of the call, plus "excluded" (dgrad_act: elements whose activation mask is
    undecidable from the float64 model, as a bool tensor of dx's shape, or None) and, for statistics outputs, entries
    whose absref is the per-channel bound term (see check_stats)."""
    op = operands
    res = {}
    if mode == "fwd":
        v, w = virtual_input(cv, op), _w(op)
        b = op.get("bias")
        y = _conv(cv, v, w, b.to(F64) if b is not None else None)
        a = _conv(cv, virtual_input(cv, op, absolute=True), w.abs(), b.to(F64).abs() if b is not None else None)
        del v
        res["y"] = (y, a)
        if op.get("stats"):
            res["stats"] = (torch.cat([_chan(y), _chan(y * y)]), torch.cat([_chan(a), 2.0 * _chan(y.abs() * a)]))
        return res
    if mode == "wgrad":
        dy, v = _dy(op), virtual_input(cv, op)
        dw = _conv_w(cv, dy, v)
        del v
        dwa = _conv_w(cv, dy.abs(), virtual_input(cv, op, absolute=True))
        res["dw"] = (dw, dwa)
        if op.get("want_bias"):
            res["dbias"] = (_chan(dy), _chan(dy.abs()))
        return res
    dy, w = _dy(op), _w(op)
    g = _conv_t(cv, dy, w)
    ga = _conv_t(cv, dy.abs(), w.abs())
    del dy
    if mode == "dgrad":
        res["dx"] = (g, ga)
        return res
    if mode == "dgrad_act":
        y = op["y"].float()
        pre1 = fmaf(y, op["scale"], op["shift"]) if op.get("scale") is not None else y
        mag = pre1.abs().to(F64)
        pre = pre1
        if op.get("residual") is not None:
            r = op["residual"].float()
            pre2 = fmaf(r, op["res_scale"], op["res_shift"]) if op.get("res_scale") is not None else r
            pre = (pre1.to(F64) + pre2.to(F64)).float()
            mag = mag + pre2.abs().to(F64)
        # the kernel's own roundings of the pre-activation may differ from this model by an ulp of its terms: within 2 fp32
        # ulps of 0 the mask is undecidable, and those elements are left out of the check (check() counts them)
        excl = (pre.to(F64).abs() <= 2.0 * 2.0 ** -23 * mag) if op.get("act", 0) in (ACT_RELU, ACT_LRELU02) else None
        m = act_grad(pre, op.get("act", 0))
        if op.get("dz2") is not None:
            g, ga = g + op["dz2"].to(F64), ga + op["dz2"].to(F64).abs()
        dx, dxa = m * g, m * ga
        if op.get("add") is not None:
            dx, dxa = dx + op["add"].to(F64), dxa + op["add"].to(F64).abs()
        res["dx"] = (dx, dxa)
        res["excluded"] = excl
        if op.get("bstats"):
            xhat = (y.to(F64) - op["mean"].to(F64).view(1, -1, 1, 1)) * op["invstd"].to(F64).view(1, -1, 1, 1)
            bnd = dxa if excl is None else dxa + torch.where(excl, ga, 0.0)      # either mask value may have been summed
            res["bstats"] = (torch.cat([_chan(dx), _chan(dx * xhat)]), torch.cat([_chan(bnd), _chan(bnd * xhat.abs())]))
        return res
    if mode == "dgrad_up2x":
        srcs = _sources(cv, op)
        C0 = cv.d.C0
        hs, ws = cv.H // 2, cv.W // 2
        lo, loa = up2x_adjoint(g, hs, ws), up2x_adjoint(ga, hs, ws)
        del g, ga
        m0 = (srcs[0][1] > 0).to(F64)
        g0, g0a = m0 * lo[:, :C0], m0 * loa[:, :C0]
        if op.get("g0_acc") is not None:
            acc = op["g0_acc"].to(F64)
            g0, g0a = g0 + acc, g0a + acc.abs()
        res["g0"] = (g0, g0a)
        if len(srcs) > 1:
            m1 = (srcs[1][1] > 0).to(F64)
            g1, g1a = m1 * lo[:, C0:], m1 * loa[:, C0:]
            res["g1"] = (g1, g1a)
            if op.get("bstats1"):
                x1 = nchw(op["x1"]).to(F64)
                xhat = (x1 - op["mean1"].to(F64).view(1, -1, 1, 1)) * op["invstd1"].to(F64).view(1, -1, 1, 1)
                res["bstats1"] = (torch.cat([_chan(g1), _chan(g1 * xhat)]), torch.cat([_chan(g1a), _chan(g1a * xhat.abs())]))
        return res
    raise ValueError(mode)


def half_ulp_bf16(x):
    """Half a bfloat16 ulp at |x| (8 significand bits: 2^(e - 9) for |x| in [2^(e-1), 2^e))."""
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.ones_like(x), e - 9)


def tile_absref(absref):
    """Winograd absref.  A Winograd kernel mixes the elements of a transform tile (a 2x2 / 4x4 output tile; the 3x3 taps of a
    weight gradient), so its rounding error at one element scales with the terms of its whole tile, not with the element's
    own: where those vanish (a dY that is zero but for the max-pool's arg-max pixels, a silent spectrogram region) the
    direct-form absref is 0 or tiny while the tile's is not.  Max of absref over every tile an element can belong to."""
    if absref.shape[-1] <= 3 and absref.shape[-2] <= 3:       # OIHW weight gradient: the taps of one (co, ci)
        return absref.amax((-2, -1), keepdim=True).expand_as(absref)
    a = absref.reshape(-1, 1, *absref.shape[-2:])
    return F.max_pool2d(a, 7, 1, 3).reshape(absref.shape)


def check(out, ref, absref, tau, b16=False, excluded=None):
    """Worst |out - ref| / bound over all elements, bound = tau * absref (+ half a bf16 ulp for a B16 output); an element whose
    absref is 0 must equal ref exactly (its ratio is inf otherwise, 0 if equal).  Returns (ratio, flat index, ref, absref,
    number of excluded elements, out at that index)."""
    o = nchw(out).to(F64).reshape(ref.shape) if out.dtype == torch.bfloat16 else out.to(F64).reshape(ref.shape)
    err = (o - ref).abs()
    bound = tau * absref
    if b16:
        bound = bound + half_ulp_bf16(torch.maximum(ref.abs(), o.abs()))
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, 1.0), torch.where(err > 0, float("inf"), 0.0))
    r = torch.where(torch.isnan(o), float("inf"), r)
    nex = 0
    if excluded is not None:
        r = torch.where(excluded, 0.0, r)
        nex = int(excluded.sum())
    i = int(torch.argmax(r.reshape(-1)))
    return (float(r.reshape(-1)[i]), i, float(ref.reshape(-1)[i]), float(absref.reshape(-1)[i]), nex, float(o.reshape(-1)[i]))


def check_stats(out, ref, bound, tau):
    """The per-channel statistics sums: |out - ref| <= tau * bound, bound = sum absref (2 sum |ref| absref for sum y^2, sum
    absref |xhat| for the BatchNorm-backward sum)."""
    return check(out.to(F64), ref, bound, tau)
