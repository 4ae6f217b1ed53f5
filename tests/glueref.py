"""Float64 references of the glue kernels between the convolutions (csrc/ops.hip, csrc/b16.hip), one function per operation.

Every function is plain torch float64 on the device of its operands and calls nothing from the library.  It returns
(ref, absref) — or, for an operation with several outputs, a dict name -> (ref, absref) — where absref is the same formula
evaluated on the absolute values of its terms: the quantity a rounding error of the kernel scales with, element by element
(convref.check: |out - ref| <= tau * absref, plus half a bf16 ulp for a B16 output; convref.check_stats for the sums).

Contracts the references evaluate:
  - a B16 image ([N, C/16, H, W, 16] bfloat16) is taken at its bf16 values (convref.nchw is exact);
  - statistics are sums of the fp32 values BEFORE any rounding of the output to bf16 (csrc/b16.hip, line 5);
  - max-pool: the winner of a window is its FIRST maximum in (kh, kw) scan order over the fp32 activated values, which
    convref.fmaf / convref.act_fwd reproduce exactly; the float64 model of the same values (`exact=False`) is what a seed
    is checked against: both must name the same winner in every window.
"""
import torch
import torch.nn.functional as F

import convref as R
from recipes import f32, out_hw

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_LRELU02 = R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU02


def vals(t):
    """float64 NCHW values of an fp32 NCHW tensor or a B16 image."""
    return R.nchw(t).to(F64)


def _c(v):
    return v.to(F64).view(1, -1, 1, 1)


def b16_image(x):
    """The B16 image [N, C/16, H, W, 16] of an NCHW tensor (rounded to bf16, nearest even)."""
    N, Cc, H, W = x.shape
    return x.view(N, Cc // 16, 16, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def blocked_to_nchw(t):
    """[N, C/16, H, W, 16] of any dtype -> [N, C, H, W] (the winning-tap image of the B16 max-pool)."""
    N, CB, H, W, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(N, CB * 16, H, W)


def nchw_to_blocked(t):
    N, Cc, H, W = t.shape
    return t.view(N, Cc // 16, 16, H, W).permute(0, 1, 3, 4, 2).contiguous()


# ---- BatchNorm pieces ---------------------------------------------------------------------------------------------------------
def channel_stats(x):
    """(sum x, sum x^2) per channel, [2C]."""
    x = vals(x)
    q = (x * x).sum((0, 2, 3))
    return torch.cat([x.sum((0, 2, 3)), q]), torch.cat([x.abs().sum((0, 2, 3)), q])


def channel_sum(x):
    x = vals(x)
    return x.sum((0, 2, 3)), x.abs().sum((0, 2, 3))


def bn_bwd_apply(dz, y, pqr):
    """dy = p*dz + q*y + r per channel."""
    dz, y = vals(dz), vals(y)
    p, q, r = _c(pqr[0]), _c(pqr[1]), _c(pqr[2])
    return p * dz + q * y + r, p.abs() * dz.abs() + q.abs() * y.abs() + r.abs()


def pre_act(y, scale=None, shift=None, res=None, res_scale=None, res_shift=None):
    """The pre-activation scale*y + shift [+ res_scale*res + res_shift | + res] and the sum of its |terms|."""
    y = vals(y)
    if scale is not None:
        pre, a = y * _c(scale) + _c(shift), y.abs() * _c(scale).abs() + _c(shift).abs()
    else:
        pre, a = y, y.abs()
    if res is not None:
        r = vals(res)
        if res_scale is not None:
            pre, a = pre + (r * _c(res_scale) + _c(res_shift)), a + r.abs() * _c(res_scale).abs() + _c(res_shift).abs()
        else:
            pre, a = pre + r, a + r.abs()
    return pre, a


def _neg_slope(act):
    return {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU02: R.LRELU_SLOPE}[act]


def undecidable(pre, a):
    """Elements whose activation mask a kernel's own roundings may decide either way: |pre| within 2^-20 of the sum of its
    |terms| of zero.  The tests move these away (make_decidable) instead of excluding them."""
    return pre.abs() <= 2.0 ** -20 * a


def make_decidable(y, pre_fn, requant=None):
    """Add 1 to every element of `y` (fp32 NCHW, on the CPU) whose pre-activation pre_fn(y) -> (pre, a) is undecidable, until
    none is left.  `requant` re-rounds the changed tensor (bf16 inputs).  Returns (y, number of elements moved)."""
    moved = 0
    for _ in range(8):
        bad = undecidable(*pre_fn(y))
        n = int(bad.sum())
        if n == 0:
            return y, moved
        moved += n
        y = torch.where(bad, y + 1.0, y)
        if requant is not None:
            y = requant(y)
    raise AssertionError("make_decidable did not converge")


def affine_act(y, scale, shift, res, res_scale, res_shift, act):
    """z = act(pre).  absref is that of pre for both signs (act is continuous and |act'| <= 1)."""
    pre, a = pre_act(y, scale, shift, res, res_scale, res_shift)
    return torch.where(pre > 0, pre, pre * _neg_slope(act)), a


def affine_act_bwd(dz, dz2, y, scale, shift, res, res_scale, res_shift, add, mean, invstd, act):
    """g = act'(pre) * (dz [+ dz2]) [+ add];  bstats = (sum g, sum g * (y - mean) * invstd) per channel, [2C]."""
    pre, a = pre_act(y, scale, shift, res, res_scale, res_shift)
    m = torch.where(pre > 0, 1.0, _neg_slope(act)).to(F64)
    d, da = vals(dz), vals(dz).abs()
    if dz2 is not None:
        d, da = d + vals(dz2), da + vals(dz2).abs()
    g, ga = m * d, m * da
    if add is not None:
        g, ga = g + vals(add), ga + vals(add).abs()
    out = {"g": (g, ga), "undecidable": undecidable(pre, a) if act != ACT_NONE else torch.zeros_like(pre, dtype=torch.bool)}
    if mean is not None:
        xhat = (vals(y) - _c(mean)) * _c(invstd)
        out["bstats"] = (torch.cat([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))]),
                         torch.cat([ga.sum((0, 2, 3)), (ga * xhat.abs()).sum((0, 2, 3))]))
    return out


# ---- max-pool 3x3 / stride 2 / pad 1 over act(scale*x + shift) -------------------------------------------------------------------
def pool_values(x, scale, shift, act, exact=True):
    """The activated values the pooling compares.  exact: the kernel's fp32 values (one fmaf rounding, fp32 slope product),
    returned as float64; else their float64 model."""
    if exact:
        x32 = R.nchw(x)
        pre = R.fmaf(x32, scale, shift) if scale is not None else x32
        return R.act_fwd(pre, act).to(F64)
    pre, _ = pre_act(x, scale, shift)
    return torch.where(pre > 0, pre, pre * _neg_slope(act))


def _scan(v):
    """First maximum of every 3x3/s2/p1 window in (kh, kw) scan order: (best, tap = kh*3+kw)."""
    N, Cc, H, W = v.shape
    Ho, Wo = out_hw(H), out_hw(W)
    pad = F.pad(v, (1, 1, 1, 1), value=float("-inf"))
    best = torch.full((N, Cc, Ho, Wo), float("-inf"), dtype=v.dtype, device=v.device)
    tap = torch.full((N, Cc, Ho, Wo), -1, dtype=torch.int64, device=v.device)
    for kh in range(3):
        for kw in range(3):
            cand = pad[:, :, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
            upd = torch.isfinite(cand) & ((cand > best) | (tap < 0))
            best = torch.where(upd, cand, best)
            tap = torch.where(upd, kh * 3 + kw, tap)
    return best, tap


def taps_to_flat(tap, H, W):
    """Winning tap (kh*3+kw) of window (ho, wo) -> flat position h*W + w inside the input plane."""
    Ho, Wo = tap.shape[-2:]
    ho = torch.arange(Ho, device=tap.device).view(1, 1, -1, 1)
    wo = torch.arange(Wo, device=tap.device).view(1, 1, 1, -1)
    t = tap.long()
    return (2 * ho - 1 + t // 3) * W + (2 * wo - 1 + t % 3)


def maxpool(x, scale, shift, act, exact=True):
    """{"y": (pooled, absref), "tap": winning taps, "idx": flat winner positions}.  absref: |terms| of the winner."""
    v = pool_values(x, scale, shift, act, exact)
    N, Cc, H, W = v.shape
    best, tap = _scan(v)
    idx = taps_to_flat(tap, H, W)
    _, a = pre_act(x, scale, shift)
    aw = a.reshape(N, Cc, H * W).gather(2, idx.reshape(N, Cc, -1)).reshape(best.shape)
    return {"y": (best, aw), "tap": tap, "idx": idx}


def _scatter(g, idx, H, W):
    N, Cc = g.shape[:2]
    out = torch.zeros((N, Cc, H * W), dtype=F64, device=g.device)
    out.scatter_add_(2, idx.reshape(N, Cc, -1).long(), g.reshape(N, Cc, -1))
    return out.view(N, Cc, H, W)


def maxpool_bwd(dy, idx, H, W):
    """dx[pos] = sum of dy over the windows whose winner is pos."""
    dy = vals(dy)
    return _scatter(dy, idx, H, W), _scatter(dy.abs(), idx, H, W)


def stem_tail_bwd(g, g2, idx, y, scale, shift, mean, invstd, pqr):
    """The fused stem-tail backward: dz[pos] = [scale*y+shift > 0] * sum of g (+ g2) over the windows that chose pos;
    bstats = (sum dz, sum dz * xhat) taken over the pooled grid;  dy = p*dz + q*y + r."""
    yv = vals(y)
    N, Cc, H, W = yv.shape
    pre, a = pre_act(y, scale, shift)
    m = (pre > 0).to(F64)
    gg, gga = vals(g), vals(g).abs()
    if g2 is not None:
        gg, gga = gg + vals(g2), gga + vals(g2).abs()
    flat = idx.reshape(N, Cc, -1).long()
    out = {"undecidable": undecidable(pre, a)}
    if mean is not None:
        mw = m.reshape(N, Cc, -1).gather(2, flat).reshape(gg.shape)
        xw = ((yv - _c(mean)) * _c(invstd)).reshape(N, Cc, -1).gather(2, flat).reshape(gg.shape)
        out["bstats"] = (torch.cat([(mw * gg).sum((0, 2, 3)), (mw * gg * xw).sum((0, 2, 3))]),
                         torch.cat([(mw * gga).sum((0, 2, 3)), (mw * gga * xw.abs()).sum((0, 2, 3))]))
    if pqr is not None:
        p, q, r = _c(pqr[0]), _c(pqr[1]), _c(pqr[2])
        dz, dza = m * _scatter(gg, idx, H, W), m * _scatter(gga, idx, H, W)
        out["dy"] = (p * dz + q * yv + r, p.abs() * dza + q.abs() * yv.abs() + r.abs())
    return out


# ---- temporal mean, SGD, space-to-depth, conversions ---------------------------------------------------------------------------
def temporal_mean(x, B, T):
    x = x.to(F64).reshape(B, T, -1)
    return x.sum(1) / T, x.abs().sum(1) / T


def temporal_mean_bwd(dy, B, T):
    d = dy.to(F64).reshape(B, 1, -1).expand(B, T, -1) / T
    return d, d.abs()


def sgd(p, g, buf, lr, momentum, weight_decay, grad_scale, first):
    """torch.optim.SGD's step on the fp32 values of the scalars: {"buf": ..., "p": ...}."""
    lr, momentum, weight_decay, grad_scale = f32(lr), f32(momentum), f32(weight_decay), f32(grad_scale)
    p, g, buf = p.to(F64), g.to(F64), buf.to(F64)
    d, da = weight_decay * p + g * grad_scale, abs(weight_decay) * p.abs() + g.abs() * abs(grad_scale)
    b, ba = (d, da) if first else (momentum * buf + d, abs(momentum) * buf.abs() + da)
    return {"buf": (b, ba), "p": (p - lr * b, p.abs() + abs(lr) * ba)}


def space_to_depth2(x, cp):
    """xs[n][(dy*2+dx)*C + c][i+2][j+2] = x[n][c][2i+dy][2j+dx], zero elsewhere; [N, cp, H/2+3, W/2+3]."""
    x = x.to(F64)
    N, Cc, H, W = x.shape
    xs = torch.zeros((N, cp, H // 2 + 3, W // 2 + 3), dtype=F64, device=x.device)
    for dy in range(2):
        for dx in range(2):
            k = (dy * 2 + dx) * Cc
            xs[:, k:k + Cc, 2:2 + H // 2, 2:2 + W // 2] = x[:, :, dy::2, dx::2]
    return xs, xs.abs()


def identity(x):
    """Conversions: the values themselves (a B16 output adds half a bf16 ulp in the gate, tau = 0)."""
    v = vals(x)
    return v, v.abs()


def truncate_bf16(ref):
    """fp32(ref) with the low 16 bits cut off instead of rounded to nearest even: the defect the B16 gates must reject."""
    bits = ref.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(F64)
