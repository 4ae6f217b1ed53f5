"""Float64 references of the kernels at the two ends of the train step: spectrogram preparation (csrc/ops.hip avsep_prepare,
avsep_warp), the bottleneck (csrc/fusion.hip, csrc/fusion_n.hip, csrc/attention.hip), the mask synthesizer
(avsep_innerprod_*), and the loss (avsep_mask_loss_*, avsep_sdr_sums).  One function per launcher, plain torch float64 on the
device of its operands; nothing here calls the library.

Every function returns, per output, (ref, absref): absref is the same formula on the absolute values of its terms, the
quantity a rounding error of the kernel scales with.  The gate is |out - ref| <= k * 2^-24 * absref, an element whose absref is
0 must equal ref exactly (convref.check); k, per launcher, is K below.

Composed formulas carry first-order terms.  An intermediate t that the kernel holds in fp32 with an error of k_t * 2^-24 * ta
(ta: the absref of t) reaches the output through |d out / d t|; the references fold that in by using ta wherever |t| appears
downstream and adding k_t to the k of everything downstream.  Where this would be loose by more than the conditioning of the
formula itself — the activation inside the mask loss's gradient, the sampling position inside the bilinear warp — the
reference returns the bound in units of 2^-24 directly (`units`: already multiplied by the k of each path) and the gate
uses k = 1.

expf, logf, log1pf, tanhf, sqrtf and the fp32 division are allowed FN = 4 units (2 ulp) each: this ROCm ships no accuracy
table of the HIP math functions, so 2 ulp is ASSUMED, as the documentation of the OCML functions states for most of them.

Discrete decisions (arg-max positions, the best permutation, the binary mask, clamp masks, the L1 sign) come with their
margins: the test rows must make every decision decidable (`decided`), except exact ties that the row constructs from
bitwise equal operands, which kernel and reference both resolve to the first index.
"""
import itertools
import math

import torch

from recipes import cdiv, f32

F64 = torch.float64
U = 2.0 ** -24
FN = 4
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_SOFTMAX = 0, 1, 3, 4, 5
BCE, L1, L2 = 0, 1, 2


EPS_COS = f32(1e-8)           # FUS_EPS, FN_EPS, ATT_EPS
EPS_MIX = f32(1e-10)
BCE_FLOOR = f32(1e-12)


# k per launcher: the fp32 roundings on the longest path (a math function: FN), with the source lines they were counted from
# and the worst ratio |err| / bound measured on an MI355X per form (tests/test_gpu_step_ends.py prints them).
def k_maps(Dc, att):
    """A similarity map.  cos: `d0 = fmaf(s_a[d], vv, d0)` Dc roundings on sum |a v|; `nv = fmaf(vv, vv, nv)` and the audio norm,
    Dc roundings and a sqrtf each, which halves them: Dc + FN for the two; the product of the norms 1; the division FN.
    sig: the dot product Dc, `1.f / sqrtf(Dc)` 2 FN, `-d0 * inv_sqrt` 1 — all on m(1 - m) sum |a v| / sqrt(Dc) — and expf FN,
    `1.f +` 1, the division FN on m."""
    return (2 * Dc + 2 * FN + 1) if att == 0 else (Dc + 2 * FN + 1)


K = {
    # ops.hip mask_loss_fwd_kernel -> activate_vec; `pred`: the bound is in units (activation()), k = 1
    "mask_loss.pred": 1,           # measured: sigmoid 0.30, tanh 0.52, softmax 0.51, none / relu exact
    # ... `acc[ti * MAXS + pj] += w * loss_elem(p[pj], t[ti], loss)`: units (mask_loss_sums), k = 1
    "mask_loss.sums": 1,           # measured: 0.12 at most
    # ops.hip mask_loss_bwd_kernel: loss_grad `(p - t) / fmaxf((1.f - p) * p, 1e-12f)` 1 + 2 + FN = 7, `c * w[ti] * loss_grad` 2,
    # `s +=` S - 1 = 3, the slope `p[s] * (1.f - p[s])` 2, `g[s] * d` 1: 15; softmax `dot += g[s] * p[s]` 2 S = 8 in place of the
    # slope, `p[s] * (g[s] - dot)` 2: 22.  The activation's own error enters through units (mask_loss_bwd).
    "mask_loss_bwd": lambda act: 22 if act == ACT_SOFTMAX else 15,    # measured: worst per form over all three outputs 0.16 none, 0.09 relu, 0.30 sigmoid, 0.52 tanh, 0.51 softmax (dlogits alone: 0.29 at most)
    # ops.hip prepare_kernel / warp_kernel through warp_coords.h: units (bilinear(), prepare()), k = 1; the 9 roundings of
    # sample_bilin are K_BILIN below
    "prepare": 1,                  # measured: warp 0.41 (binary, 30 elements excluded), 0.16 (ratio); no warp 0.58, 0.99 (mix + 1e-10f: one rounding)
    "warp": 1,                     # measured: un-warp 256 -> 512 0.28, warp 512 -> 256 0.30
    # ops.hip innerprod_kernel `s_w[k] = img * scale` 1, `s = fmaf(s_w[k], snd, s)` K, `s + bs` 1
    "innerprod_fwd": lambda Kc: Kc + 2,    # measured: gemv 0.46
    # ops.hip innerprod_bwd_kernel `w = img * scale`, `op[i] = w * d`
    "innerprod_bwd.dsnd": 2,       # measured: 0.85
    # ... `acc = fmaf(sp[i], d, acc)` ceil(HW / 256) per thread, wave_sum 6 levels, `sh[0] + sh[1] + sh[2] + sh[3]` 3
    "innerprod_bwd.r": lambda HW: cdiv(HW, 256) + 9,    # measured: 0.06 at most over r, dimg, dscale and dbias
    # models/synthesizer_net.py _InnerProdFn.backward `r * scale` 1 more; `(img * r).sum(0)` 1 + B more; `dz.sum()` is a torch
    # reduction, not a kernel of the project: 64 covers its per-thread partial sums and tree
    "innerprod_bwd.dimg": lambda HW: cdiv(HW, 256) + 10,    # measured: see r
    "innerprod_bwd.dscale": lambda HW, B: cdiv(HW, 256) + 10 + B,    # measured: see r
    "innerprod_bwd.dbias": 64,     # measured: see r
    # ops.hip innerprod_nosum_kernel `w = img * scale`, `fmaf(w, v.x, bs)`
    "innerprod_nosum": 2,          # measured: vec4 0.59, scalar 0.65
    # ops.hip innerprod_pixelwise_kernel `imgs * scale` 1, v_mfma_f32_32x32x2_f32 over K / 2 steps: a product and an addition
    # per k (the instruction's internal rounding is not documented: both counted), `acc[r] + bs` 1
    "innerprod_pixelwise": lambda Kc: 2 * Kc + 2,    # measured: mfma 0.26, with the LDS opt-in (K = 128) 0.01
    # ops.hip sdr_sums_kernel: fp64 throughout, in units of 2^-53: `a += x * y` ceil(L / (gx * 256)) per thread (the products of
    # two fp32 values are exact), wave_sum_d 6, the sum of four 3, one atomicAdd per workgroup gx
    "sdr_sums": lambda L: cdiv(L, min(cdiv(L, 2048), 64) * 256) + 9 + min(cdiv(L, 2048), 64),    # measured: dense rows 0.12, strided rows 0.06
    # fusion.hip fusion_maps / fusion_n.hip fn_maps / attention.hip: k_maps above
    "fusion.maps": k_maps,         # measured (worst of all forward outputs): fusion_av 0.14 cos, 0.16 sig, MixVis 0.19; fusion_n 0.11 cos, 0.13 sig
    # fusion.hip fusion_av_fwd_kernel `p0 = s_mx[0] + s_mx[3]`, `p0 - p1`: 2 on top of the maps; MixVis: mixvis_sums
    # `sm += s_m[..] + s_m[..]` 2 ceil(HW / 256), block_sum4 6 + 3, `/ (float)HW` FN, the cosine of the selected vectors
    # ceil(Dc / 256) + 9 per sum, 2 sqrtf, product, division: 3 FN + 1, the two additions 2
    # fusion_n.hip: `s += l.mx[..]` C, `others += sc[p]` C! - 1, `others - sbest` 1
    "fusion_av.match": lambda Dc, HW, att, kind: k_maps(Dc, att) + (2 if kind < 2 else 2 * cdiv(HW, 256) + cdiv(Dc, 256) + 4 * FN + 21),
    #                                measured: see fusion.maps
    "fusion_n.match": lambda Dc, att, C: k_maps(Dc, att) + C + math.factorial(C),    # measured: see fusion.maps
    # `v = vp[hw] * at[hw]`: 1 on top of the maps (kind 0); kinds 1, 2 copy v: exact
    "fusion.feat": lambda Dc, att, kind: (k_maps(Dc, att) + 1) if kind == 0 else 0,    # measured: see fusion.maps; kinds 1, 2 exact
    # fusion.hip fusion_av_bwd_kernel on top of the maps (whose absref stands for |m| throughout): `acc += df[d] * vp[..]` Dc + 1
    # on an element of E, the slope `m * (1.f - m) * inv_sqrt` 3 + 2 FN / `q0 += s_E[i] * s_m[i]` 2 ceil(2 HW / 256) + 9,
    # `g0 = fmaf(E0[hw] / dn, vv, g0)` (1 + FN) * 2 ceil(HW / 64) + 6, `g / nac`, `s_S[k] * s_a[i] / (na * na)` 3 + 2 FN, `dx[o] += g` 1;
    # dv: 12 products and sums and 3 FN; MixVis' cosine gradient another 6 + 3 FN
    "fusion_av_bwd": lambda Dc, HW, att: k_maps(Dc, att) + Dc + (1 + FN) * 2 * cdiv(HW, 64) + 2 * cdiv(2 * HW, 256) + 8 * FN + 40,
    #                                measured: dv 0.06 at most; dx 0.82 (the rounding of `dx[o] += g` into the prefill); parts 1, 2, 3, 4 alike
    # fusion_n.hip fusion_n_av_bwd_kernel: as above but one thread per (k, d) walks all C * HW positions:
    # `g = fmaf(E[hw] / fmaxf(nv[hw], FN_EPS), vp[hw], g)` (1 + FN) C HW, and `q = fmaf(l.E[..], l.m[..], q)` ceil(C HW / 64) + 6
    "fusion_n_av_bwd": lambda Dc, HW, att, C: k_maps(Dc, att) + Dc + (1 + FN) * C * HW + cdiv(C * HW, 64) + 8 * FN + 40,
    #                                measured: 0.07 (C = 2), 0.06 (C = 3), 0.01 (C = 4)
    # fusion_ao / fusion_n_ao: copies (exact); `dx[..] += g`, g a sum of <= 2 gradients: 2
    "fusion_ao.feat": 0, "fusion_ao.dx": 2,    # measured: feat exact, dx 0.58 (fusion_ao), 0.50 (fusion_n_ao)
    # attention.hip att_infer_fwd_kernel: the maps with Dc = K; `msum += m` S ceil(HW / 256), block_sum 6 + 3, `-tot / HW` FN;
    # `c[s] = fmaf(v, s_m[..], c[s])` ceil(HW / 64), wave_sum 6, `t / (float)HW` FN
    "att.maps": lambda Kc, att: k_maps(Kc, att),    # measured (worst of all six outputs): cos 0.16, sig 0.17, the limit shape 0.02 / 0.03
    "att.match": lambda Kc, HW, att, S: k_maps(Kc, att) + S * cdiv(HW, 256) + 9 + FN,    # measured: see att.maps
    "att.ctx": lambda Kc, HW, att: k_maps(Kc, att) + cdiv(HW, 64) + 6 + FN,    # measured: see att.maps
    # attention.hip att_infer_bwd_kernel: `s_dc = dctx / HW` FN, `dmc[s] = fmaf(s_dc[..], v, dmc[s])` K, `+ dmaps`, `+= cmatch`
    # (FN + 1) 3, the slope 3 + 2 FN / `inv = 1.f / (An * Vn)`, `t -= m * v / (nvv * nvv)` 5 + 2 FN; `dv = fmaf(..)` 2 S;
    # `acc[s] = fmaf(g, v * inv, acc[s])` 2 ceil(HW / 64), wave_sum 6, `s_q[s] * s_a[..] / (na * na)` 3 + FN with
    # `qs[s] = fmaf(g, m, qs[s])` ceil(HW / 256) + 9
    "att_bwd": lambda Kc, HW, att, S: k_maps(Kc, att) + Kc + 2 * cdiv(HW, 64) + cdiv(HW, 256) + 2 * S + 6 * FN + 36,
    #                                measured: see att.maps
}
K_BILIN = 9        # warp_coords.h: `fx + 1.f - ix` 2, `ex * ey` 1, `p[..] + eps` 1, `* b.wnw` 1, `v +=` 3, and `ix - fx` 1


def decided(margin, scale, k=16.0):
    """A decision between two fp32 quantities is decidable when their float64 distance exceeds k * 2^-24 * scale, scale being
    the sum of their absrefs (k = 16: 2^-20, the rule of glueref.undecidable)."""
    return margin > k * U * scale


def first_argmax(t):
    """(index of the FIRST maximum over the last dim, margin = max - the largest value below the max; inf when all are equal)."""
    n = t.shape[-1]
    mx = t.amax(-1, keepdim=True)
    ar = torch.arange(n, device=t.device).expand(t.shape)
    idx = torch.where(t == mx, ar, n).amin(-1)
    second = torch.where(t < mx, t, float("-inf")).amax(-1)
    return idx, mx[..., 0] - second


def take(t, idx):
    """t[..., idx] with idx shaped like t without its last dim."""
    return t.gather(-1, idx[..., None])[..., 0]


# ---- mask loss -------------------------------------------------------------------------------------------------------------------
def activation(l, act):
    """(p, units): the activation of the logits [B, S, FT] and the bound of the kernel's fp32 p, in units of 2^-24."""
    l = l.to(F64)
    if act == ACT_NONE:
        return l, torch.zeros_like(l)
    if act == ACT_RELU:
        return l.clamp_min(0.0), torch.zeros_like(l)
    if act == ACT_SIGMOID:          # 1 / (1 + expf(-v)): expf FN on e = p'(1 - p) of the denominator, `1.f +` 1, division FN
        p = torch.sigmoid(l)
        return p, p * (FN * (1.0 - p) + 1 + FN)
    if act == ACT_TANH:
        p = torch.tanh(l)
        return p, FN * p.abs()
    if act == ACT_SOFTMAX:          # `l[s] - m` 1 (an absolute error |l - m| 2^-24 of the exponent), expf FN; z: S - 1 sums; division FN
        S = l.shape[1]
        p = torch.softmax(l, 1)
        rel = (l - l.amax(1, keepdim=True)).abs() + FN
        relz = (p * rel).sum(1, keepdim=True) + (S - 1)
        return p, p * (rel + relz + FN)
    raise ValueError(act)


def _weights(weight, B, S, FT, like):
    """[B, S(target), FT] of a weight that is None, shared [B, FT] or per target [S, B, FT]."""
    if weight is None:
        return torch.ones((B, S, FT), dtype=F64, device=like.device)
    w = weight.to(F64)
    return w[:, None].expand(B, S, FT) if w.dim() == 2 else w.permute(1, 0, 2)


def loss_iters(FT):
    """Terms a thread of mask_loss_fwd_kernel adds in fp32: grid (min(ceil(FT / 1024), 64), B), 256 threads."""
    return cdiv(FT, min(cdiv(FT, 1024), 64) * 256)


def mask_loss_sums(pred, gt, weight, loss):
    """sums[b, i, j] = sum_ft w_i * l(pred_j, gt_i) on `pred` as given (the kernel's own fp32 pred promoted, or the float64
    activation), and its bound in units: per element the roundings of loss_elem and of `w *`, per thread the fp32 additions."""
    p = pred.to(F64)
    B, S, FT = p.shape
    P, T = p[:, None], gt.to(F64).permute(1, 0, 2)[:, :, None]
    if loss == BCE:       # logf FN, `1.f - p` 1 (exact above 0.5; an absolute 2^-24 of the logarithm), `1.f - t` 1, products 2, sum 1
        lp, lq = torch.log(P).clamp_min(-100.0), torch.log(1.0 - P).clamp_min(-100.0)
        e = -(T * lp + (1.0 - T) * lq)
        ea = T.abs() * lp.abs() + (1.0 - T).abs() * lq.abs()
        units = (FN + 3) * ea + (1.0 - T).abs()
    elif loss == L1:
        e = (P - T).abs()
        ea, units = e, e
    else:
        e = (P - T) ** 2
        ea, units = e, 3 * e
    w = _weights(weight, B, S, FT, p)[:, :, None]
    ref = (w * e).sum(-1)
    bound = (w.abs() * (units + ea)).sum(-1) + loss_iters(FT) * (w.abs() * ea).sum(-1)
    return ref, bound


def _loss_grad(P, T, loss):
    if loss == BCE:
        return (P - T) / ((1.0 - P) * P).clamp_min(BCE_FLOOR)
    if loss == L1:
        return torch.sign(P - T)
    return 2.0 * (P - T)


def mask_loss_bwd(logits, gt, weight, coef, act, loss):
    """dlogits[b, j] = act' * sum_i coef[b, i, j] w_i l'(p_j, gt_i) with float64 autograd for the first-order effect of the
    activation's fp32 error: (ref, units, margins).  units = k * absref + sum_r |d out / d p_r| * units(p_r)."""
    l = logits.to(F64)
    B, S, FT = l.shape
    p0, pu = activation(l, act)
    p = p0.detach().requires_grad_(True)
    P, T = p[:, None], gt.to(F64).permute(1, 0, 2)[:, :, None]
    G = _loss_grad(P, T, loss)                                              # [B, i, j, FT]
    cw = coef.to(F64).reshape(B, S, S)[..., None] * _weights(weight, B, S, FT, l)[:, :, None]
    g, ga = (cw * G).sum(1), (cw.abs() * G.abs()).sum(1)
    if act == ACT_SOFTMAX:
        out = p * (g - (g * p).sum(1, keepdim=True))
        oa = p * (ga + (ga * p).sum(1, keepdim=True))
    else:
        d = {ACT_NONE: torch.ones_like(p), ACT_RELU: (l > 0).to(F64), ACT_SIGMOID: p * (1.0 - p), ACT_TANH: 1.0 - p * p}[act]
        da = {ACT_TANH: 1.0 + p * p}.get(act, d)
        out, oa = g * d, ga * da
    sens = torch.zeros_like(out)
    if bool((pu > 0).any()):
        for s in range(S):
            (gr,) = torch.autograd.grad(out[:, s].sum(), p, retain_graph=True)
            sens[:, s] = (gr.abs() * pu).sum(1)
    k = K["mask_loss_bwd"](act)
    margins = {}
    Pd = p0[:, None]
    if loss == L1:          # fl(p - t) has the sign of p - t: only the fp32 error of p can flip it
        margins["l1 sign"] = (torch.where(pu > 0, (Pd - T).abs().amin(1), float("inf")), pu)
    if loss == BCE:
        pq = ((1.0 - Pd) * Pd)[:, 0]
        margins["bce floor"] = ((pq - BCE_FLOOR).abs(), pq)
    return out.detach(), (k * oa + sens).detach(), margins


# ---- synthesizer -----------------------------------------------------------------------------------------------------------------
def _w(img, scale):
    w = img.to(F64)
    return w * scale.to(F64) if scale is not None else w


def innerprod_fwd(img, snd, scale, bias):
    """z[b, hw] = sum_k img[b, k] scale[k] snd[b, k, hw] + bias."""
    w, s = _w(img, scale), snd.to(F64)
    b = bias.to(F64)[0] if bias is not None else 0.0
    return torch.einsum("bk,bkh->bh", w, s) + b, torch.einsum("bk,bkh->bh", w.abs(), s.abs()) + abs(b)


def innerprod_nosum(img, snd, scale, bias):
    w, s = _w(img, scale)[..., None], snd.to(F64)
    b = bias.to(F64)[0] if bias is not None else 0.0
    return w * s + b, w.abs() * s.abs() + abs(b)


def innerprod_pixelwise(imgs, snd, scale, bias):
    """z[b, p, hw] = sum_k imgs[b, k, p] scale[k] snd[b, k, hw] + bias."""
    w = imgs.to(F64) * (scale.to(F64)[None, :, None] if scale is not None else 1.0)
    s = snd.to(F64)
    b = bias.to(F64)[0] if bias is not None else 0.0
    return torch.einsum("bkp,bkh->bph", w, s) + b, torch.einsum("bkp,bkh->bph", w.abs(), s.abs()) + abs(b)


def innerprod_bwd(img, snd, scale, dz):
    """What avsep_innerprod_bwd writes (dsnd, r) and what _InnerProdFn.backward forms from r (dimg, dscale, dbias)."""
    w, s, d, im = _w(img, scale), snd.to(F64), dz.to(F64), img.to(F64)
    r, ra = torch.einsum("bkh,bh->bk", s, d), torch.einsum("bkh,bh->bk", s.abs(), d.abs())
    out = {"dsnd": (w[..., None] * d[:, None], w.abs()[..., None] * d.abs()[:, None]), "r": (r, ra),
           "dbias": (d.sum().reshape(1), d.abs().sum().reshape(1))}
    if scale is not None:
        sc = scale.to(F64)
        out["dimg"] = (r * sc, ra * sc.abs())
        out["dscale"] = ((im * r).sum(0), (im.abs() * ra).sum(0))
    else:
        out["dimg"] = (r, ra)
    return out


# ---- SDR sums --------------------------------------------------------------------------------------------------------------------
def sdr_sums(est, ref):
    """(<est, ref>, <ref, ref>, <est, est>) per row, summed exactly (math.fsum of the exact float64 products): [R, 3], and the
    sums of the |products|."""
    e, g = est.to(F64).cpu(), ref.to(F64).cpu()
    out, a = [], []
    for r in range(e.shape[0]):
        prods = (e[r] * g[r], g[r] * g[r], e[r] * e[r])
        out.append([math.fsum(t.tolist()) for t in prods])
        a.append([math.fsum(t.abs().tolist()) for t in prods])
    return torch.tensor(out, dtype=F64), torch.tensor(a, dtype=F64)


# ---- log-frequency warp and the preparation of the spectrograms ---------------------------------------------------------------
def linspace_pm1(n):
    """numpy.linspace(-1, 1, n) in float64 (warp_coords.h linspace_pm1)."""
    if n == 1:
        return torch.tensor([-1.0], dtype=F64)
    v = -1.0 + torch.arange(n, dtype=F64) * (2.0 / (n - 1))
    v[-1] = 1.0
    return v


def warp_gy(n_out, warp):
    """The y coordinate of the reference's warpgrid (utils.py:12-26) in float64, before the cast to fp32."""
    yv = linspace_pm1(n_out)
    return (torch.pow(torch.tensor(21.0, dtype=F64), (yv + 1.0) / 2.0) - 11.0) / 10.0 if warp else \
        torch.log(yv * 10.0 + 11.0) / math.log(21.0) * 2.0 - 1.0


def pixel_coord(g, n_in):
    """F.grid_sample's un-normalisation (align_corners=False) of the fp32-cast grid coordinate g, and the bound of the kernel's
    fp32 result in units of 2^-24 (pixels): the cast is taken exactly, but a float64 pow / log that is off by its last bit can
    move the cast by one fp32 ulp (2 units of |g|); `(g + 1.f) * (float)n` 2, `- 1.f` 1, `/ 2.f` exact."""
    g = g.float().to(F64)
    i = ((g + 1.0) * n_in - 1.0) / 2.0
    return i, (2.0 * (g + 1.0).abs() * n_in + ((g + 1.0) * n_in - 1.0).abs()) / 2.0 + g.abs() * n_in


def bilinear(x, iy, uy, ix, ux, eps=0.0):
    """Bilinear sampling with zero padding of x [N, Hin, Win] at the pixel coordinates iy [Hout], ix [Wout] (whose fp32 errors are
    uy, ux units): (ref, units) [N, Hout, Wout].  units = K_BILIN * absref + the position errors times the slopes, the slope
    along y being bounded by (|north| + |south|) and along x by (|west| + |east|) of the interpolated neighbours."""
    x = x.to(F64)
    N, Hin, Win = x.shape
    dev = x.device
    iy, uy, ix, ux = (t.to(dev) for t in (iy, uy, ix, ux))
    fy, fx = torch.floor(iy), torch.floor(ix)
    wy, wx = (iy - fy)[None, :, None], (ix - fx)[None, None, :]
    ey, ex = 1.0 - wy, 1.0 - wx

    def tap(dy, dx):
        yy, xx = (fy + dy).long(), (fx + dx).long()
        ok = ((yy >= 0) & (yy < Hin))[:, None] & ((xx >= 0) & (xx < Win))[None, :]
        v = x[:, yy.clamp(0, Hin - 1)][:, :, xx.clamp(0, Win - 1)] + eps
        return torch.where(ok[None], v, 0.0)
    nw, ne, sw, se = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    ref = nw * ex * ey + ne * wx * ey + sw * ex * wy + se * wx * wy
    a = nw.abs() * ex * ey + ne.abs() * wx * ey + sw.abs() * ex * wy + se.abs() * wx * wy
    slope_y = (nw.abs() + sw.abs()) * ex + (ne.abs() + se.abs()) * wx
    slope_x = (nw.abs() + ne.abs()) * ey + (sw.abs() + se.abs()) * wy
    return ref, K_BILIN * a + uy[None, :, None] * slope_y + ux[None, None, :] * slope_x


def warp(x, Hout, Wout, warp_flag):
    """avsep_warp: grid_sample of x [BC, Hin, Win] on warpgrid(Hout, Wout, warp_flag)."""
    iy, uy = pixel_coord(warp_gy(Hout, warp_flag), x.shape[1])
    ix, ux = pixel_coord(linspace_pm1(Wout), x.shape[2])
    return bilinear(x, iy, uy, ix, ux)


def _clamped(v, units, lo, hi):
    """clamp(v, lo, hi) of a value with a bound: where v is beyond a limit by more than its bound the output IS the limit."""
    sure = (v - U * units > hi) | (v + U * units < lo)
    return v.clamp(lo, hi), torch.where(sure, 0.0, units)


def prepare(mag_mix, mags, warp_flag, weighted, binary, Fout):
    """avsep_prepare (main.py:51-95): mag_mix [B, Fin, T], mags [S, B, Fin, T] -> name -> (ref, units), all of [.., Fout, T];
    "gt_margin": (|src - 0.5 mix|, its bound in units) for the binary mask."""
    S, B, Fin, T = mags.shape
    if warp_flag:
        iy, uy = pixel_coord(warp_gy(Fout, 1), Fin)
        ix, ux = pixel_coord(linspace_pm1(T), T)
        mix, mu = bilinear(mag_mix, iy, uy, ix, ux, EPS_MIX)
        src, su = bilinear(mags.reshape(S * B, Fin, T), iy, uy, ix, ux)
        src, su = src.view(S, B, Fout, T), su.view(S, B, Fout, T)
    else:
        mix, src = mag_mix.to(F64) + EPS_MIX, mags.to(F64)
        mu, su = mix.abs(), torch.zeros_like(src)
    out = {"mag_mix": (mix, mu), "mags": (src, su)}
    lg = torch.log(mix)
    out["log_mag_mix"] = (lg, FN * lg.abs() + mu / mix)
    if weighted:
        w = torch.log1p(mix)
        out["weight"] = _clamped(w, FN * w.abs() + mu / (1.0 + mix), f32(1e-3), 10.0)
    else:
        out["weight"] = (torch.ones_like(mix), torch.zeros_like(mix))
    if binary:
        out["gt"] = ((src > 0.5 * mix).to(F64), torch.zeros_like(src))
        out["gt_margin"] = ((src - 0.5 * mix).abs(), su + 0.5 * mu)
    else:
        r = src / mix
        out["gt"] = _clamped(r, FN * r.abs() + su / mix + r.abs() * mu / mix, 0.0, 5.0)
    return out


# ---- bottleneck fusion -----------------------------------------------------------------------------------------------------------
def cnorm(q):
    """max(sqrt(q), eps) with the gradient the kernels take: none below eps (`if (nv > FUS_EPS) g -= ..`)."""
    big = q > EPS_COS * EPS_COS
    return torch.where(big, torch.where(big, q, 1.0).sqrt(), EPS_COS)


def sim_maps(a, v, att):
    """a [B, Ka, Dc] audio vectors, v [B, C, Dc, HW] visual maps -> (m, ma) [B, Ka, C, HW]: cos (F.cosine_similarity, eps 1e-8) or
    sigmoid(dot / sqrt(Dc)).  ma >= |m|: cos sum |a v| / (|a| |v|); sig m (1 - m) sum |a v| / sqrt(Dc) + m."""
    Dc = a.shape[-1]
    dot = torch.einsum("bkd,bcdh->bkch", a, v)
    dota = torch.einsum("bkd,bcdh->bkch", a.abs(), v.abs()).detach()
    if att == 1:
        m = torch.sigmoid(dot / math.sqrt(Dc))
        md = m.detach()
        return m, md * (1.0 - md) * dota / math.sqrt(Dc) + md
    den = cnorm((a * a).sum(-1))[:, :, None, None] * cnorm((v * v).sum(2))[:, None]
    return dot / den, dota / den.detach()


class Fus:
    pass


def fusion_fwd(x, vs, kind, att, grad=False):
    """The forward of avsep_fusion_av_* (kind 0 hidsep / CoLoc, 1 CoLoc_Sel with C = 2; 2 MixVis with ONE map) and of
    avsep_fusion_n_av_* (kind 0, C = len(vs) in 2..4), restating oracle/nets.py Fusion._coloc / _coloc_n / _mixvis in float64
    with every maximum taken at its FIRST index.  x [B, D, FT], vs: C maps [B, Dc, HW].  Returns an object with the outputs,
    their absrefs (suffix `a`) and the margins of the decisions; grad=True keeps the autograd graph on x64 and v."""
    f = Fus()
    B, D, FT = x.shape
    C, Dc, HW = len(vs), vs[0].shape[1], vs[0].shape[2]
    Ka = 2 if kind == 2 else C
    f.kind, f.att, f.C, f.Ka, f.Dc, f.HW, f.D = kind, att, C, Ka, Dc, HW, D
    f.x64 = x.to(F64).requires_grad_(grad)
    f.v = torch.stack([t.to(F64) for t in vs], 1).requires_grad_(grad)
    f.pool_idx, _ = first_argmax(f.x64.detach())
    f.a_pool = take(f.x64, f.pool_idx)                                    # [B, D]
    f.a = f.a_pool[:, :Ka * Dc].reshape(B, Ka, Dc)
    f.m, f.ma = sim_maps(f.a, f.v, att)
    md = f.m.detach()
    f.arg, f.arg_margin = first_argmax(md)                                # [B, Ka, C]
    f.arg_scale = 2 * f.ma.amax(-1)
    mx, mxa = take(f.m, f.arg), take(f.ma, f.arg)
    vd = f.v.detach()
    f.margins = {"map arg-max": (f.arg_margin, f.arg_scale)}
    if kind == 2:
        w = f.arg[:, :, 0]                                                # [B, 2]
        u = f.v[:, 0].gather(2, w[:, None, :].expand(B, Dc, 2))           # [B, Dc, 2]
        nu, nw = cnorm((u[..., 0] ** 2).sum(1)), cnorm((u[..., 1] ** 2).sum(1))
        f.cos = (u[..., 0] * u[..., 1]).sum(1) / (nu * nw)
        f.cosa = ((u[..., 0] * u[..., 1]).abs().sum(1) / (nu * nw)).detach()
        f.match = -(mx[:, 0, 0] + mx[:, 1, 0]) + f.m[:, :, 0].sum((1, 2)) / HW + f.cos
        f.matcha = mxa[:, 0, 0] + mxa[:, 1, 0] + f.ma[:, :, 0].sum((1, 2)) / HW + f.cosa
        f.att_maps, f.att_mapsa = f.m[:, :, 0], f.ma[:, :, 0]
        f.feat = u.permute(0, 2, 1).reshape(B, 2 * Dc)
        f.feata = f.feat.detach().abs()
        f.sel = w[:, :, None].expand(B, 2, Dc).reshape(B, 2 * Dc)
        f.best = torch.zeros(B, dtype=torch.int64, device=x.device)
        f.u, f.nu, f.nw, f.w = u.detach(), nu.detach(), nw.detach(), w
        return f
    perms = list(itertools.permutations(range(C)))
    f.perms = perms
    scores = torch.stack([sum(mx[:, pm[c], c] for c in range(C)) for pm in perms], 1)              # [B, P]
    scoresa = torch.stack([sum(mxa[:, pm[c], c] for c in range(C)) for pm in perms], 1)
    f.best, best_margin = first_argmax(scores.detach())
    if C > 2:       # sums of three and more maxima in permutation order: equal terms do not make equal fp32 scores, a tie is no tie
        top = scores.detach().topk(2, dim=1).values
        best_margin = top[:, 0] - top[:, 1]
    f.margins["best permutation"] = (best_margin, 2 * scoresa.amax(-1))
    f.match = scores.sum(1) - 2.0 * take(scores, f.best)
    f.matcha = scoresa.sum(1)
    f.kk = torch.tensor(perms, device=x.device)[f.best]                   # [B, C]: audio block of visual map c
    route = f.kk[:, None, :, None].expand(B, 1, C, HW)
    f.att_maps, f.att_mapsa = f.m.gather(1, route)[:, 0], f.ma.gather(1, route)[:, 0]          # [B, C, HW]
    if kind == 0:
        prod = f.v * f.att_maps[:, :, None]
        proda = vd.abs() * f.att_mapsa[:, :, None]
        sel, sel_margin = first_argmax(prod.detach())                     # [B, C, Dc]
        f.margins["attended arg-max"] = (sel_margin, 2 * proda.amax(-1))
        feat, feata = take(prod, sel), take(proda, sel)
    else:
        where = take(f.arg.permute(0, 2, 1), f.kk)                        # [B, C]: arg-max of the chosen map of c
        sel = where[:, :, None].expand(B, C, Dc)
        feat = take(f.v, sel)
        feata = feat.detach().abs()
    pad = D - C * Dc
    z = torch.zeros((B, pad), dtype=F64, device=x.device)
    f.feat, f.feata = torch.cat([feat.reshape(B, C * Dc), z], 1), torch.cat([feata.reshape(B, C * Dc), z], 1)
    f.sel = torch.cat([sel.reshape(B, C * Dc), z.long()], 1)
    return f


def fusion_bwd(f, dfeat, dmaps, dmatch):
    """Gradients of sum(dfeat * feat) + sum(dmaps * att_maps) + dmatch * sum_b match[b] by float64 autograd of fusion_fwd
    (grad=True): {"dx": values at the pooled positions [B, D], "dv": [B, C, Dc, HW]} as (ref, absref); the absref restates the
    kernels' backward on absolute values, with the maps' absref standing for |m| (and for the sigmoid's slope)."""
    B, Ka, C, Dc, HW, kind, att = f.x64.shape[0], f.Ka, f.C, f.Dc, f.HW, f.kind, f.att
    L = (dfeat.to(F64) * f.feat).sum() + float(dmatch) * f.match.sum()
    if dmaps is not None:
        L = L + (dmaps.to(F64) * f.att_maps).sum()
    gx, gv = torch.autograd.grad(L, [f.x64, f.v], allow_unused=True)
    dx = take(gx, f.pool_idx)
    a, v, ma, dm = f.a.detach().abs(), f.v.detach().abs(), f.ma, abs(float(dmatch))
    df = dfeat.to(F64).abs()
    E = torch.zeros_like(ma)                                              # [B, Ka, C, HW]
    if kind == 2:
        E[:, :, 0] = dm / HW + (dmaps.to(F64).abs() if dmaps is not None else 0.0)
        E[:, :, 0].scatter_add_(-1, f.w[..., None], torch.full((B, 2, 1), dm, dtype=F64, device=E.device))
    else:
        cf = torch.zeros((B, Ka, C), dtype=F64, device=E.device)          # coefficient of max m[k][c] in the match term
        for p, pm in enumerate(f.perms):
            sign = torch.where(f.best == p, -1.0, 1.0).to(F64)
            for c in range(C):
                cf[:, pm[c], c] += sign
        E.scatter_add_(-1, f.arg[..., None], (cf.abs() * dm)[..., None])
        chosen = (f.kk[:, None, :] == torch.arange(Ka, device=E.device)[None, :, None]).to(F64)[..., None]     # [B, Ka, C, 1]
        if dmaps is not None:
            E = E + chosen * dmaps.to(F64).abs()[:, None]
        if kind == 0:
            sel = f.sel[:, :C * Dc].reshape(B, C, Dc)
            t = torch.zeros((B, C, HW), dtype=F64, device=E.device)
            t.scatter_add_(2, sel, df[:, :C * Dc].reshape(B, C, Dc) * take(v, sel))
            E = E + chosen * t[:, None]
    if att == 1:
        G = E * ma / math.sqrt(Dc)
        dxa = torch.einsum("bkch,bcdh->bkd", G, v)
        dva = torch.einsum("bkch,bkd->bcdh", G, a)
    else:
        qa, qv = (f.a.detach() ** 2).sum(-1), (f.v.detach() ** 2).sum(2)
        nac, nvc = cnorm(qa), cnorm(qv)                                   # [B, Ka], [B, C, HW]
        a_ok, v_ok = (nac > EPS_COS).to(F64), (nvc > EPS_COS).to(F64)
        S = (E * ma).sum((2, 3))
        dxa = torch.einsum("bkch,bcdh->bkd", E / nvc[:, None], v) / nac[..., None] + (a_ok * S / nac ** 2)[..., None] * a
        dva = torch.einsum("bkch,bkd->bcdh", E, a / nac[..., None]) / nvc[:, :, None] \
            + (v_ok * (E * ma).sum(1) / nvc ** 2)[:, :, None] * v
    if kind == 0:
        sel = f.sel[:, :C * Dc].reshape(B, C, Dc)
        dva.scatter_add_(3, sel[..., None], (df[:, :C * Dc].reshape(B, C, Dc) * take(f.att_mapsa[:, :, None].expand(B, C, Dc, HW), sel))[..., None])
    elif kind == 1:
        sel = f.sel.reshape(B, C, Dc)
        dva.scatter_add_(3, sel[..., None], df.reshape(B, C, Dc)[..., None])
    else:
        u0, u1 = f.u[..., 0].abs(), f.u[..., 1].abs()
        nn = (f.nu * f.nw)[:, None]
        t0 = u1 / nn + ((f.nu > EPS_COS) * f.cosa / f.nu ** 2)[:, None] * u0
        t1 = u0 / nn + ((f.nw > EPS_COS) * f.cosa / f.nw ** 2)[:, None] * u1
        add = torch.stack([df[:, :Dc] + dm * t0, df[:, Dc:] + dm * t1], 2)              # [B, Dc, 2]
        dva[:, 0].scatter_add_(2, f.w[:, None, :].expand(B, Dc, 2), add)
    z = torch.zeros((B, f.D - Ka * Dc), dtype=F64, device=E.device)
    return {"dx": (dx, torch.cat([dxa.reshape(B, Ka * Dc), z], 1)), "dv": (gv, dva)}


def perm_table(C, device=None):
    return torch.tensor(list(itertools.permutations(range(C))), device=device)


def fusion_ao(x, draws, C, all_zero=False):
    """The audio-only branch: the pooled blocks in the drawn order.  C = 2 with boolean draws: oracle/nets.py ao_swap (draw 0 ->
    (block 1, block 0); every draw 0 -> both slots block 1, `all_zero`); otherwise ao_permute_n with permutation indices.
    Returns (feat [B, D], pool_idx [B, D], src [B, D]: the pooled channel a tile channel copies, -1 for the zero remainder)."""
    B, D, FT = x.shape
    Dc = D // C
    x64 = x.to(F64)
    pool_idx, _ = first_argmax(x64)
    a = take(x64, pool_idx)
    if draws.dtype in (torch.bool, torch.uint8):
        d = draws.to(x.device).long()
        blocks = torch.stack([torch.where(d > 0, 0, 1), torch.where(d > 0, 1, 0)], 1)
        if all_zero:
            blocks = torch.ones_like(blocks)
    else:
        blocks = perm_table(C, x.device)[draws.to(x.device).long()]                                   # [B, C]
    src = (blocks[:, :, None] * Dc + torch.arange(Dc, device=x.device)[None, None]).reshape(B, C * Dc)
    src = torch.cat([src, torch.full((B, D - C * Dc), -1, device=x.device)], 1)
    feat = torch.where(src >= 0, a.gather(1, src.clamp_min(0)), 0.0)
    return feat, pool_idx, src


def fusion_ao_bwd(src, dfeat):
    """dx at the pooled positions [B, D]: channel i receives the gradients of every tile channel that copied it."""
    B, D = src.shape
    g = torch.zeros((B, D + 1), dtype=F64, device=dfeat.device)
    ga = torch.zeros_like(g)
    idx = torch.where(src >= 0, src, D)
    g.scatter_add_(1, idx, dfeat.to(F64))
    ga.scatter_add_(1, idx, dfeat.to(F64).abs())
    return g[:, :D], ga[:, :D]


# ---- SoP++ attention module ---------------------------------------------------------------------------------------------------
def attention_fwd(a, mix, att, grad=False):
    """avsep_attmodel_infer_fwd: a [B, S, K] queries, mix [B, K, HW] -> maps_raw, match [B], ctx [B, S, K] (the formula of
    tests/test_gpu_ops.py::test_attmodel_core_kernel), their absrefs and the clamp's margins."""
    f = Fus()
    f.a64, f.v = a.to(F64).requires_grad_(grad), mix.to(F64).requires_grad_(grad)
    f.m, f.ma = sim_maps(f.a64, f.v[:, None], att)
    f.m, f.ma = f.m[:, :, 0], f.ma[:, :, 0]                               # [B, S, HW]
    HW = f.m.shape[-1]
    f.match, f.matcha = -f.m.sum((1, 2)) / HW, f.ma.sum((1, 2)) / HW
    f.mc = f.m.clamp(0.0, 1.0)
    f.ctx = torch.einsum("bkh,bsh->bsk", f.v, f.mc) / HW
    f.ctxa = torch.einsum("bkh,bsh->bsk", f.v.detach().abs(), f.ma) / HW
    md = f.m.detach()
    live = f.ma > 0                                                       # a zero query or position: m is exactly 0 on both sides
    f.margins = {"clamp": (torch.where(live, torch.minimum(md.abs(), (1.0 - md).abs()), float("inf")), f.ma)}
    f.att = att
    return f


def attention_bwd(f, dctx, dmaps, dmatch):
    """Gradients of sum(dctx * ctx) + sum(dmaps * clamp(maps)) + sum(dmatch * match) by float64 autograd, and the absref that
    restates att_infer_bwd_kernel on absolute values: {"da": .., "dmix": ..}."""
    L = (dctx.to(F64) * f.ctx).sum()
    if dmaps is not None:
        L = L + (dmaps.to(F64) * f.mc).sum()
    if dmatch is not None:
        L = L + (dmatch.to(F64) * f.match).sum()
    da, dmix = torch.autograd.grad(L, [f.a64, f.v])
    a, v, ma = f.a64.detach().abs(), f.v.detach().abs(), f.ma
    B, S, Kc = a.shape
    HW = v.shape[-1]
    md = f.m.detach()
    dc = dctx.to(F64).abs() / HW
    g = torch.einsum("bsk,bkh->bsh", dc, v)
    if dmaps is not None:
        g = g + dmaps.to(F64).abs()
    g = g * ((md >= 0) & (md <= 1)).to(F64)
    if dmatch is not None:
        g = g + dmatch.to(F64).abs()[:, None, None] / HW
    through_ctx = torch.einsum("bsk,bsh->bkh", dc, ma)
    if f.att == 1:
        G = g * ma / math.sqrt(Kc)
        return {"da": (da, torch.einsum("bsh,bkh->bsk", G, v)), "dmix": (dmix, through_ctx + torch.einsum("bsh,bsk->bkh", G, a))}
    qa, qv = (f.a64.detach() ** 2).sum(-1), (f.v.detach() ** 2).sum(1)
    An, Vn = cnorm(qa), cnorm(qv)                                         # [B, S], [B, HW]
    a_ok, v_ok = (An > EPS_COS).to(F64), (Vn > EPS_COS).to(F64)
    inv = 1.0 / (An[:, :, None] * Vn[:, None])                            # [B, S, HW]
    daa = torch.einsum("bsh,bkh->bsk", g * inv, v) + (a_ok * (g * ma).sum(-1) / An ** 2)[..., None] * a
    dma = through_ctx + torch.einsum("bsh,bsk->bkh", g * inv, a) + ((g * ma).sum(1) * v_ok / Vn ** 2)[:, None] * v
    return {"da": (da, daa), "dmix": (dmix, dma)}


# ---- the gate ------------------------------------------------------------------------------------------------------------------
def gate(out, ref, absref, k, unit=U, excluded=None):
    """(elements with |out - ref| > k * unit * absref or NaN — where absref is 0: out != ref —, worst ratio, its flat index)."""
    o = out.to(F64).reshape(ref.shape)
    err, bound = (o - ref).abs(), k * unit * absref
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, 1.0), torch.where(err > 0, float("inf"), 0.0))
    r = torch.where(torch.isnan(o), float("inf"), r)
    if excluded is not None:
        r = torch.where(excluded, 0.0, r)
    if r.numel() == 0:
        return 0, 0.0, 0
    i = int(torch.argmax(r.reshape(-1)))
    return int((r > 1.0).sum()), float(r.reshape(-1)[i]), i
