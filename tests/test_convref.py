"""not-gpu: tests/convref.py (the float64 reference of one conv call and its error gate) against independent direct
computations, the gate's sensitivity to planted defects, and the 32-bit buffer-range guards of the Winograd kernels."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import convref as R

F64 = torch.float64


# ---- independent restatement: explicit loops for the virtual input, F.unfold GEMMs for the convolution ----------------------
def _act(v, act):
    v = v.contiguous()
    out = v.clone()
    for idx in range(v.numel()):
        x = v.view(-1)[idx]
        if x <= 0 and act == R.ACT_RELU:
            out.view(-1)[idx] = 0.0
        elif x <= 0 and act == R.ACT_LRELU02:
            out.view(-1)[idx] = x * torch.tensor(0.2, dtype=torch.float32)
    return out


def _direct_virtual(srcs, up, bf=False, absolute=False):
    chans = []
    for x, sc, sh, act in srcs:
        if bf:
            x = x.to(torch.bfloat16).float()
        for c in range(x.shape[1]):
            p = x[:, c]
            if sc is not None:       # one fp32 rounding of the exact product + sum
                p = (p.double() * float(sc[c]) + float(sh[c])).float()
            v = _act(p, act)
            chans.append((v.to(torch.bfloat16).float() if bf else v).double())
    v = torch.stack(chans, 1)
    if absolute:
        v = v.abs()
    if not up:
        return v
    N, C, h, w = v.shape
    out = torch.zeros(N, C, 2 * h, 2 * w, dtype=F64)
    for i in range(2 * h):
        fy = i * (h - 1) / (2 * h - 1)
        y0 = int(fy); y1 = min(y0 + 1, h - 1); ay = fy - y0
        for j in range(2 * w):
            fx = j * (w - 1) / (2 * w - 1)
            x0 = int(fx); x1 = min(x0 + 1, w - 1); ax = fx - x0
            out[:, :, i, j] = ((1 - ay) * ((1 - ax) * v[:, :, y0, x0] + ax * v[:, :, y0, x1]) +
                               ay * ((1 - ax) * v[:, :, y1, x0] + ax * v[:, :, y1, x1]))
    return out


def _unfold(g, v):
    return F.unfold(v, (g.KH, g.KW), dilation=g.d.dil, padding=g.d.pad, stride=g.d.stride)     # [N, Cin*KH*KW, L]


def _direct_fwd(g, v, w, b):
    y = w.reshape(g.Cout, -1) @ _unfold(g, v)
    if b is not None:
        y = y + b.view(1, -1, 1)
    return y.reshape(g.N, g.Cout, g.Ho, g.Wo)


def _direct_dgrad(g, dy, w):
    cols = w.reshape(g.Cout, -1).t() @ dy.reshape(g.N, g.Cout, -1)
    return F.fold(cols, (g.H, g.W), (g.KH, g.KW), dilation=g.d.dil, padding=g.d.pad, stride=g.d.stride)


def _direct_wgrad(g, dy, v):
    return (dy.reshape(g.N, g.Cout, -1) @ _unfold(g, v).transpose(1, 2)).sum(0).reshape(g.Cout, g.Cin, g.KH, g.KW)


def _case(seed, N, C0, C1, Hs, Ws, Cout, k, s, p, dil, acts, up, bf):
    gen = torch.Generator().manual_seed(seed)
    srcs, op = [], {"bf16": bf}
    for i, (c, act) in enumerate(zip((C0, C1), acts)):
        if c == 0:
            continue
        x = torch.randn(N, c, Hs, Ws, generator=gen)
        sc, sh = (torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.3) if act else (None, None)
        srcs.append((x, sc, sh, act))
        op.update({f"x{i}": x, f"sc{i}": sc, f"sh{i}": sh})
    H, W = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    g = R.Geometry(N, C0 + C1, H, W, Cout, k, s, p, dil, C0=C0, act0=acts[0], act1=acts[1], up2x=up)
    op["w"] = torch.randn(Cout, C0 + C1, k, k, generator=gen)
    op["bias"] = torch.randn(Cout, generator=gen)
    op["dy"] = torch.randn(N, Cout, g.Ho, g.Wo, generator=gen)
    return g, op, srcs


CASES = [
    # seed, N, C0, C1, Hs, Ws, Cout, k, stride, pad, dil, (act0, act1), up2x, bf16
    (1, 2, 3, 2, 7, 6, 4, 3, 1, 1, 1, (R.ACT_RELU, R.ACT_LRELU02), False, False),      # two sources, affine + ReLU / LeakyReLU
    (2, 2, 2, 3, 5, 3, 3, 3, 1, 1, 1, (R.ACT_RELU, R.ACT_RELU), True, False),           # up2x with odd low-res sizes
    (3, 2, 4, 0, 9, 8, 5, 3, 2, 1, 1, (R.ACT_LRELU02, 0), False, False),                # stride 2
    (4, 1, 3, 0, 11, 10, 4, 3, 1, 2, 2, (0, 0), False, False),                          # dilation 2
    (5, 2, 4, 0, 9, 7, 3, 1, 2, 0, 1, (R.ACT_RELU, 0), False, False),                   # 1x1 / stride 2
    (6, 1, 3, 0, 15, 13, 2, 7, 2, 3, 1, (0, 0), False, False),                          # 7x7 / stride 2 (the stem)
    (7, 2, 16, 0, 6, 5, 4, 4, 2, 1, 1, (R.ACT_LRELU02, 0), False, True),               # bf16 operand model, 4x4 / s2
    (8, 2, 16, 0, 5, 6, 3, 3, 1, 1, 1, (0, 0), False, True),                            # bf16, raw input
]


@pytest.mark.parametrize("case", CASES)
def test_reference_matches_direct_computation(case):
    g, op, srcs = _case(*case)
    bf = op["bf16"]
    v = _direct_virtual(srcs, g.d.up2x, bf)
    va = _direct_virtual(srcs, g.d.up2x, bf, absolute=True)
    w = op["w"].double()
    w = w.to(torch.bfloat16).double() if bf else w
    dy = op["dy"].double()
    dy = dy.to(torch.bfloat16).double() if bf else dy
    b = op["bias"].double()
    torch.testing.assert_close(R.virtual_input(g, op), v, rtol=1e-13, atol=1e-13)
    r = R.reference(g, "fwd", dict(op, stats=True))
    y = _direct_fwd(g, v, w, b)
    torch.testing.assert_close(r["y"][0], y, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["y"][1], _direct_fwd(g, va, w.abs(), b.abs()), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["stats"][0], torch.cat([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))]), rtol=1e-12, atol=1e-11)
    r = R.reference(g, "dgrad", op)
    torch.testing.assert_close(r["dx"][0], _direct_dgrad(g, dy, w), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["dx"][1], _direct_dgrad(g, dy.abs(), w.abs()), rtol=1e-12, atol=1e-12)
    r = R.reference(g, "wgrad", dict(op, want_bias=True))
    torch.testing.assert_close(r["dw"][0], _direct_wgrad(g, dy, v), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["dw"][1], _direct_wgrad(g, dy.abs(), va), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["dbias"][0], dy.sum((0, 2, 3)), rtol=1e-12, atol=1e-12)


def test_reference_dgrad_act_composition():
    """act'(scale*y + shift + res_scale*residual + res_shift) * (dgrad(dy) + dz2) + add and the BatchNorm-backward sums, each
    element written out from its definition; pre-activations that sit on 0 are reported as excluded."""
    g, op, _ = _case(11, 2, 4, 0, 6, 7, 5, 3, 1, 1, 1, (0, 0), False, False)
    gen = torch.Generator().manual_seed(12)
    shape = (g.N, g.Cin, g.H, g.W)
    y, res, dz2, add = (torch.randn(shape, generator=gen) for _ in range(4))
    sc, sh, rs, rh = (torch.randn(g.Cin, generator=gen) for _ in range(4))
    mean, invstd = torch.randn(g.Cin, generator=gen), torch.rand(g.Cin, generator=gen) + 0.5
    # a pre-activation that cancels to (close to) 0: the residual term is the negative of the BatchNorm term
    p1 = float(y[0, 1, 2, 3]) * float(sc[1]) + float(sh[1])
    res[0, 1, 2, 3] = (-p1 - float(rh[1])) / float(rs[1])
    for act in (R.ACT_RELU, R.ACT_LRELU02):
        r = R.reference(g, "dgrad_act", dict(op, y=y, scale=sc, shift=sh, residual=res, res_scale=rs, res_shift=rh, dz2=dz2,
                                             add=add, mean=mean, invstd=invstd, act=act, bstats=True))
        gd = _direct_dgrad(g, op["dy"].double(), op["w"].double())
        gda = _direct_dgrad(g, op["dy"].double().abs(), op["w"].double().abs())
        dx, dxa = torch.empty(shape, dtype=F64), torch.empty(shape, dtype=F64)
        for n in range(g.N):
            for c in range(g.Cin):
                for i in range(g.H):
                    for j in range(g.W):
                        p1 = torch.tensor(float(y[n, c, i, j]) * float(sc[c]) + float(sh[c]), dtype=F64).float()
                        p2 = torch.tensor(float(res[n, c, i, j]) * float(rs[c]) + float(rh[c]), dtype=F64).float()
                        pre = float((p1.double() + p2.double()).float())
                        m = 1.0 if pre > 0 else (0.0 if act == R.ACT_RELU else float(torch.tensor(0.2, dtype=torch.float32)))
                        dx[n, c, i, j] = m * (gd[n, c, i, j] + float(dz2[n, c, i, j])) + float(add[n, c, i, j])
                        dxa[n, c, i, j] = m * (gda[n, c, i, j] + abs(float(dz2[n, c, i, j]))) + abs(float(add[n, c, i, j]))
        torch.testing.assert_close(r["dx"][0], dx, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(r["dx"][1], dxa, rtol=1e-12, atol=1e-12)
        assert r["excluded"][0, 1, 2, 3] and int(r["excluded"].sum()) <= 2
        xhat = (y.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
        torch.testing.assert_close(r["bstats"][0], torch.cat([dx.sum((0, 2, 3)), (dx * xhat).sum((0, 2, 3))]),
                                   rtol=1e-12, atol=1e-11)


def test_reference_dgrad_up2x_composition():
    """dgrad followed by relu_up2x_bwd: the transposed bilinear x2 written as explicit scatters, ReLU masks from the affine
    pre-activations, g0 accumulated into, g1 and the BatchNorm-backward sums of source 1."""
    g, op, srcs = _case(21, 2, 3, 2, 5, 3, 2, 3, 1, 1, 1, (R.ACT_RELU, R.ACT_RELU), True, False)
    gen = torch.Generator().manual_seed(22)
    acc = torch.randn(g.N, 3, 5, 3, generator=gen)
    mean1, invstd1 = torch.randn(2, generator=gen), torch.rand(2, generator=gen) + 0.5
    r = R.reference(g, "dgrad_up2x", dict(op, g0_acc=acc, mean1=mean1, invstd1=invstd1, bstats1=True))
    gd = _direct_dgrad(g, op["dy"].double(), op["w"].double())
    h, w = 5, 3
    lo = torch.zeros(g.N, g.Cin, h, w, dtype=F64)
    for i in range(2 * h):
        fy = i * (h - 1) / (2 * h - 1); y0 = int(fy); y1 = min(y0 + 1, h - 1); ay = fy - y0
        for j in range(2 * w):
            fx = j * (w - 1) / (2 * w - 1); x0 = int(fx); x1 = min(x0 + 1, w - 1); ax = fx - x0
            gij = gd[:, :, i, j]
            lo[:, :, y0, x0] += (1 - ay) * (1 - ax) * gij
            lo[:, :, y0, x1] += (1 - ay) * ax * gij
            lo[:, :, y1, x0] += ay * (1 - ax) * gij
            lo[:, :, y1, x1] += ay * ax * gij
    pre = [(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float() for x, sc, sh, _ in srcs]
    g0 = (pre[0] > 0).double() * lo[:, :3] + acc.double()
    g1 = (pre[1] > 0).double() * lo[:, 3:]
    torch.testing.assert_close(r["g0"][0], g0, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["g1"][0], g1, rtol=1e-12, atol=1e-12)
    xhat = (srcs[1][0].double() - mean1.double().view(1, -1, 1, 1)) * invstd1.double().view(1, -1, 1, 1)
    torch.testing.assert_close(r["bstats1"][0], torch.cat([g1.sum((0, 2, 3)), (g1 * xhat).sum((0, 2, 3))]), rtol=1e-12, atol=1e-11)
    assert (r["g0"][1] >= r["g0"][0].abs() - 1e-12).all() and (r["g1"][1] >= r["g1"][0].abs() - 1e-12).all()


def test_reference_takes_b16_images_verbatim():
    """A B16 image [N, C/16, H, W, 16] is the same operand as its fp32 NCHW form."""
    g, op, _ = _case(31, 2, 16, 0, 5, 4, 3, 3, 1, 1, 1, (R.ACT_RELU, 0), False, True)
    x = op["x0"].to(torch.bfloat16)
    img = x.reshape(2, 1, 16, 5, 4).permute(0, 1, 3, 4, 2).contiguous()
    a = R.reference(g, "fwd", dict(op, x0=x.float()))["y"][0]
    b = R.reference(g, "fwd", dict(op, x0=img))["y"][0]
    assert torch.equal(a, b)


# ---- check(): an honest fp32 convolution passes at the direct-form tau, planted defects fail ---------------------------------
TAU_DIRECT = 2e-5


def _defects(g, op, out, ref, absref, tau):
    """(a) input channel c of the weight zeroed for every tap, (b) one border row of the last image zeroed,
    (c) one element off by 8 tau absref.  Each returns the defective output."""
    w = op["w"].clone()
    w[:, 1] = 0
    a = F.conv2d(R.virtual_input(g, op).float(), w, op["bias"], g.d.stride, g.d.pad, g.d.dil)
    b = out.clone()
    b[-1, :, -1, :] = 0
    c = out.clone()
    i = int(torch.argmax(absref))
    c.view(-1)[i] += float(8 * tau * absref.reshape(-1)[i])
    return a, b, c


@pytest.mark.parametrize("case", CASES[:6])
def test_check_passes_honest_fp32_and_rejects_planted_defects(case):
    g, op, _ = _case(*case)
    ref, absref = R.reference(g, "fwd", op)["y"]
    out = F.conv2d(R.virtual_input(g, op).float(), op["w"], op["bias"], g.d.stride, g.d.pad, g.d.dil)
    ratio, *_ = R.check(out, ref, absref, TAU_DIRECT)
    assert ratio <= 1.0, ratio
    for what, bad in zip("abc", _defects(g, op, out, ref, absref, TAU_DIRECT)):
        ratio, *_ = R.check(bad, ref, absref, TAU_DIRECT)
        assert ratio > 1.0, (what, ratio)
    # the weight gradient (heavy cancellation): an honest fp32 one passes
    v = R.virtual_input(g, op).float().requires_grad_(True)
    w = op["w"].clone().requires_grad_(True)
    dw = torch.autograd.grad(F.conv2d(v, w, None, g.d.stride, g.d.pad, g.d.dil), w, op["dy"])[0]
    ratio, *_ = R.check(dw, *R.reference(g, "wgrad", op)["dw"], TAU_DIRECT)
    assert ratio <= 1.0, ratio


def test_check_exact_where_absref_is_zero_and_b16_half_ulp():
    ref = torch.tensor([0.0, 1.0, -3.0], dtype=F64)
    absref = torch.tensor([0.0, 1.0, 3.0], dtype=F64)
    assert R.check(torch.tensor([0.0, 1.0, -3.0]), ref, absref, 1e-5)[0] == 0.0
    assert R.check(torch.tensor([1e-30, 1.0, -3.0]), ref, absref, 1e-5)[0] == float("inf")
    assert R.check(torch.tensor([0.0, 1.0, float("nan")]), ref, absref, 1e-5)[0] == float("inf")
    # a B16 output may be off by half a bf16 ulp of the value on top of tau * absref (2^-8 relative at the bottom of a binade,
    # 2^-9 at its top), not by more
    v = torch.tensor([0.0, 1.0 + 2.0 ** -8, -3.0 + 3 * 2.0 ** -9], dtype=torch.float32)
    assert R.check(v, ref, absref, 1e-5)[0] > 1.0 and R.check(v, ref, absref, 1e-5, b16=True)[0] <= 1.0
    v = torch.tensor([0.0, 1.0 + 2.0 ** -7, -3.0], dtype=torch.float32)
    assert R.check(v, ref, absref, 1e-5, b16=True)[0] > 1.0
    assert float(R.half_ulp_bf16(torch.tensor(1.0))) == 2.0 ** -8 and float(R.half_ulp_bf16(torch.tensor(1.99))) == 2.0 ** -8


def test_tile_absref_covers_every_tile_of_an_element():
    a = torch.zeros(1, 1, 12, 12, dtype=F64)
    a[0, 0, 5, 5] = 1.0
    t = R.tile_absref(a)
    assert (t[0, 0, 2:9, 2:9] == 1).all() and t.sum() == 49          # every 4x4 tile holding (5, 5)
    w = torch.zeros(2, 2, 3, 3, dtype=F64)
    w[1, 0, 2, 1] = 3.0
    tw = R.tile_absref(w)
    assert (tw[1, 0] == 3).all() and tw.sum() == 27


# ---- 32-bit buffer-range guards of the Winograd kernels ---------------------------------------------------------------------
LIMIT = 0x3ffffffc          # last addressable element + resource shift: 4 * (elems + shift) <= 0xfffffff0


def _desc(P, N, C, H, W, Cout, k=3, stride=1, pad=1, dil=1, algo=0):
    d = P.lib.ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout = N, C, H, W, Cout
    d.Ho, d.Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    d.KH = d.KW = k
    d.stride, d.pad, d.dil, d.C0, d.algo = stride, pad, dil, C, algo
    d.x0 = 256                                   # never dereferenced: the dispatch queries only check that it is set
    return d


def _nmax(*terms):
    """Largest N with per_image * N + shift <= LIMIT for every (per_image, shift)."""
    return min((LIMIT - shift) // per for per, shift in terms)


# family, mode, (C, H, W, Cout, k, stride, pad, dil), algo bits, [(elements per image, resource shift)] of x and dY
GUARDS = [
    ("winow4_kernel", 2, (64, 45, 241, 64, 3, 1, 1, 1), 0, lambda C, H, W, Co: [(C * H * W, W + 1), (Co * H * W, 0)]),
    ("winow4_kernel", 2, (64, 56, 56, 128, 3, 1, 1, 1), 0, lambda C, H, W, Co: [(C * H * W, W + 1), (Co * H * W, 0)]),
    ("winow4_kernel", 2, (64, 28, 28, 64, 3, 1, 2, 2), 0, lambda C, H, W, Co: [(C * H * W, 2 * W + 2), (Co * H * W, 0)]),
    ("winow_kernel", 2, (64, 56, 56, 64, 3, 1, 1, 1), 64, lambda C, H, W, Co: [(C * H * W, W + 2), (Co * H * W, 0)]),
    ("winow_kernel", 2, (64, 28, 28, 64, 3, 1, 2, 2), 64, lambda C, H, W, Co: [(C * H * W, 2 * (W + 2)), (Co * H * W, 0)]),
    ("wgrad4d_kernel", 2, (64, 64, 64, 128, 4, 2, 1, 1), 0, lambda C, H, W, Co: [(C * H * W, W + 2), (Co * H * W // 4, 0)]),
    ("wino4_kernel", 0, (64, 56, 56, 64, 3, 1, 1, 1), 0, lambda C, H, W, Co: [(C * H * W, 0)]),
    ("wino4_kernel", 1, (64, 56, 56, 128, 3, 1, 1, 1), 0, lambda C, H, W, Co: [(Co * H * W, 0)]),
    ("wino_kernel", 0, (64, 32, 32, 64, 3, 1, 1, 1), 64, lambda C, H, W, Co: [(C * H * W, 0)]),
    ("wino_kernel", 1, (128, 32, 32, 64, 3, 1, 1, 1), 64, lambda C, H, W, Co: [(Co * H * W, 0)]),
]


@pytest.mark.parametrize("family,mode,geo,algo,terms", GUARDS)
def test_winograd_buffer_range_guards(family, mode, geo, algo, terms):
    """Each guarded family takes its shape up to the largest N whose last valid element (plus the resource's base shift) is
    addressable through num_records = 0xfffffff0, and not one image more.  (C0 = Cout = 64, 45 x 241, N = 1547: N*C*H*W =
    2^30 - 64 used to pass the winow4_kernel guard, with the last image's x at byte offsets past 2^32.)"""
    import avsep_amd as P
    L = P.lib.load()
    C, H, W, Co, k, s, p, dil = geo
    n = _nmax(*terms(C, H, W, Co))
    name = lambda N: L.avsep_conv_kernel_name(ctypes.byref(_desc(P, N, C, H, W, Co, k, s, p, dil, algo)), mode, 1).decode()
    assert name(n) == family, (n, name(n))
    assert name(n + 1) != family, (n + 1, name(n + 1))
    if geo[:4] == (64, 45, 241, 64):
        assert 1547 * C * H * W == 2 ** 30 - 64 and n == 1546
