"""not-gpu: tests/glueref.py (the float64 references of the glue kernels) against torch autograd, BatchNorm2d, F.max_pool2d and
optim.SGD in float64, at two small shapes each."""
import pytest
import torch
import torch.nn.functional as F

import convref as R
import glueref as G

F64 = torch.float64
SHAPES = [(2, 3, 5, 7), (3, 4, 6, 4)]
TOL = 1e-12


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _close(a, b, what=""):
    a, b = a.detach().to(F64), b.detach().to(F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max())), what


def _act64(v, act):
    return {0: v, 1: F.relu(v), 2: F.leaky_relu(v, R.LRELU_SLOPE)}[act]


@pytest.mark.parametrize("shape", SHAPES)
def test_batchnorm_pieces_against_batchnorm2d(shape):
    """channel_stats -> mean / var; affine_act_bwd's sums with act = none -> the folded coefficients; bn_bwd_apply -> the
    gradient BatchNorm2d's autograd returns in training mode."""
    N, Cc, H, W = shape
    x, dz = _rand(shape, 1), _rand(shape, 2)
    gamma, beta = _rand((Cc,), 3), _rand((Cc,), 4)
    bn = torch.nn.BatchNorm2d(Cc, eps=1e-5).double()
    bn.weight.data, bn.bias.data = gamma.double(), beta.double()
    xd = x.double().requires_grad_()
    z = bn(xd)
    (want,) = torch.autograd.grad(z, xd, dz.double())
    stats, bound = G.channel_stats(x)
    cnt = N * H * W
    mean, var = stats[:Cc] / cnt, stats[Cc:] / cnt - (stats[:Cc] / cnt) ** 2
    _close(mean, x.double().mean((0, 2, 3)), "mean")
    _close(var, x.double().var((0, 2, 3), unbiased=False), "var")
    _close(bound[:Cc], x.double().abs().sum((0, 2, 3)), "absref")
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    _close(G.affine_act(x, gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd, None, None, None, 0)[0], z, "bn forward")
    b = G.affine_act_bwd(dz, None, x, None, None, None, None, None, None, mean, invstd, 0)
    _close(b["g"][0], dz, "act none: g = dz")
    s1, s2 = b["bstats"][0][:Cc], b["bstats"][0][Cc:]
    p = gamma.double() * invstd
    q = -p * invstd * s2 / cnt
    r = -p * s1 / cnt - q * mean
    dy, a = G.bn_bwd_apply(dz, x, torch.stack([p, q, r]))
    _close(dy, want, "bn backward")
    assert bool((a >= dy.abs() - 1e-15).all())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("res", ["none", "plain", "affine"])
def test_affine_act_and_backward_against_autograd(shape, act, res):
    Cc = shape[1]
    y, r, dz, dz2, add = (_rand(shape, s) for s in (1, 2, 3, 4, 5))
    sc, sh, rs, rh, mu, inv = (_rand((Cc,), s) for s in (6, 7, 8, 9, 10, 11))
    res_t = None if res == "none" else r
    rs_t, rh_t = (rs, rh) if res == "affine" else (None, None)
    yd = y.double().requires_grad_()
    pre = yd * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    if res == "plain":
        pre = pre + r.double()
    if res == "affine":
        pre = pre + r.double() * rs.double().view(1, -1, 1, 1) + rh.double().view(1, -1, 1, 1)
    z = _act64(pre, act)
    ref, a = G.affine_act(y, sc, sh, res_t, rs_t, rh_t, act)
    _close(ref, z, "forward")
    assert bool((a >= ref.abs() - 1e-15).all())
    pre_l = pre.detach().requires_grad_()
    (gpre,) = torch.autograd.grad(_act64(pre_l, act), pre_l, dz.double() + dz2.double())
    b = G.affine_act_bwd(dz, dz2, y, sc, sh, res_t, rs_t, rh_t, add, mu, inv, act)
    g = gpre + add.double()
    _close(b["g"][0], g, "backward")
    xhat = (y.double() - mu.double().view(1, -1, 1, 1)) * inv.double().view(1, -1, 1, 1)
    _close(b["bstats"][0], torch.cat([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))]), "bstats")
    assert bool((b["bstats"][1] >= b["bstats"][0].abs() - 1e-12).all())


def test_make_decidable_moves_every_undecidable_element():
    y = _rand((2, 3, 4, 5), 1)
    sc, sh = torch.tensor([1.0, 2.0, -1.0]), torch.tensor([0.5, -1.0, 0.25])
    y[0, 0, 0, 0], y[1, 1, 2, 3], y[1, 2, 3, 4] = -0.5, 0.5, 0.25 + 2.0 ** -24      # pre = 0, 0, -2^-24
    fn = lambda t: G.pre_act(t, sc, sh)
    assert int(G.undecidable(*fn(y)).sum()) == 3
    y2, moved = G.make_decidable(y, fn)
    assert moved == 3 and int(G.undecidable(*fn(y2)).sum()) == 0
    assert int((y2 != y).sum()) == 3 and float(y2[0, 0, 0, 0]) == 0.5


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 4, 6, 4), (1, 2, 1, 2), (2, 2, 2, 1)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_maxpool_and_backward_against_max_pool2d(shape, act):
    N, Cc, H, W = shape
    x, sc, sh = _rand(shape, 1), _rand((Cc,), 2), _rand((Cc,), 3)
    v = _act64(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), act).requires_grad_()
    want, widx = F.max_pool2d(v, 3, 2, 1, return_indices=True)
    for exact in (True, False):
        m = G.maxpool(x, sc, sh, act, exact)
        assert torch.equal(m["idx"], widx), exact
        assert float((m["y"][0] - want.detach()).abs().max()) <= (2.0 ** -23 if exact else 1e-14) * float(m["y"][1].max())
    dy = _rand(want.shape, 4)
    (gx,) = torch.autograd.grad(want, v, dy.double())
    dx, dxa = G.maxpool_bwd(dy, m["idx"], H, W)
    _close(dx, gx, "pool backward")
    assert bool((dxa >= dx.abs() - 1e-15).all())
    # ties: the first maximum in scan order wins
    ties = torch.zeros(1, 1, 4, 4)
    t = G.maxpool(ties, None, None, 0)
    assert t["tap"].tolist() == [[[[4, 3], [1, 0]]]] and t["idx"].tolist() == [[[[0, 1], [4, 5]]]]


@pytest.mark.parametrize("shape", SHAPES)
def test_stem_tail_backward_against_autograd(shape):
    """conv output -> BatchNorm (training) -> ReLU -> MaxPool(3, 2, 1): dL/dy from dL/d(pooled) through the folded form."""
    N, Cc, H, W = shape
    y, gamma, beta = _rand(shape, 1), _rand((Cc,), 2), _rand((Cc,), 3)
    bn = torch.nn.BatchNorm2d(Cc, eps=1e-5).double()
    bn.weight.data, bn.bias.data = gamma.double(), beta.double()
    yd = y.double().requires_grad_()
    pooled = F.max_pool2d(F.relu(bn(yd)), 3, 2, 1)
    g, g2 = _rand(pooled.shape, 4), _rand(pooled.shape, 5)
    (want,) = torch.autograd.grad(pooled, yd, g.double() + g2.double())
    cnt = N * H * W
    mean = y.double().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(y.double().var((0, 2, 3), unbiased=False) + 1e-5)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    idx = G.maxpool(y, scale, shift, 1, exact=False)["idx"]
    s = G.stem_tail_bwd(g, g2, idx, y, scale, shift, mean, invstd, None)["bstats"][0]
    q = -scale * invstd * s[Cc:] / cnt
    r = -scale * s[:Cc] / cnt - q * mean
    out = G.stem_tail_bwd(g, g2, idx, y, scale, shift, None, None, torch.stack([scale, q, r]))
    _close(out["dy"][0], want, "stem tail backward")
    assert bool((out["dy"][1] >= out["dy"][0].abs() - 1e-12).all())
    # the blocked tap image of the B16 kernels round-trips
    tap = torch.randint(0, 9, (2, 32, 3, 5), dtype=torch.uint8)
    assert torch.equal(G.blocked_to_nchw(G.nchw_to_blocked(tap)), tap)


@pytest.mark.parametrize("B,T,rest", [(2, 3, (4, 5, 6)), (3, 1, (2, 7, 3))])
def test_temporal_mean_against_autograd(B, T, rest):
    x = _rand((B * T,) + rest, 1)
    xd = x.double().requires_grad_()
    want = xd.view((B, T) + rest).mean(1)
    ref, a = G.temporal_mean(x, B, T)
    _close(ref.view(want.shape), want, "mean")
    dy = _rand(want.shape, 2)
    (gx,) = torch.autograd.grad(want, xd, dy.double())
    _close(G.temporal_mean_bwd(dy, B, T)[0].reshape(gx.shape), gx, "mean backward")
    assert bool((a >= ref.abs() - 1e-15).all())


@pytest.mark.parametrize("n,wd", [(37, 1e-4), (130, 0.0)])
def test_sgd_against_optim_sgd(n, wd):
    p0, g1, g2 = _rand((n,), 1), _rand((n,), 2), _rand((n,), 3)
    lr, mom = G.f32(1e-2), G.f32(0.9)
    par = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.SGD([par], lr=lr, momentum=mom, weight_decay=G.f32(wd))
    p, buf = p0.double(), torch.zeros(n, dtype=F64)
    for it, g in enumerate((g1, g2)):
        par.grad = g.double() * G.f32(0.5)
        opt.step()
        s = G.sgd(p, g, buf, lr, mom, wd, 0.5, first=(it == 0))
        p, buf = s["p"][0], s["buf"][0]
        _close(p, par.data, f"step {it}")
        _close(buf, opt.state[par]["momentum_buffer"], f"buffer {it}")
        assert bool((s["p"][1] >= p.abs() - 1e-15).all())


@pytest.mark.parametrize("shape,cp", [((2, 3, 6, 8), 16), ((1, 1, 2, 4), 4)])
def test_space_to_depth_is_the_stem_conv_in_stride_one(shape, cp):
    """conv 7x7 / s2 / p3 over x == conv 4x4 / s1 / p0 over space_to_depth2(x) with the re-indexed weight (csrc/ops.hip)."""
    N, Cc, H, W = shape
    x, w = _rand(shape, 1).double(), _rand((5, Cc, 7, 7), 2).double()
    xs, a = G.space_to_depth2(x, cp)
    w2 = torch.zeros(5, cp, 4, 4, dtype=F64)
    for dy in range(2):
        for dx in range(2):
            for a_ in range(4):
                for b_ in range(4):
                    kh, kw = 2 * a_ + dy - 1, 2 * b_ + dx - 1
                    if 0 <= kh < 7 and 0 <= kw < 7:
                        w2[:, (dy * 2 + dx) * Cc:(dy * 2 + dx + 1) * Cc, a_, b_] = w[:, :, kh, kw]
    _close(F.conv2d(xs, w2), F.conv2d(x, w, None, 2, 3), "stem")
    assert torch.equal(a, xs.abs())


def test_bf16_truncation_differs_from_rounding_and_half_ulp_gate_sees_it():
    x = _rand((1, 16, 3, 5), 1).double()
    t, r = G.truncate_bf16(x), R.bf16(x.float()).double()
    assert bool((t.abs() <= x.abs()).all()) and int((t != r).sum()) > 50
    img = G.b16_image(x.float())
    assert img.shape == (1, 1, 3, 5, 16) and float(img[0, 0, 2, 4, 7]) == float(r[0, 7, 2, 4])
    assert torch.equal(G.vals(img), r)                                    # B16 operands are taken at their bf16 values
    ok = R.check(img, x, x.abs(), 0.0, b16=True)[0]
    bad = R.check(t, x, x.abs(), 0.0, b16=True)[0]
    assert ok <= 1.0 < bad
