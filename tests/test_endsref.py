"""not-gpu: tests/endsref.py (the float64 references of the step-end kernels) against independent torch formulations —
F.grid_sample on the float64 warpgrid, F.binary_cross_entropy / l1_loss / mse_loss with autograd through the activations,
F.cosine_similarity, torch.bmm, oracle.nets.Fusion —, the decidability of every row of tests/ends_cases.py, the sensitivity of
every gate (an element moved by 8x its bound and a reference with one term dropped must both be rejected), and the argument
rejections of the launchers that return before any launch (the library loads without a device)."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ends_cases as S
import endsref as E
from recipes import lib as _lib

F64 = torch.float64
TOL = 1e-11


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, what="", tol=TOL):
    a, b = a.detach().to(F64), b.detach().to(F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (what, float((a - b).abs().max()))


def _warpgrid(bs, HO, WO, warp):
    """utils.py:12-26 of the reference: the float32 grid of the log-frequency warp."""
    x, y = np.linspace(-1, 1, WO), np.linspace(-1, 1, HO)
    xv, yv = np.meshgrid(x, y)
    gy = (np.power(21, (yv + 1) / 2) - 11) / 10 if warp else np.log(yv * 10 + 11) / np.log(21) * 2 - 1
    grid = np.zeros((bs, HO, WO, 2))
    grid[..., 0], grid[..., 1] = xv, gy
    return torch.from_numpy(grid.astype(np.float32)).to(F64)


# ---- references against independent formulations ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Hin,Win,Hout,Wout,warp", [(9, 7, 13, 5, 1), (13, 6, 9, 11, 0), (5, 1, 4, 1, 1), (64, 3, 256, 4, 1), (256, 2, 512, 3, 0)])
def test_warp_against_grid_sample(Hin, Win, Hout, Wout, warp):
    x = torch.randn(2, Hin, Win, generator=_g(1))
    ref, units = E.warp(x, Hout, Wout, warp)
    want = F.grid_sample(x.to(F64)[:, None], _warpgrid(2, Hout, Wout, warp), align_corners=False)[:, 0]
    _close(ref, want, "warp")
    assert bool((units >= E.K_BILIN * want.abs() - 1e-9).all())


@pytest.mark.parametrize("warp,weighted,binary", [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_prepare_against_grid_sample(warp, weighted, binary):
    Sn, B, Fin, T, Fout = 2, 2, 12, 9, (20 if warp else 12)
    g = _g(2)
    mags = torch.randn(Sn, B, Fin, T, generator=g).abs()
    mix = mags.sum(0) * (0.5 + torch.rand(B, Fin, T, generator=g))
    r = E.prepare(mix, mags, warp, weighted, binary, Fout)
    m64, s64 = mix.to(F64) + E.EPS_MIX, mags.to(F64)
    if warp:
        grid = _warpgrid(B, Fout, T, True)
        m64 = F.grid_sample(m64[:, None], grid, align_corners=False)[:, 0]
        s64 = torch.stack([F.grid_sample(s64[n][:, None], grid, align_corners=False)[:, 0] for n in range(Sn)])
    _close(r["mag_mix"][0], m64, "mix")
    _close(r["mags"][0], s64, "mags")
    _close(r["log_mag_mix"][0], torch.log(m64), "log")
    _close(r["weight"][0], torch.log1p(m64).clamp(E.f32(1e-3), 10) if weighted else torch.ones_like(m64), "weight")
    _close(r["gt"][0], (s64 > 0.5 * m64).to(F64) if binary else (s64 / m64).clamp(0, 5), "gt")


_ACT = {0: lambda l: l, 1: torch.relu, 3: torch.sigmoid, 4: torch.tanh, 5: lambda l: torch.softmax(l, 1)}


@pytest.mark.parametrize("act,loss", [(3, 0), (5, 0), (0, 0), (0, 1), (1, 1), (3, 1), (4, 1), (5, 1), (0, 2), (1, 2), (3, 2), (4, 2), (5, 2)])
@pytest.mark.parametrize("wkind", [None, "shared", "target"])
def test_mask_loss_against_torch_losses(act, loss, wkind):
    B, Sn, FT = 2, 3, 11
    g = _g(act * 10 + loss)
    logits = torch.rand(B, Sn, FT, generator=g) * 0.9 + 0.05 if (act, loss) == (0, 0) else torch.randn(B, Sn, FT, generator=g) * 2
    gt = (torch.rand(Sn, B, FT, generator=g) > 0.5).float()
    w = {None: None, "shared": torch.rand(B, FT, generator=g), "target": torch.rand(Sn, B, FT, generator=g)}[wkind]
    coef = torch.randn(B, Sn, Sn, generator=g)
    l64 = logits.to(F64).requires_grad_(True)
    p = _ACT[act](l64)
    fn = {0: F.binary_cross_entropy, 1: F.l1_loss, 2: F.mse_loss}[loss]
    rows = []
    for i in range(Sn):
        wi = torch.ones(B, FT, dtype=F64) if w is None else (w if w.dim() == 2 else w[i]).to(F64)
        rows.append(torch.stack([(wi * fn(p[:, j], gt[i].to(F64), reduction="none")).sum(-1) for j in range(Sn)], 1))
    want = torch.stack(rows, 1)                                                   # [B, i, j]
    pr, pu = E.activation(logits, act)
    _close(pr, p, "pred")
    sums, bound = E.mask_loss_sums(pr, gt, w, loss)
    _close(sums, want, "sums")
    assert bool((bound >= want.abs() - 1e-9).all()) and bool((pu >= 0).all())
    (grad,) = torch.autograd.grad((coef.to(F64) * want).sum(), l64)
    ref, units, _ = E.mask_loss_bwd(logits, gt, w, coef, act, loss)
    _close(ref, grad, "dlogits")
    assert bool((units >= E.K["mask_loss_bwd"](act) * ref.abs() * (1 - 1e-9) - 1e-9).all())


def test_mask_loss_saturation_follows_the_kernel_clamps():
    """pred == 1.0f: log(1 - p) = -inf clamps to -100 (binary_cross_entropy's own rule), staged on the fp32 pred."""
    pred = torch.tensor([[[1.0, 0.0, 0.5]]])
    gt = torch.tensor([[[0.0, 1.0, 1.0]]])
    sums, bound = E.mask_loss_sums(pred, gt, None, E.BCE)
    want = F.binary_cross_entropy(pred.double(), gt.double().permute(1, 0, 2), reduction="sum")
    _close(sums.reshape(()), want)
    assert bool(torch.isfinite(bound).all())


@pytest.mark.parametrize("with_scale", [True, False])
def test_innerprod_against_bmm_and_autograd(with_scale):
    B, Kc, P, HW = 2, 6, 5, 9
    g = _g(5)
    img, imgs, snd = (torch.randn(s, generator=g) for s in ((B, Kc), (B, Kc, P), (B, Kc, HW)))
    scale, bias, dz = (torch.rand(Kc, generator=g) + 0.5 if with_scale else None), torch.randn(1, generator=g), torch.randn(B, HW, generator=g)
    i64, s64, b64 = img.to(F64).requires_grad_(True), snd.to(F64).requires_grad_(True), bias.to(F64).requires_grad_(True)
    sc64 = scale.to(F64).requires_grad_(True) if with_scale else None
    w = i64 * sc64 if with_scale else i64
    z = torch.bmm(w[:, None], s64)[:, 0] + b64
    ref, a = E.innerprod_fwd(img, snd, scale, bias)
    _close(ref, z, "fwd")
    assert bool((a >= z.abs() - 1e-12).all())
    _close(E.innerprod_nosum(img, snd, scale, bias)[0], w[..., None] * s64 + b64, "nosum")
    wi = imgs.to(F64).transpose(1, 2) * (sc64 if with_scale else 1.0)
    _close(E.innerprod_pixelwise(imgs, snd, scale, bias)[0], torch.bmm(wi, s64) + b64, "pixelwise")
    grads = torch.autograd.grad(z, [i64, s64, b64] + ([sc64] if with_scale else []), dz.to(F64))
    r = E.innerprod_bwd(img, snd, scale, dz)
    _close(r["dimg"][0], grads[0], "dimg"); _close(r["dsnd"][0], grads[1], "dsnd"); _close(r["dbias"][0], grads[2], "dbias")
    if with_scale:
        _close(r["dscale"][0], grads[3], "dscale")


def test_sdr_sums_against_float64_sums():
    g = _g(6)
    est, ref = torch.randn(3, 1000, generator=g), torch.randn(3, 1000, generator=g)
    s, a = E.sdr_sums(est, ref)
    e, r = est.to(F64), ref.to(F64)
    _close(s, torch.stack([(e * r).sum(1), (r * r).sum(1), (e * e).sum(1)], 1), "sums", 1e-13)
    assert bool((a >= s.abs()).all())


def _oracle_fusion(kind, att, x4, vs4):
    from oracle import nets as O
    net = O.Fusion({0: "hidsep", 1: "CoLoc_Sel", 2: "MixVis"}[kind], "cos" if att == 0 else "sig")
    return net(x4, vs4)


@pytest.mark.parametrize("att", [0, 1])
@pytest.mark.parametrize("kind,C", [(0, 2), (1, 2), (2, 1), (0, 3), (0, 4)])
def test_fusion_against_oracle_fusion(kind, C, att):
    """Values and float64 autograd gradients of oracle.nets.Fusion (_coloc, _coloc_n, _mixvis) on a draw without ties; the
    absrefs dominate their references."""
    B, Dc, H, W, Fq, T = 3, 5, 3, 4, 2, 3
    Ka = 2 if kind == 2 else C
    D = Ka * Dc + (2 if C > 2 else 0)
    g = _g(kind * 7 + C + att)
    x = torch.randn(B, D, Fq * T, generator=g)
    vs = [torch.randn(B, Dc, H * W, generator=g) for _ in range(C)]
    f = E.fusion_fwd(x, vs, kind, att, grad=True)
    x4 = x.to(F64).view(B, D, Fq, T).requires_grad_(True)
    vs4 = [v.to(F64).view(B, Dc, H, W).requires_grad_(True) for v in vs]
    y, (match, attm) = _oracle_fusion(kind, att, x4, vs4)
    _close(f.feat, y[:, :D, 0, 0], "feat")
    _close(f.match.mean().reshape(-1), match.reshape(-1), "match")
    _close(f.att_maps, attm.reshape(B, -1, H * W), "att maps")
    assert bool((f.feata >= f.feat.abs() - 1e-12).all()) and bool((f.matcha >= f.match.abs() - 1e-12).all())
    assert bool((f.att_mapsa >= f.att_maps.abs() - 1e-12).all())
    dfeat, dmaps, dm = torch.randn(B, D, generator=g), (torch.randn(B, Ka if kind == 2 else C, H * W, generator=g) if C == 2 or kind == 2 else None), 0.7
    L = (y[:, :D, 0, 0] * dfeat.to(F64)).sum() + dm * B * match.sum()
    if dmaps is not None:
        L = L + (attm.reshape(B, -1, H * W) * dmaps.to(F64)).sum()
    grads = torch.autograd.grad(L, [x4] + vs4)
    r = E.fusion_bwd(f, dfeat, dmaps, dm)
    _close(r["dx"][0], E.take(grads[0].reshape(B, D, -1), f.pool_idx), "dx")
    _close(r["dv"][0], torch.stack([t.reshape(B, Dc, H * W) for t in grads[1:]], 1), "dv")
    for n in ("dx", "dv"):
        assert bool((r[n][1] >= r[n][0].abs() * (1 - 1e-9) - 1e-12).all()), n


def test_fusion_ao_against_oracle():
    from oracle import nets as O
    g = _g(9)
    x = torch.randn(4, 10, 6, generator=g)
    for draws, allz in ((torch.tensor([1, 0, 1, 0], dtype=torch.uint8), False), (torch.zeros(4, dtype=torch.uint8), True)):
        feat, _, src = E.fusion_ao(x, draws, 2, allz)
        _close(feat, O.ao_swap(x.to(F64).view(4, 10, 2, 3), draws.bool())[:, :10, 0, 0], "ao_swap")
    x = torch.randn(6, 11, 6, generator=g)
    draws = torch.arange(6, dtype=torch.int32)
    feat, pool_idx, src = E.fusion_ao(x, draws, 3)
    x4 = x.to(F64).view(6, 11, 2, 3).requires_grad_(True)
    y = O.ao_permute_n(x4, draws, 3)[:, :11, 0, 0]
    _close(feat, y, "ao_permute_n")
    dfeat = torch.randn(6, 11, generator=g)
    (gx,) = torch.autograd.grad((y * dfeat.to(F64)).sum(), x4)
    _close(E.fusion_ao_bwd(src, dfeat)[0], E.take(gx.reshape(6, 11, 6), pool_idx), "ao dx")


@pytest.mark.parametrize("att", [0, 1])
def test_attention_against_cosine_similarity(att):
    B, Sn, Kc, HW = 2, 3, 6, 10
    g = _g(11 + att)
    a, mix = torch.randn(B, Sn, Kc, generator=g), torch.randn(B, Kc, HW, generator=g)
    a64, m64 = a.to(F64).requires_grad_(True), mix.to(F64).requires_grad_(True)
    a5, v5 = a64[..., None], m64[:, None]
    maps = F.cosine_similarity(a5, v5, dim=2) if att == 0 else torch.sigmoid(torch.sum(a5 * v5 / Kc ** 0.5, dim=2))
    match = -maps.mean(-1).sum(-1)
    mc = maps.clamp(0, 1)
    ctx = (m64[:, None] * mc[:, :, None]).mean(-1)
    f = E.attention_fwd(a, mix, att, grad=True)
    _close(f.m, maps, "maps"); _close(f.match, match, "match"); _close(f.ctx, ctx, "ctx")
    dctx, dmaps, dmatch = torch.randn(B, Sn, Kc, generator=g), torch.randn(B, Sn, HW, generator=g), torch.randn(B, generator=g)
    want = torch.autograd.grad((ctx * dctx).sum() + (mc * dmaps).sum() + (match * dmatch).sum(), [a64, m64])
    r = E.attention_bwd(f, dctx, dmaps, dmatch)
    _close(r["da"][0], want[0], "da"); _close(r["dmix"][0], want[1], "dmix")
    for n in ("da", "dmix"):
        assert bool((r[n][1] >= r[n][0].abs() * (1 - 1e-9) - 1e-12).all()), n


def test_first_index_wins_every_tie():
    t = torch.tensor([[1.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0]], dtype=F64)
    idx, margin = E.first_argmax(t)
    assert idx.tolist() == [1, 0] and margin.tolist() == [1.0, float("inf")]


# ---- the rows ------------------------------------------------------------------------------------------------------------------
def _id(row):
    return f"{row['op']}-{row['id']}"


_HOST_ROWS = [r for r in S.ROWS]


@pytest.mark.parametrize("row", _HOST_ROWS, ids=_id)
def test_row_is_decidable_and_within_the_size_limit(row):
    """Every decision of every row has a margin beyond the fp32 bound of what it compares (ends_cases draws and resamples); the
    warped binary masks, which cannot be resampled, exclude at most 1e-4 of their elements by the reference alone."""
    assert S.largest_tensor(row) < S.SIZE_LIMIT and row["note"]
    inp = S.inputs(row)                  # raises when no decidable draw exists
    op = row["op"]
    if op == "mask_loss" and not row.get("fwd_only"):
        assert not bool(S.mask_loss_undecided(*inp, S.A[row["act"]], S.Ls[row["loss"]]).any())
    if op == "prepare" and row["binary"]:
        m, s = E.prepare(*inp, row["warp"], row["weighted"], 1, row["Fout"])["gt_margin"]
        share = float((m <= E.U * s).double().mean())
        assert share <= (1e-4 if row["warp"] else 0.0), share
    if op in ("fusion_av", "fusion_n_av"):
        x, vs = inp[0], inp[1]
        f = E.fusion_fwd(x, vs, row.get("kind", 0), row["att"])
        for name, (m, s) in f.margins.items():
            assert bool(E.decided(m, s).all()), name
        sp = row["special"]
        if sp == "tie_cols":                        # the tie is where the row says: both columns carry the maximum of map (0, 0)
            h1 = row["HW"] // 3
            assert bool((f.arg[:, 0, 0] == h1).all()) and bool((f.m[:, 0, 0, h1] == f.m[:, 0, 0, h1 + 5]).all())
        if sp == "equal_maps":
            assert bool((f.best == 0).all()) and bool(torch.isinf(f.margins["best permutation"][0]).all())
        if sp == "zero_channel":
            assert bool((f.sel[:, 1] == 0).all())
        if sp == "zero_sel":
            assert bool((f.nu == E.EPS_COS).all()) and bool((f.nw == E.EPS_COS).all())
    if op == "attention":
        f = E.attention_fwd(inp[0], inp[1], row["att"])
        assert all(bool(E.decided(m, s).all()) for m, s in f.margins.values())
        if row["att"] == 0 and row["special"] is None:
            assert bool((f.m < 0).any()) and bool((f.m > 0).any())          # the clamp's lower branch on both sides


def test_every_form_of_the_issue_has_a_row():
    ids = {_id(r) for r in S.ROWS}
    assert len(ids) == len(S.ROWS)
    fav = S.cases("fusion_av")
    assert {(r["kind"], r["att"]) for r in fav} == set(itertools.product(range(3), range(2)))
    parts = {min(1 if r["B"] >= 256 else (2 if r["B"] >= 128 else 4), r["Dc"]) for r in fav}
    assert parts == {1, 2, 3, 4}
    assert any(4 * (4 * r["Dc"] + 10 * r["HW"] + 44) > 65536 for r in fav)
    assert any(r["K"] * (32 * E.cdiv(r["P"], 32) + 1) * 4 > 65536 for r in S.cases("innerprod_pixelwise"))
    assert any(4 * (r["D"] + (2 * r["C"] ** 2 + r["C"]) * r["HW"] + 61) > 65536 for r in S.cases("fusion_n_av"))
    ml = S.cases("mask_loss")
    assert {r["S"] for r in ml} == {1, 2, 3, 4} and {r["coef"] for r in ml} == set(S._COEF) and {r["weight"] for r in ml} == set(S._WEIGHT)
    assert any(E.loss_iters(r["FT"]) > 1 and E.cdiv(r["FT"], 1024) > 64 for r in ml)
    assert {r["S"] for r in S.cases("prepare")} == {1, 2, 3, 4} and {r["T"] for r in S.cases("prepare")} == {1, 255, 257, 600}
    assert {r["C"] for r in S.cases("fusion_n_av")} == {2, 3, 4} and {r["C"] for r in S.cases("fusion_n_ao")} == {2, 3, 4}
    assert {r["S"] for r in S.cases("attention")} == {1, 2, 4} and {r["K"] for r in S.cases("attention")} >= {1, 7, 128}


# ---- sensitivity of the gates ----------------------------------------------------------------------------------------------------
def _smallest(op):
    return min(S.cases(op), key=S.largest_tensor)


def _drop_one_term(row, inp):
    """The operands of `row` with one term of the formula removed: what a kernel that forgets it would compute."""
    op = row["op"]
    if op == "warp":
        inp = inp.clone()
        inp[:, -1] = 0.0                                                       # one input row
        return inp
    inp = [t.clone() if torch.is_tensor(t) else ([u.clone() for u in t] if isinstance(t, list) else t) for t in inp]
    if op == "mask_loss":
        inp[3][:, 0, -1] = 0.0 if row["S"] > 1 else inp[3][:, 0, -1] * 0.5    # one off-diagonal coef entry
        inp[1][-1] = 1.0 - inp[1][-1]                                          # and one source's targets (the sums)
    elif op == "prepare":
        inp[1][-1] = 0.0                                                       # one source
    elif op.startswith("innerprod"):
        inp[1][:, -1] = 0.0                                                    # one channel k
    elif op == "sdr_sums":
        inp = [inp[0].clone(), inp[1].clone()]
        inp[0][:, -1] = 0.0
        inp[1][:, -1] = 0.0
    elif op in ("fusion_av", "fusion_n_av"):
        inp[1][-1][:, -1] = 0.0                                                # one channel of the last visual map
    elif op in ("fusion_ao", "fusion_n_ao"):
        inp[2][:, 0] = 0.0
        inp[0][:, 0] = 0.0
    elif op == "attention":
        inp[1][:, -1] = 0.0
        inp[2][:, :, -1] = 0.0
    return tuple(inp)


@pytest.mark.parametrize("op", S.OPS)
def test_gate_rejects_a_moved_element_and_a_dropped_term(op):
    """On the smallest row of every launcher: the reference itself passes its gate; the reference with its largest-absref element
    moved by 8x its bound does not; nor does the reference of the same operands with one term dropped."""
    row = _smallest(op)
    inp = S.inputs(row)
    exp = S.expected(row, inp)
    other = S.expected(row, _drop_one_term(row, inp))
    caught = 0
    for name, val in exp.items():
        if name.startswith(("=", "excluded:")):
            continue
        ref, absref, k, unit = val
        assert E.gate(ref, ref, absref, k, unit)[0] == 0
        bound = (k * unit * absref).reshape(-1)
        i = int(torch.argmax(absref.reshape(-1)))
        moved = ref.clone().reshape(-1)
        step = 8.0 * float(bound[i])
        if step == 0.0:                      # an exact output: one fp32 ulp
            step = float(torch.nextafter(moved[i].float().abs(), torch.tensor(float("inf")))) - abs(float(moved[i].float()))
        moved[i] += step
        assert E.gate(moved.reshape(ref.shape), ref, absref, k, unit)[0] == 1, (name, "a moved element passed")
        caught += E.gate(other[name][0], ref, absref, k, unit)[0] > 0
    assert caught > 0, "the dropped term passed every gate"


def test_gate_rejects_one_zeroed_slice_of_the_fusion_backward():
    """fusion_av_bwd splits the channels over `parts` workgroups: dv and dx with the slice of one part left at zero are rejected,
    also where the slice is small against the largest element (the selected positions carrying dfeat)."""
    row = next(r for r in S.cases("fusion_av") if r["id"] == "Dc10-slices")
    exp = S.expected(row, S.inputs(row))
    Dc = row["Dc"]
    for part in range(4):
        lo, hi = Dc * part // 4, Dc * (part + 1) // 4
        ref, absref, k, unit = exp["dv"]
        t = ref.clone()
        t[:, :, lo:hi] = 0.0
        assert E.gate(t, ref, absref, k, unit)[0] > 0, part
        ref, absref, k, unit = exp["dx"]
        t = ref.clone()
        t[:, lo:hi] = 0.0
        assert E.gate(t, ref, absref, k, unit)[0] > 0, part


# ---- argument rejections that return before any launch ----------------------------------------------------------------------------
DUMMY = 256          # a non-null address: these calls only check that it is set


def test_launchers_reject_bad_arguments_before_launching():
    L, P, ERR = _lib(), DUMMY, -1
    # fusion_av: (4 Dc + 10 HW + 44) * 4 bytes of LDS > 160 KB
    assert 4 * (4 * 16 + 10 * 4100 + 44) > 160 * 1024
    assert L.avsep_fusion_av_fwd(P, P, P, 2, 16, 4, 4100, 0, 0, P, P, P, P, P, P, P, None) == ERR
    assert L.avsep_fusion_av_bwd(P, P, P, 2, 16, 4, 4100, 0, 0, P, P, P, P, P, P, None, None, 0.5, P, P, P, None) == ERR
    # fusion_n: (D + (2 C C + C) HW + 61) * 4 > 160 KB
    assert 4 * (64 + 36 * 1200 + 61) > 160 * 1024
    arr = (ctypes.c_void_p * 4)(P, P, P, P)
    assert L.avsep_fusion_n_av_fwd(P, arr, 2, 4, 64, 4, 1200, 0, P, P, P, P, P, P, P, None) == ERR
    assert L.avsep_fusion_n_av_bwd(P, arr, 2, 4, 64, 4, 1200, 0, P, P, P, P, P, None, 0.5, P, arr, None) == ERR
    # pixelwise: odd K; K * (roundup(P, 32) + 1) * 4 > 160 KB
    assert L.avsep_innerprod_pixelwise(P, P, P, P, 2, 3, 4, 4, P, None) == ERR
    assert L.avsep_innerprod_pixelwise(P, P, P, P, 2, 512, 128, 4, P, None) == ERR
    # attention: S = 5, K = 129, HW = 4097
    for Sn, Kc, HW in ((5, 8, 16), (2, 129, 16), (2, 8, 4097)):
        assert L.avsep_attmodel_infer_fwd(P, P, 2, Sn, Kc, HW, 0, P, P, P, None) == ERR
        assert L.avsep_attmodel_infer_bwd(P, P, P, P, P, P, 2, Sn, Kc, HW, 0, P, P, None) == ERR
    # prepare: no warp with Fout != Fin; S = 5
    assert L.avsep_prepare(P, P, 2, 2, 8, 4, 9, 0, 1, 1, P, P, P, P, P, None) == ERR
    assert L.avsep_prepare(P, P, 5, 2, 8, 4, 8, 0, 1, 1, P, P, P, P, P, None) == ERR
