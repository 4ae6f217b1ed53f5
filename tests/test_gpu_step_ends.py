"""-m gpu: the kernels at the two ends of the train step alone — spectrogram preparation (avsep_prepare, avsep_warp), the
bottleneck (avsep_fusion_av_*, avsep_fusion_ao_*, avsep_fusion_n_*, avsep_attmodel_infer_*), the mask synthesizer
(avsep_innerprod_*) and the loss (avsep_mask_loss_*, avsep_sdr_sums) — at the rows of tests/ends_cases.py, against the float64
references of tests/endsref.py, element by element: |out - ref| <= k * 2^-24 * absref (2^-53 for the fp64 SDR sums); an
element whose absref is 0 must equal ref exactly; integer outputs (pool_idx, sel_idx, best) must be equal.

k per launcher is endsref.K: counted from the source lines named there, not measured; the worst measured ratio per launcher and
form is printed as one table at the end of the run (pytest -s) and copied into the comments of K and into DESIGN.md §20.
Nothing is excluded but elements of a WARPED binary mask whose float64 margin |src - 0.5 mix| lies inside its own bound (at most
1e-4 of a mask; tests/test_endsref.py shows that the rows stay within that by the reference alone): every other decision of
every row is decidable by construction (ends_cases draws and resamples on the CPU).

Each launcher is called through the Python entry the model uses, or through lib.call where that entry fixes an argument (the
fusion wrapper never passes dmaps, evaluate.sdr_sums takes dense rows only)."""
import pytest
import torch

import ends_cases as S
import endsref as E
from recipes import pkg as _pkg

pytestmark = pytest.mark.gpu
F64 = torch.float64
_TABLE = {}          # (launcher, form) -> [rows, worst ratio, excluded elements]


def _id(row):
    return row["id"]


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\nstep ends | launcher | form | rows | worst ratio | excluded elements")
    for (launcher, form), (rows, worst, nex) in sorted(_TABLE.items()):
        print(f"step ends | {launcher} | {form} | {rows} | {worst:.3f} | {nex}")


def _check(row, launcher, form, outs, exp):
    """Gate every output of `outs` (name -> tensor) against exp (ends_cases.expected)."""
    worst, nex = 0.0, 0
    for name, out in outs.items():
        if name.startswith("="):
            want = exp[name]
            assert torch.equal(out.long().reshape(want.shape), want.long()), (row["id"], name, int((out.long().reshape(want.shape) != want).sum()))
            continue
        ref, absref, k, unit = exp[name]
        excluded = exp.get("excluded:" + name)
        bad, ratio, i = E.gate(out, ref, absref, k, unit, excluded)
        n = int(excluded.sum()) if excluded is not None else 0
        if excluded is not None:
            assert n <= 1e-4 * excluded.numel(), (row["id"], name, n)
        print(f"step ends | {launcher} | {form} | {row['id']} | {name} | k={k} | worst ratio {ratio:.3f} (at {i}: out "
              f"{float(out.reshape(-1)[i]):.9g} ref {float(ref.reshape(-1)[i]):.9g} absref {float(absref.reshape(-1)[i]):.3g}) | excluded {n}")
        assert bad == 0, (row["id"], name, bad, ratio, i)
        worst, nex = max(worst, ratio), nex + n
    t = _TABLE.setdefault((launcher, form), [0, 0.0, 0])
    t[0], t[1], t[2] = t[0] + 1, max(t[1], worst), t[2] + nex


def _dev(dev, *ts):
    return S._to(dev, *ts)


def _ptr(t):
    return None if t is None else _pkg().lib.ptr(t)


# ---- loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.cases("mask_loss"), ids=_id)
def test_mask_loss(row, dev):
    """avsep_mask_loss_fwd and _bwd through models.criterion.mask_loss: pred against the float64 activation, the loss sums
    against float64 on the kernel's own pred, dlogits (the cotangent of sums is the row's coef) against float64 autograd."""
    from avsep_amd.models.criterion import mask_loss
    inp = S.inputs(row)
    logits, gt, weight, coef = _dev(dev, *inp)
    x = logits.clone().requires_grad_(not row.get("fwd_only"))
    pred, sums, FT = mask_loss(x, gt, weight, S.A[row["act"]], row["loss"])
    assert FT == row["FT"] and sums.dtype == F64
    outs = {"pred": pred.detach(), "sums": sums.detach()}
    if not row.get("fwd_only"):
        (sums * coef.to(F64)).sum().backward()
        outs["dlogits"] = x.grad
    exp = S.expected(row, inp, dev, pred=pred.detach())
    _check(row, "mask_loss", f"{row['act']}+{row['loss']}", outs, exp)


@pytest.mark.parametrize("row", S.cases("sdr_sums"), ids=_id)
def test_sdr_sums(row, dev):
    P = _pkg()
    inp = S.inputs(row)
    R_, L = row["R"], row["L"]
    est = torch.empty((R_, L + row["pad"]), device=dev)[:, :L].copy_(inp[0])
    ref = torch.empty((R_, L + 2 * row["pad"]), device=dev)[:, :L].copy_(inp[1])
    if row["pad"]:           # evaluate.sdr_sums takes dense rows only
        sums = torch.zeros((R_, 3), dtype=F64, device=dev)
        P.lib.call("avsep_sdr_sums", est.data_ptr(), ref.data_ptr(), R_, L, est.stride(0), ref.stride(0), _ptr(sums))
    else:
        from avsep_amd import evaluate
        sums = evaluate.sdr_sums(est, ref)
    _check(row, "sdr_sums", "strided rows" if row["pad"] else "dense rows", {"sums": sums}, S.expected(row, inp, dev))


# ---- preparation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.cases("prepare"), ids=_id)
def test_prepare(row, dev):
    inp = S.inputs(row)
    mix, mags = _dev(dev, *inp)
    mix_w, mags_w, logm, weight, gt = _pkg().kernels.prepare(mix[:, None].contiguous(), mags[:, :, None].contiguous(), row["warp"],
                                                             row["weighted"], row["binary"], fout=row["Fout"])
    outs = {"mag_mix": mix_w[:, 0], "mags": mags_w[:, :, 0], "log_mag_mix": logm[:, 0], "weight": weight[:, 0], "gt": gt[:, :, 0]}
    form = ("warp" if row["warp"] else "no warp") + (", binary" if row["binary"] else ", ratio")
    _check(row, "prepare", form, outs, S.expected(row, inp, dev))


@pytest.mark.parametrize("row", S.cases("warp"), ids=_id)
def test_warp(row, dev):
    inp = S.inputs(row)
    (x,) = _dev(dev, inp)
    y = _pkg().kernels.warp(x[None].contiguous(), row["Hout"], row["Wout"], row["warp"])[0]
    _check(row, "warp", "warp" if row["warp"] else "un-warp", {"y": y}, S.expected(row, inp, dev))


# ---- synthesizer -----------------------------------------------------------------------------------------------------------------
def _synth(row, scale, bias, dev):
    M = _pkg().models.synthesizer_net
    mod = M.InnerProd(row["K"]) if scale is not None else M.Bias()
    with torch.no_grad():
        if scale is not None:
            mod.scale.copy_(scale)
        mod.bias.copy_(bias if bias is not None else torch.zeros(1))
    return mod.to(dev)


@pytest.mark.parametrize("row", S.cases("innerprod_fwd") + S.cases("innerprod_nosum") + S.cases("innerprod_pixelwise"), ids=lambda r: f"{r['op']}-{r['id']}")
def test_innerprod_forward_forms(row, dev):
    """InnerProd / Bias .forward, .forward_nosum and .forward_pixelwise without autograd: the three forward kernels.  A row
    without bias runs the module's zero bias (the kernel adds 0.f: exact)."""
    inp = S.inputs(row)
    img, snd, scale, bias, _ = _dev(dev, *inp)
    mod = _synth(row, scale, bias, dev)
    B, Kc, HW = row["B"], row["K"], row["HW"]
    with torch.no_grad():
        if row["op"] == "innerprod_fwd":
            z, form = mod(img.view(B, Kc, 1, 1), snd.view(B, Kc, 1, HW)).view(B, HW), "gemv"
        elif row["op"] == "innerprod_nosum":
            z, form = mod.forward_nosum(img.view(B, Kc, 1, 1), snd.view(B, Kc, 1, HW)).view(B, Kc, HW), ("vec4" if HW % 4 == 0 else "scalar")
        else:
            P = row["P"]
            z = mod.forward_pixelwise(img.view(B, Kc, 1, P), snd.view(B, Kc, 1, HW)).view(B, P, HW)
            form = "mfma" + (", LDS > 64 KB" if Kc * (32 * E.cdiv(P, 32) + 1) * 4 > 65536 else "")
    _check(row, row["op"], form, {"z": z}, S.expected(row, inp, dev))


@pytest.mark.parametrize("row", S.cases("innerprod_bwd"), ids=_id)
def test_innerprod_backward(row, dev):
    """avsep_innerprod_bwd through _InnerProdFn.backward: dsnd and r (= dimg for Bias) from the kernel, and dimg, dscale, dbias as
    the autograd node forms them; the null-dsnd form is the call autograd makes when the sound features need no gradient, and r
    itself is read from a direct call."""
    P = _pkg()
    inp = S.inputs(row)
    img, snd, scale, bias, dz = _dev(dev, *inp)
    mod = _synth(row, scale, bias, dev)
    B, Kc, HW = row["B"], row["K"], row["HW"]
    a, s = img.clone().requires_grad_(True), snd.clone().requires_grad_(row["dsnd"])
    z = mod(a.view(B, Kc, 1, 1) if row["dsnd"] else a, s.view(B, Kc, 1, HW))      # [B, K, 1, 1] as forward_nosum takes it, or [B, K]
    z.backward(dz.view(z.shape))
    outs = {"dimg": a.grad, "dbias": mod.bias.grad}
    if row["dsnd"]:
        outs["dsnd"] = s.grad
    if row["scale"]:
        outs["dscale"] = mod.scale.grad
    r = torch.empty((B, Kc), device=dev)
    dsnd = torch.empty_like(snd) if row["dsnd"] else None
    P.lib.call("avsep_innerprod_bwd", _ptr(img), _ptr(snd), _ptr(scale), _ptr(dz), B, Kc, HW, _ptr(dsnd), _ptr(r))
    outs["r"] = r
    if row["dsnd"]:
        assert torch.equal(dsnd, s.grad)
    form = ("dsnd" if row["dsnd"] else "no dsnd") + (", scale" if row["scale"] else ", no scale")
    _check(row, "innerprod_bwd", form, outs, S.expected(row, inp, dev))


# ---- bottleneck --------------------------------------------------------------------------------------------------------------------
def _parts(B, Dc):
    return min(1 if B >= 256 else (2 if B >= 128 else 4), Dc)


@pytest.mark.parametrize("row", S.cases("fusion_av"), ids=_id)
def test_fusion_av(row, dev):
    """avsep_fusion_av_fwd and _bwd by lib.call (models/fusion_net.py passes no dmaps): every output of the forward, then the
    backward on the forward's own outputs with cotangents on feat, the attention maps and the match term; dx is accumulated
    into a random prefill, of which every element but the pooled positions must come back bit for bit."""
    P = _pkg()
    inp = S.inputs(row)
    x, vs, dfeat, dmaps, dmatch, prefill = _dev(dev, *inp)
    B, Dc, HW, FT, kind, att = row["B"], row["Dc"], row["HW"], row["FT"], row["kind"], row["att"]
    D = 2 * Dc
    v0, v1 = vs[0], vs[-1]
    f32 = lambda *s: torch.empty(s, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    a_pool, pool_idx, feat, sel_idx, maps, match, best = f32(B, D), i32(B, D), f32(B, D), i32(B, D), f32(B, 2, HW), f32(B), i32(B)
    P.lib.call("avsep_fusion_av_fwd", _ptr(x), _ptr(v0), _ptr(v1), B, Dc, FT, HW, kind, att, _ptr(a_pool), _ptr(pool_idx), _ptr(feat),
               _ptr(sel_idx), _ptr(maps), _ptr(match), _ptr(best))
    null = row["null"]
    dx = None if null == "dx" else prefill.clone()
    dv0 = None if null == "dv0" else torch.full((B, Dc, HW), float("nan"), device=dev)
    dv1 = None if (null == "dv1" or kind == 2) else torch.full((B, Dc, HW), float("nan"), device=dev)
    P.lib.call("avsep_fusion_av_bwd", _ptr(x), _ptr(v0), _ptr(v1), B, Dc, FT, HW, kind, att, _ptr(a_pool), _ptr(pool_idx), _ptr(sel_idx),
               _ptr(maps), _ptr(best), _ptr(dfeat), _ptr(dmaps), _ptr(dmatch), 1.0 / B, _ptr(dx), _ptr(dv0), _ptr(dv1))
    exp = S.expected(row, inp, dev)
    outs = {"a_pool": a_pool, "=pool_idx": pool_idx, "=sel_idx": sel_idx, "=best": best, "att_maps": maps, "match_part": match, "feat": feat}
    _check(row, "fusion_av_fwd", f"{S._KN[kind]}, {S._AN[att]}" + (", LDS > 64 KB" if 4 * (4 * Dc + 10 * HW + 44) > 65536 else ""), outs, exp)
    outs = {}
    if dx is not None:
        at = exp["=pool_idx"]
        outs["dx"] = E.take(dx, at)
        untouched = torch.ones_like(dx, dtype=torch.bool).scatter_(2, at[..., None], False)
        assert torch.equal(dx[untouched], prefill[untouched])
    ref, absref, k, unit = exp["dv"]
    if kind == 2:
        outs["dv"] = dv0[:, None] if dv0 is not None else None
    else:
        have = [c for c, t in enumerate((dv0, dv1)) if t is not None]
        outs["dv"] = torch.stack([t for t in (dv0, dv1) if t is not None], 1)
        exp["dv"] = (ref[:, have], absref[:, have], k, unit)
    if outs["dv"] is None:
        del outs["dv"]
    _check(row, "fusion_av_bwd", f"{S._KN[kind]}, {S._AN[att]}, parts {_parts(B, Dc)}" + (f", {null} null" if null else ""), outs, exp)


@pytest.mark.parametrize("row", S.cases("fusion_ao") + S.cases("fusion_n_ao"), ids=lambda r: f"{r['op']}-{r['id']}")
def test_fusion_audio_only(row, dev):
    """The audio-only branch through the fusion module's run_forward / run_backward (avsep_fusion_ao_*, avsep_fusion_n_ao_*)."""
    P = _pkg()
    inp = S.inputs(row)
    x, draws, dfeat, prefill = _dev(dev, *inp)
    B, D, FT = x.shape
    net = P.models.fusion_net.CoLoc(att_type="cos")
    x4, dx = x.view(B, D, 1, FT), prefill.clone().view(B, D, 1, FT)
    if row["op"] == "fusion_ao":
        fus = net.run_forward(x4, [], inp[1])
        net.run_backward(x4, [], fus, dfeat, dx, None, None)
    else:                    # run_forward sends two sources to fusion.hip: the C = 2 row of fusion_n.hip needs the inner entry
        net.num_src = row["C"]
        fus = net._run_forward_n(x4, [], draws)
        net._run_backward_n(x4, [], fus, dfeat, dx, None)
    exp = S.expected(row, inp, dev)
    dx = dx.view(B, D, FT)
    untouched = torch.ones_like(dx, dtype=torch.bool).scatter_(2, exp["=pool_idx"][..., None], False)
    assert torch.equal(dx[untouched], prefill[untouched])
    _check(row, row["op"], "all draws zero" if row["op"] == "fusion_ao" and max(row["draws"]) == 0 else "draws",
           {"feat": fus["feat"], "=pool_idx": fus["pool_idx"], "dx": E.take(dx, exp["=pool_idx"])}, exp)


@pytest.mark.parametrize("row", S.cases("fusion_n_av"), ids=_id)
def test_fusion_n_av(row, dev):
    """avsep_fusion_n_av_fwd and _bwd through the fusion module's run_forward / run_backward (C sources); with C = 2 every output
    must also equal fusion.hip's kind 0 bit for bit."""
    P = _pkg()
    inp = S.inputs(row)
    x, vs, dfeat, dmatch, prefill = _dev(dev, *inp)
    B, C, D, HW, FT, att = row["B"], row["C"], row["D"], row["HW"], row["FT"], row["att"]
    Dc = D // C
    net = P.models.fusion_net.CoLoc(att_type=S._AN[att])
    x4, vs4 = x.view(B, D, 1, FT), [v.view(B, Dc, 1, HW) for v in vs]
    fus = net._run_forward_n(x4, vs4, None)
    dx = prefill.clone().view(B, D, 1, FT)
    if dmatch is not None:
        dvs = net._run_backward_n(x4, vs4, fus, dfeat, dx, dmatch)
    else:            # the wrapper sends scale 0 without a cotangent of the match term: the kernel's `1.f * scale` form by lib.call
        dvs = [torch.empty_like(v) for v in vs4]
        P.lib.call("avsep_fusion_n_av_bwd", _ptr(x4), net._ptr_array(vs4), B, C, D, FT, HW, att, _ptr(fus["a_pool"]), _ptr(fus["pool_idx"]),
                   _ptr(fus["sel_idx"]), _ptr(fus["best"]), _ptr(dfeat), None, 1.0 / B, _ptr(dx), net._ptr_array(dvs))
    exp = S.expected(row, inp, dev)
    dx = dx.view(B, D, FT)
    untouched = torch.ones_like(dx, dtype=torch.bool).scatter_(2, exp["=pool_idx"][..., None], False)
    assert torch.equal(dx[untouched], prefill[untouched])
    lds = ", LDS > 64 KB" if 4 * (D + (2 * C * C + C) * HW + 61) > 65536 else ""
    _check(row, "fusion_n_av_fwd", f"C = {C}, {S._AN[att]}{lds}",
           {"a_pool": fus["a_pool"], "=pool_idx": fus["pool_idx"], "=sel_idx": fus["sel_idx"], "=best": fus["best"],
            "att_maps": fus["att_maps"].view(B, C, HW), "match_part": fus["match_part"], "feat": fus["feat"]}, exp)
    _check(row, "fusion_n_av_bwd", f"C = {C}, {S._AN[att]}{lds}",
           {"dx": E.take(dx, exp["=pool_idx"]), "dv": torch.stack([t.view(B, Dc, HW) for t in dvs], 1)}, exp)
    if C == 2 and D == 2 * Dc:
        two = net.run_forward(x4, vs4, None)
        for n in ("a_pool", "pool_idx", "feat", "sel_idx", "att_maps", "match_part", "best"):
            assert torch.equal(two[n], fus[n]), n


# ---- attention -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.cases("attention"), ids=_id)
def test_attention(row, dev):
    """avsep_attmodel_infer_fwd and _bwd through attention_net._AttInferFn; maps_raw (which the node keeps to itself) is read
    from a direct call of the forward."""
    P = _pkg()
    from avsep_amd.models.attention_net import _AttInferFn
    inp = S.inputs(row)
    a, mix, dctx, dmaps, dmatch = _dev(dev, *inp)
    B, Sn, Kc, HW, att = row["B"], row["S"], row["K"], row["HW"], row["att"]
    with torch.no_grad():
        ctx, maps, match = _AttInferFn.apply(a, mix.view(B, Kc, 1, HW), att)
    raw, ctx2, match2 = torch.empty((B, Sn, HW), device=dev), torch.empty((B, Sn, Kc), device=dev), torch.empty((B,), device=dev)
    P.lib.call("avsep_attmodel_infer_fwd", _ptr(a), _ptr(mix), B, Sn, Kc, HW, att, _ptr(raw), _ptr(ctx2), _ptr(match2))
    assert torch.equal(ctx2, ctx) and torch.equal(match2, match) and torch.equal(raw.clamp(0, 1), maps.view(B, Sn, HW))
    da, dmix = torch.full_like(a, float("nan")), torch.full_like(mix, float("nan"))     # autograd always materialises dmaps and dmatch
    P.lib.call("avsep_attmodel_infer_bwd", _ptr(a), _ptr(mix), _ptr(raw), _ptr(dctx), _ptr(dmaps), _ptr(dmatch), B, Sn, Kc, HW, att,
               _ptr(da), _ptr(dmix))
    if dmaps is not None and dmatch is not None:                                         # the same call as the autograd node makes it
        ad, md = a.clone().requires_grad_(True), mix.view(B, Kc, 1, HW).clone().requires_grad_(True)
        c, m, t = _AttInferFn.apply(ad, md, att)
        ((c * dctx).sum() + (m * dmaps.view(m.shape)).sum() + (t * dmatch).sum()).backward()
        assert torch.equal(ad.grad, da) and torch.equal(md.grad.view(B, Kc, HW), dmix)
    outs = {"maps_raw": raw, "maps": maps.view(B, Sn, HW), "match": match, "ctx": ctx, "da": da, "dmix": dmix}
    lds = ", LDS > 64 KB" if 4 * (Sn * Kc + Sn * HW + 8) > 65536 else ""
    form = S._AN[att] + lds + ("" if row["dmaps"] else ", dmaps null") + ("" if row["dmatch"] else ", dmatch null")
    _check(row, "attmodel_infer", form, outs, S.expected(row, inp, dev))
