"""-m gpu: every glue kernel between the convolutions (csrc/ops.hip, csrc/b16.hip) alone, at the shapes of tests/glue_cases.py
— every launch form, every capped loop at least twice with a ragged last pass, the edges — against the float64 references of
tests/glueref.py, element by element: |out - ref| <= tau * absref (+ half a bf16 ulp for a B16 output), an element whose
absref is 0 must equal ref exactly (convref.check); sums: tau * sum absref (convref.check_stats).

tau = k * 2^-24 is derived, not measured: k = the number of fp32 roundings on the longest path of the kernel's formula, counted
at the source lines named in K below.  A sum's k is the per-thread term count of its fp32 partial sum (from the plan's grid)
plus its fp32 shuffle levels plus the roundings of one term.  The worst measured ratio |err| / bound of every kernel and form
is printed (pytest -s) and copied into the comments of K; above 1 the test fails.

Nothing is excluded: elements whose activation mask the kernel's own roundings could decide either way are moved away on the
CPU before the run (glueref.make_decidable), pool winners must equal the reference's first maximum (glueref.maxpool) but for
windows whose two candidates agree within 2^-23 relative in float64, at most 1e-6 of all windows.

Negative controls, on the smallest shape of every kernel: the gate rejects the last element set to 0, one element moved by
8x its bound, the fp32 result truncated to bf16 instead of rounded (B16 outputs) and a winner moved to the neighbouring tap."""
import pytest
import torch

import convref as R
import glue_cases as S
import glue_inputs as I
import glueref as G
from recipes import pkg as _pkg

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -24

# k per output: the fp32 roundings on the longest path, with the source line they were counted from, and the worst ratio
# |err| / (k * 2^-24 * absref [+ half a bf16 ulp]) measured on an MI355X per form (pytest -s prints them).
K = {
    # ops.hip channel_stats_kernel `s += v; q += v * v; if (++cnt == 64)`: at most 64 terms per fp32 partial (63 additions and
    # the product's rounding), fp64 from there on; +1 covers the second-order terms of 64 compounded roundings
    "channel_stats": lambda terms: min(terms, 64) + 1,    # measured: chunks 0.135 (k = 2), 0.007 at k = 65
    # ops.hip bn_bwd_apply_kernel `fmaf(p, a.x, fmaf(q, b.x, r))`: two fmaf
    "bn_bwd_apply": 2,    # measured: vec4 0.868, scalar 0.694
    # b16.hip f32_bn_bwd_apply_to_b16_kernel: the same two fmaf, then v_cvt_pk_bf16_f32 (the gate's half ulp)
    "bn_bwd_apply_to_b16": 2,    # measured: position 1.000 (exact bf16 ties)
    # ops.hip affine_act_kernel `fmaf(a.x, sc, sh)`, `v.x += fmaf(r.x, rs, rh)` (fmaf + addition), act_by_slope `v * slope`
    "affine_act": 4,    # measured: vec4 0.450, scalar 0.468
    # ops.hip affine_act_bwd_kernel `act_grad(pre, act) * (dz2 ? dv[k] + d2[k] : dv[k])`, `gk += av[k]`: sum, product, sum
    "affine_act_bwd": 3,    # measured: v4 0.610, v1 0.580
    # ... `s1 += gk; s2 += gk * (yk - mu) * is`: terms additions of fp32 partials (fp64 from wave_sum_d on), the 3 roundings
    # of gk and (yk - mu), * gk, * is
    "affine_act_bwd.bstats": lambda terms: terms + 6,    # measured: v4 0.063, v1 0.122
    # ops.hip maxpool_fwd*_kernel `act_apply(fmaf(p[h * W + w], sc, sh), act)`: fmaf and the 0.2f product; the winner itself
    # is copied
    "maxpool": 2,    # measured: fwd4 0.000, generic 0.000 (every winner bit for bit), no window differs
    # ops.hip maxpool_bwd_kernel `if (idx[o] == self) s += dy[o]` over <= 4 windows: 3 additions
    "maxpool_bwd": 3,    # measured: gather 0.648
    # ops.hip maxpool_bn_relu_bwd_stats_kernel `s1 += gv; s2 = fmaf(gv, (yv - mu) * is, s2)`: one rounding per term,
    # (yv - mu) and * is
    "maxpool_bn_relu_bwd_stats": lambda terms: terms + 2,    # measured: plane 0.576
    # ops.hip maxpool_bn_relu_bwd_apply*_kernel: <= 4 gradients summed (3 additions), `fmaf(cp, sk, fmaf(cq, yv[k], cr))`
    "maxpool_bn_relu_bwd_apply": 5,    # measured: apply4 0.326, pair 0.253, apply1 0.383
    # ops.hip temporal_mean_fwd_kernel `s += x[..]` T - 1 additions, `s / (float)T`
    "temporal_mean": lambda T: T,    # measured: flat 0.592
    # ops.hip temporal_mean_bwd_kernel `inv = 1.f / (float)T`, `dy[..] * inv`
    "temporal_mean_bwd": 2,    # measured: flat 0.666
    # ops.hip sgd_kernel `d = fmaf(wd, pv, g[i] * gs)` 2, `b = fmaf(mom, buf[i], d)` 1; `p[i] = pv - lr * b` 2 more
    "sgd.buf": 3, "sgd.p": 5,    # measured: flat buf 0.625, p 0.338
    # copies: exact (the B16 outputs: half a bf16 ulp)
    # measured: space_to_depth2 planes 0.000, to_f32 position 0.000, to_b16 position 1.000, b16_space_to_depth2 flat 1.000 (ties)
    "space_to_depth2": 0, "to_b16": 0, "to_f32": 0, "b16_space_to_depth2": 0,
    # b16.hip b16_affine_act_kernel: as affine_act
    "b16_affine_act": 4,    # measured: slot 1.000, slot,images 1.000 (exact bf16 ties: the inputs are bf16 values)
    # b16.hip b16_affine_act_bwd_kernel `g += d2[j]`, `g *= pre > 0.f ? 1.f : neg`, `g += ad[j]`
    "b16_affine_act_bwd": 3,    # measured: slot 1.000, slot,images 1.000 (ties)
    # ... `s1[j] += g; s2[j] = fmaf(g, (v[j] - mu[j]) * is[j], s2[j])` over the thread's whole iteration count, b16_block_stats'
    # five fp32 xor-shuffle levels (fp64 across the waves), the 3 roundings of g, (v - mu) and * is
    "b16_affine_act_bwd.bstats": lambda terms: terms + 10,    # measured: slot 0.086, slot,images 0.001
    # b16.hip b16_bn_bwd_apply_kernel `fmaf(cp[j], d[j], fmaf(cq[j], v[j], cr[j]))`
    "b16_bn_bwd_apply": 2,    # measured: slot 1.000, slot,images 1.000 (ties)
    # b16.hip b16_maxpool_fwd_kernel `act_by_slope(fmaf(v[j], sc[j], sh[j]), slope)`
    "b16_maxpool": 2,    # measured: slot 1.000, slot,images 1.000 (ties), no window differs
    # b16.hip b16_maxpool_bwd_stats_kernel `gg = gv[j] + g2v[j]`, `s1[j] += gg; s2[j] = fmaf(gg, (yv - mu[j]) * is[j], s2[j])`,
    # five shuffle levels
    "b16_maxpool_bwd_stats": lambda terms: terms + 8,    # measured: slot 0.136, slot,images 0.004
    # b16.hip b16_maxpool_bwd_apply_kernel `acc[j] += gv[j] + g2v[j]` over <= 4 windows (4 sums of two, 3 additions: the
    # longest path holds 1 + 3), `fmaf(cp[j], dz, fmaf(cq[j], yv[j], cr[j]))`
    "b16_maxpool_bwd_apply": 6,    # measured: slot 1.000, slot,images 1.000 (ties)
    # b16.hip b16_channel_sum_kernel `s1[j] += v[j]` over the thread's iterations, five shuffle levels, b16_sum_finish_kernel
    # `(float)acc[c]`
    "b16_channel_sum": lambda terms: terms + 6,    # measured: slot 0.033, slot,images 0.026
}


def _id(row):
    return f"{row[0]}-{S.case_id(row)}"


def _large(row):
    """Rows of more than 2^20 elements run two variants of their kernel instead of all (a test case takes seconds)."""
    return S.largest_tensor(row[1], row[2], row[3]) > 2 ** 20


def _smallest(kernel):
    return min(S.cases(kernel), key=lambda r: S.largest_tensor(r[1], r[2], r[3]))


def _plan(row):
    """Assert the row's form and grid, and that the loops it names are taken at least twice; returns the loops."""
    kernel, op, dims, aux, form, grid, twice, _ = row
    assert S.plan(_pkg().lib.load(), op, dims, aux) == (form, grid), row
    lp = S.loops(op, dims, aux, form, grid)
    for name in twice:
        assert lp[name] > 1, (row, lp)
    assert S.largest_tensor(op, dims, aux) < S.SIZE_LIMIT
    return lp


def _f64(out, ref):
    return (R.nchw(out) if out.dtype == torch.bfloat16 else out).to(F64).reshape(ref.shape).contiguous()


def _half_ulp_bf16(x):
    """convref.half_ulp_bf16 with the power of two built from its exponent bits: torch.ldexp on the device goes through pow and
    may miss 2^(e-9) by an ulp, which turns an exact round-to-nearest-even tie (error == half an ulp) into a violation."""
    _, e = torch.frexp(x.abs())
    return ((e.to(torch.int64) - 9 + 1023) << 52).view(torch.float64)


def _violations(o, ref, absref, tau, b16):
    """Elements with |o - ref| > tau * absref (+ half a bf16 ulp), or NaN: convref.check's bound, compared as the inequality."""
    bound = tau * absref
    if b16:
        bound = bound + _half_ulp_bf16(torch.maximum(ref.abs(), o.abs()))
    return int((((o - ref).abs() > bound) | torch.isnan(o)).sum())


def _gate(row, name, out, ref, absref, k, b16=False, stats=False, controls=None, variant=""):
    """The per-element gate, its printed worst ratio, and (on the kernel's smallest shape) the negative controls."""
    tau = k * U
    r = R.check_stats(out, ref, absref, tau) if stats else R.check(out, ref, absref, tau, b16=b16)
    print(f"glue | {row[0]} | {row[4]} | {S.case_id(row)} | {variant} | {name} | k={k} | worst ratio {r[0]:.3f} "
          f"(at {r[1]}: out {r[5]:.9g} ref {r[2]:.9g} absref {r[3]:.3g})")
    # the inequality itself decides, with an exact half ulp: an exact bf16 tie sits ON the bound (ratio 1.0)
    assert _violations(_f64(out, ref), ref, absref, tau, b16) == 0, (row, variant, name, r)
    if controls is None:
        controls = row is _smallest(row[0])
    if not controls:
        return
    o, ref, absref = _f64(out, ref), ref.contiguous(), absref.contiguous()
    bound = tau * absref + (_half_ulp_bf16(torch.maximum(ref.abs(), o.abs())) if b16 else 0.0)
    chk = lambda t: 2.0 if _violations(t, ref, absref, tau, b16) else 0.0
    live = (ref.abs() > 2 * bound).reshape(-1).nonzero()
    assert live.numel() > 0, (row, name)
    if not stats:                                    # the last element (of the last image) that is not a legitimate zero -> 0
        t = o.clone()
        t.view(-1)[int(live[-1])] = 0.0
        assert chk(t) > 1.0, ("zeroed last element passed", row, variant, name, int(live[-1]), o.numel())
    t = o.clone()                                    # one element moved by 8x its bound (an exact output: by one fp32 ulp)
    i = int(live[0])
    step = 8.0 * float(bound.reshape(-1)[i])
    if step == 0.0:
        step = float(torch.nextafter(ref.reshape(-1)[i].float().abs(), torch.tensor(float("inf"), device=ref.device)).to(F64)
                     - ref.reshape(-1)[i].abs())
    t.view(-1)[i] += step
    assert chk(t) > 1.0, ("moved element passed", row, variant, name)
    if b16:                                          # the same fp32 result truncated to bf16 instead of rounded
        assert chk(G.truncate_bf16(ref)) > 1.0, ("truncation passed", row, variant, name)


def _idx_gate(row, idx, want, x, scale, shift, act, H, W, controls, variant=""):
    """Pool winners (flat positions) against the reference's first maximum; a mismatch is tolerated only between candidates
    whose float64 values agree within 2^-23 relative, in at most 1e-6 of the windows."""
    N, Cc = want.shape[:2]
    v = G.pool_values(x, scale, shift, act, exact=False).reshape(N, Cc, -1)

    def bad_windows(got):
        got = got.long().reshape(N, Cc, -1)
        ref = want.reshape(N, Cc, -1)
        if bool(((got < 0) | (got >= H * W)).any()):
            return float("inf"), 0
        mis = got != ref
        a, b = v.gather(2, got), v.gather(2, ref)
        close = (a - b).abs() <= 2.0 ** -23 * torch.maximum(a.abs(), b.abs())
        return int((mis & ~close).sum()), int(mis.sum())
    hard, soft = bad_windows(idx)
    print(f"glue | {row[0]} | {row[4]} | {S.case_id(row)} | {variant} | idx | {soft} of {want.numel()} windows differ, "
          f"{hard} beyond 2^-23")
    assert hard == 0 and soft <= 1e-6 * want.numel(), (row, variant, hard, soft)
    if controls:                                     # one winner moved to the neighbouring tap
        t = idx.long().clone().reshape(-1)
        t[-1] = t[-1] - 1 if int(t[-1]) % W > 0 else t[-1] + 1
        if 0 <= int(t[-1]) < H * W:
            hard, soft = bad_windows(t.reshape(idx.shape))
            assert hard > 0 or soft > 1e-6 * want.numel(), ("moved winner passed", row)


def _dev(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _img(t):
    return None if t is None else G.b16_image(t)


# ---- fp32 kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.cases("channel_stats"), ids=_id)
def test_channel_stats(row, dev):
    lp, Kn = _plan(row), _pkg().kernels
    (x,) = _dev(dev, I.randn(I.gen(row), *row[2]) + 0.5)
    stats = torch.zeros(2 * row[2][1], dtype=F64, device=dev)
    Kn.channel_stats(x, stats)
    ref, bound = G.channel_stats(x)
    _gate(row, "stats", stats, ref, bound, K["channel_stats"](lp["terms"]), stats=True)


@pytest.mark.parametrize("row", S.cases("bn_bwd_apply") + S.cases("bn_bwd_apply_to_b16") + S.cases("b16_bn_bwd_apply"), ids=_id)
def test_bn_bwd_apply(row, dev):
    _plan(row)
    Kn, g, Cc = _pkg().kernels, I.gen(row), row[2][1]
    dz, y, pqr = _dev(dev, I.act_input(g, row), I.act_input(g, row), torch.stack([I.chan(g, Cc), I.chan(g, Cc), I.randn(g, Cc)]))
    if row[0] == "b16_bn_bwd_apply":
        out = Kn.bn_bwd_apply_(_img(dz), _img(y), pqr, fresh=True)
    else:
        out = Kn.bn_bwd_apply_(dz.clone(), y, pqr, fresh=True, to_b16_out=row[0].endswith("to_b16"))
    b16 = row[0] != "bn_bwd_apply"
    assert (out.dtype == torch.bfloat16) == b16
    ref, a = G.bn_bwd_apply(dz, y, pqr)
    _gate(row, "dy", out, ref, a, K[row[0]], b16=b16)


_RES = ("none", "plain", "affine")


def _act_operands(row, g, res, act):
    Cc = row[2][1]
    y, r = I.act_input(g, row), (I.act_input(g, row) if res != "none" else None)
    sc, sh = I.chan(g, Cc), 0.3 * I.randn(g, Cc)
    rs, rh = (I.chan(g, Cc), 0.3 * I.randn(g, Cc)) if res == "affine" else (None, None)
    if act != 0:
        y = I.decidable(y, row, sc, sh, r, rs, rh)
    return y, r, sc, sh, rs, rh


@pytest.mark.parametrize("row", S.cases("affine_act") + S.cases("b16_affine_act"), ids=_id)
def test_affine_act(row, dev):
    _plan(row)
    Kn, b16 = _pkg().kernels, I.is_b16(row)
    first = True
    for act in (0, 1, 2):
        for res in _RES:
            if _large(row) and (act, res) not in ((1, "affine"), (2, "plain")):
                continue
            y, r, sc, sh, rs, rh = _dev(dev, *_act_operands(row, I.gen(row, f"{act}{res}"), res, act))
            out = Kn.affine_act(_img(y) if b16 else y, sc, sh, _img(r) if b16 else r, act, rs, rh)
            ref, a = G.affine_act(y, sc, sh, r, rs, rh, act)
            _gate(row, "z", out, ref, a, K[row[0]], b16=b16, controls=first and row is _smallest(row[0]), variant=f"act{act},res={res}")
            first = False


# (act, dz2, add, residual, stats_only)
_BWD_VARIANTS = [(1, False, False, "none", False), (1, True, True, "affine", False), (2, False, True, "plain", False),
                 (0, True, False, "none", False), (2, True, True, "affine", False), (1, False, False, "plain", True),
                 (0, False, False, "none", True)]


@pytest.mark.parametrize("row", S.cases("affine_act_bwd") + S.cases("b16_affine_act_bwd"), ids=_id)
def test_affine_act_bwd(row, dev):
    lp = _plan(row)
    Kn, b16, Cc = _pkg().kernels, I.is_b16(row), row[2][1]
    terms = lp["terms"] * (4 if row[4] == "v4" else 1)
    im = _img if b16 else (lambda t: t)
    for n, (act, has2, has_add, res, stats_only) in enumerate(_BWD_VARIANTS):
        if _large(row) and n not in (1, 5):
            continue
        g = I.gen(row, str(n))
        y, r, sc, sh, rs, rh = _act_operands(row, g, res, act)
        dz, dz2, add = I.act_input(g, row), (I.act_input(g, row) if has2 else None), (I.act_input(g, row) if has_add else None)
        mean, invstd = 0.2 * I.randn(g, Cc), I.chan(g, Cc, signed=False)
        y, r, sc, sh, rs, rh, dz, dz2, add, mean, invstd = _dev(dev, y, r, sc, sh, rs, rh, dz, dz2, add, mean, invstd)
        bstats = torch.zeros(2 * Cc, dtype=F64, device=dev)
        out = Kn.affine_act_bwd_(im(dz.clone()), im(y), sc, sh, im(r), im(add), mean, invstd, act, bstats, rs, rh, dz2=im(dz2),
                                 stats_only=stats_only)
        ref = G.affine_act_bwd(dz, dz2, y, sc, sh, r, rs, rh, add, mean, invstd, act)
        assert int(ref["undecidable"].sum()) == 0
        var = f"act{act},dz2={int(has2)},add={int(has_add)},res={res}" + (",stats_only" if stats_only else "")
        ctl = n == 1 and row is _smallest(row[0])
        if not (stats_only and b16):                  # the B16 kernel's statistics-only pass writes nothing
            _gate(row, "g", out, *ref["g"], K[row[0]], b16=b16, controls=ctl, variant=var)
        else:
            assert torch.equal(R.nchw(out), dz)
        _gate(row, "bstats", bstats, *ref["bstats"], K[row[0] + ".bstats"](terms), stats=True, controls=ctl, variant=var)


@pytest.mark.parametrize("row", S.cases("maxpool_fwd") + S.cases("b16_maxpool"), ids=_id)
def test_maxpool(row, dev):
    _plan(row)
    Kn, b16 = _pkg().kernels, I.is_b16(row)
    N, Cc, H, W = row[2]
    big = N * Cc > 65536
    for act, affine in ((1, True),) if big else ((0, True), (1, True), (2, True), (1, False)):
        x, sc, sh = _dev(dev, *I.pool_operands(row, act))
        if not affine:
            sc = sh = None
        want = G.maxpool(x, sc, sh, act)
        assert torch.equal(want["tap"], G.maxpool(x, sc, sh, act, exact=False)["tap"]), "seed: the reference itself is undecided"
        y, idx = Kn.maxpool3x3s2(_img(x) if b16 else x, sc, sh, act)
        ctl = act == 1 and affine and row is _smallest(row[0])
        var = f"act{act}" + ("" if affine else ",no affine")
        flat = G.taps_to_flat(G.blocked_to_nchw(idx), H, W) if b16 else idx
        _idx_gate(row, flat, want["idx"], x, sc, sh, act, H, W, ctl, var)
        _gate(row, "y", y, *want["y"], K["b16_maxpool" if b16 else "maxpool"], b16=b16, controls=ctl, variant=var)


@pytest.mark.parametrize("row", S.cases("maxpool_bwd"), ids=_id)
def test_maxpool_bwd(row, dev):
    _plan(row)
    N, Cc, H, W = row[2]
    x, sc, sh = _dev(dev, *I.pool_operands(row, 1))
    idx = G.maxpool(x, sc, sh, 1)["idx"]
    (dy,) = _dev(dev, I.randn(I.gen(row), *idx.shape))
    dx = _pkg().kernels.maxpool3x3s2_bwd(dy, idx.to(torch.int32).contiguous(), H, W)
    _gate(row, "dx", dx, *G.maxpool_bwd(dy, idx, H, W), K["maxpool_bwd"])


def _stem_operands(row, dev, with_g2):
    g = I.gen(row)
    N, Cc, H, W = row[2]
    y, sc, sh = I.pool_operands(row, 1)
    y = I.decidable(y, row, sc, sh)
    Ho, Wo = S.out_hw(H), S.out_hw(W)
    gr = I.randn(g, N, Cc, Ho, Wo)
    g2 = I.randn(g, N, Cc, Ho, Wo) if with_g2 else None
    if I.is_b16(row):
        gr, g2 = R.bf16(gr), (R.bf16(g2) if with_g2 else None)
    mean, invstd = 0.2 * I.randn(g, Cc), I.chan(g, Cc, signed=False)
    pqr = torch.stack([I.chan(g, Cc), I.chan(g, Cc), I.randn(g, Cc)])
    y, sc, sh, gr, g2, mean, invstd, pqr = _dev(dev, y, sc, sh, gr, g2, mean, invstd, pqr)
    m = G.maxpool(y, sc, sh, 1)
    return y, sc, sh, gr, g2, mean, invstd, pqr, m


@pytest.mark.parametrize("row", S.cases("maxpool_bn_relu_bwd_stats") + S.cases("b16_maxpool_bwd_stats"), ids=_id)
def test_maxpool_bn_relu_bwd_stats(row, dev):
    lp = _plan(row)
    Kn, b16, Cc = _pkg().kernels, I.is_b16(row), row[2][1]
    for with_g2 in ((False, True) if b16 else (False,)):
        y, sc, sh, gr, g2, mean, invstd, pqr, m = _stem_operands(row, dev, with_g2)
        bnrow = torch.stack([sc, sh, mean, invstd])
        bstats = torch.zeros(2 * Cc, dtype=F64, device=dev)
        if b16:
            Kn.maxpool_bn_relu_bwd_stats(_img(gr), G.nchw_to_blocked(m["tap"].to(torch.uint8)), _img(y), bnrow, bstats, g2=_img(g2))
        else:
            Kn.maxpool_bn_relu_bwd_stats(gr, m["idx"].to(torch.int32).contiguous(), y, bnrow, bstats)
        ref = G.stem_tail_bwd(gr, g2, m["idx"], y, sc, sh, mean, invstd, None)
        assert int(ref["undecidable"].sum()) == 0
        _gate(row, "bstats", bstats, *ref["bstats"], K[row[0]](lp["terms"]), stats=True, variant=f"g2={int(with_g2)}",
              controls=not with_g2 and row is _smallest(row[0]))


@pytest.mark.parametrize("row", S.cases("maxpool_bn_relu_bwd_apply") + S.cases("b16_maxpool_bwd_apply"), ids=_id)
def test_maxpool_bn_relu_bwd_apply(row, dev):
    _plan(row)
    Kn, b16 = _pkg().kernels, I.is_b16(row)
    for with_g2, out_f32 in (((False, False), (True, False), (True, True)) if b16 else ((False, False),)):
        y, sc, sh, gr, g2, mean, invstd, pqr, m = _stem_operands(row, dev, with_g2)
        bnrow = torch.stack([sc, sh, mean, invstd])
        if b16:
            dy = Kn.maxpool_bn_relu_bwd_apply(_img(gr), G.nchw_to_blocked(m["tap"].to(torch.uint8)), _img(y), bnrow, pqr, g2=_img(g2),
                                              out_f32=out_f32)
        else:
            dy = Kn.maxpool_bn_relu_bwd_apply(gr, m["idx"].to(torch.int32).contiguous(), y, bnrow, pqr)
        assert (dy.dtype == torch.bfloat16) == (b16 and not out_f32)
        ref = G.stem_tail_bwd(gr, g2, m["idx"], y, sc, sh, None, None, pqr)
        _gate(row, "dy", dy, *ref["dy"], K[row[0]], b16=b16 and not out_f32, variant=f"g2={int(with_g2)},out_f32={int(out_f32)}",
              controls=not with_g2 and row is _smallest(row[0]))


@pytest.mark.parametrize("row", S.cases("temporal_mean") + S.cases("temporal_mean_bwd"), ids=_id)
def test_temporal_mean(row, dev):
    _plan(row)
    Kn, (B, Cc, H, W), T = _pkg().kernels, row[2], row[3]
    if row[1] == "temporal_mean_fwd":
        (x,) = _dev(dev, I.randn(I.gen(row), B * T, Cc, H, W))
        out = Kn.temporal_mean(x, B, T)
        assert out.shape == (B, Cc, H, W)
        _gate(row, "y", out, *G.temporal_mean(x, B, T), K["temporal_mean"](T))
    else:
        (dy,) = _dev(dev, I.randn(I.gen(row), B, Cc, H, W))
        out = Kn.temporal_mean_bwd(dy, B, T)
        assert out.shape == (B * T, Cc, H, W)
        _gate(row, "dx", out, *G.temporal_mean_bwd(dy, B, T), K["temporal_mean_bwd"])


@pytest.mark.parametrize("row", S.cases("sgd_momentum_"), ids=_id)
def test_sgd_momentum(row, dev):
    _plan(row)
    n = row[2][3]
    for first in (True, False):
        g = I.gen(row, str(first))
        p, gr, buf = _dev(dev, I.randn(g, n), I.randn(g, n), I.randn(g, n))
        p2, buf2 = p.clone(), buf.clone()
        _pkg().kernels.sgd_momentum_(p2, gr, buf2, 1e-2, 0.9, 1e-4, 0.5, first)
        ref = G.sgd(p, gr, buf, 1e-2, 0.9, 1e-4, 0.5, first)
        ctl = first and row is _smallest(row[0])
        _gate(row, "buf", buf2, *ref["buf"], K["sgd.buf"], controls=ctl, variant=f"first={int(first)}")
        _gate(row, "p", p2, *ref["p"], K["sgd.p"], controls=ctl, variant=f"first={int(first)}")


@pytest.mark.parametrize("row", S.cases("space_to_depth2") + S.cases("b16_space_to_depth2"), ids=_id)
def test_space_to_depth2(row, dev):
    _plan(row)
    b16 = I.is_b16(row)
    (x,) = _dev(dev, I.randn(I.gen(row), *row[2]))
    out = _pkg().kernels.space_to_depth2(x, 16 if b16 else row[3], b16=b16)
    assert (out.dtype == torch.bfloat16) == b16
    _gate(row, "xs", out, *G.space_to_depth2(x, 16 if b16 else row[3]), K[row[0]], b16=b16)


@pytest.mark.parametrize("row", S.cases("to_b16") + S.cases("to_f32"), ids=_id)
def test_conversions(row, dev):
    _plan(row)
    Kn = _pkg().kernels
    (x,) = _dev(dev, I.randn(I.gen(row), *row[2]))
    if row[0] == "to_b16":
        out = Kn.to_b16(x)
        assert out.dtype == torch.bfloat16 and out.shape == (row[2][0], row[2][1] // 16, row[2][2], row[2][3], 16)
        _gate(row, "img", out, *G.identity(x), K["to_b16"], b16=True)
    else:
        img = G.b16_image(x)
        out = Kn.to_f32(img)
        assert out.dtype == torch.float32 and out.shape == tuple(row[2])
        _gate(row, "x", out, *G.identity(img), K["to_f32"])


@pytest.mark.parametrize("row", S.cases("b16_channel_sum"), ids=_id)
def test_b16_channel_sum_through_the_weight_gradient(row, dev):
    """b16_channel_sum has no entry point of its own: it is the bias gradient of avsep_conv2d_wgrad on the B16 kernel."""
    lp = _plan(row)
    Kn, g, (N, Co, H, W) = _pkg().kernels, I.gen(row), row[2]
    x, dy = _dev(dev, R.bf16(I.randn(g, N, 16, H, W)), R.bf16(I.randn(g, N, Co, H, W) + 0.25))
    cv = Kn.Conv(_img(x), Co, 3, 1, 1, prec="bf16")
    assert cv.kernel_name("wgrad") == "wgradb_kernel" and cv._grid_geometry() is None
    dw, db = cv.wgrad(_img(dy), want_bias=True)
    _gate(row, "dbias", db, *G.channel_sum(dy), K["b16_channel_sum"](lp["terms"]), stats=True)
