"""gpu: every launch variant the stored conv dispatch table names, run once and checked per element against float64.

test_gpu_benched_conv_calls.py gates what the benched step launches: batch 64 (or the config-5 batch), plan_n = 0, no
AVSEP_ALGO_NO_* bit.  The table (tests/golden/conv_dispatch.json) names many more (mode, variant, precision) routes: those
of N = 1, 2 and 8 (inference, long recordings, localisation, a last short batch), of a planned batch (plan_n, what the parity
tests run) and of a forbidden family.  tests/conv_variant_cases.py picks the cheapest sweep descriptor of every such triple;
here each is built as a kernels.Conv, the variant of the descriptor that is really launched is asserted BEFORE anything
runs (a case that runs another variant than it names fails), the case's mode is launched, and every output is gated with
convref: |out - ref| <= tau * absref per element, tau / tile_absref / the bf16 operand model by the rules of the benched-calls
test, tolerances convref.TAU unchanged (two variants whose short sums round worse relative to absref than the benched ones
have their own entry and the reason in convref.VARIANT_TAU).  A variant planned for batch 64 and launched at N = 1 runs on a
tiny grid: partial last workgroups, split-K slabs with nothing in them, tiles that cross the only image.

  fwd    with bias and statistics, and without statistics (the smallco_fwd / head_fwd_kernel route); B16 output where allowed
  dgrad  plain; where the table says dgrad_act is fused also dgrad_act (ReLU, bstats, residual behind its affine, dz2, add: no
         element excluded, see conv_variant_cases.act_operands); B16 output where allowed.  The head descriptor's data
         gradient is the entry point its variant names, dgrad_up2x: with bstats1, and once more accumulating into g0
  wgrad  with the bias gradient

Negative controls on the main output of every call (no relaunch): one border row of the last image zeroed (dw: a kernel row
of the last output channel), and one element moved by 8 times its bound; the gate must reject both.

One line per call is printed (pytest -s): variant, mode, geometry, worst |out - ref| / absref, tau; profiles/
conv_variant_ratios.txt is that table as measured on an MI355X.  Measured there: the 178 cases (241 gated calls, the float64
self-check of the module included) take 3 s, 3.9 s with collection; no case takes more than half a second.
"""
import time

import pytest
import torch

import conv_variant_cases as V
import convref as R
from convref import WINOGRAD, tau_of_variant
from test_gpu_benched_conv_calls import MUST_BF16, _fp64_path_is_exact, _variant

pytestmark = pytest.mark.gpu

CASES = V.cases()
MAIN = ("y", "dx", "g0", "dw")
STATS = ("stats", "bstats", "bstats1")


@pytest.fixture(scope="module")
def fp64_exact(dev):
    t0 = time.time()
    _fp64_path_is_exact(dev)
    yield
    print(f"\ntests/test_gpu_conv_variants.py: {len(CASES)} cases, {time.time() - t0:.0f} s in all")


def _controls(out, r, ra, tau, excl):
    """The two corruptions of test_gpu_benched_conv_calls._Shadow._controls that need no relaunch: {name: ratio}."""
    rejected = {}
    o = R.nchw(out).to(torch.float64).reshape(r.shape).clone()
    row = max((-1, 0), key=lambda i: float(r[-1, :, i, :].abs().sum()))
    o[-1, :, row, :] = 0
    rejected["b"] = R.check(o, r, ra, tau, excluded=excl)[0]
    o = R.nchw(out).to(torch.float64).reshape(r.shape).clone()
    i = int(ra.reshape(-1).argmax())
    o.view(-1)[i] += 8 * tau * float(ra.reshape(-1)[i])
    rejected["c"] = R.check(o, r, ra, tau, excluded=excl)[0]
    return rejected


class _Gate:
    """Collects, for one case, the worst ratio of every call and everything that failed."""

    def __init__(self, case, cv):
        self.case, self.cv, self.lines, self.failures = case, cv, [], []

    def call(self, name, variant, outs, op):
        """outs: {output name: tensor}; op: the call's operands for convref.reference."""
        family = variant.split(":")[0]
        tau = tau_of_variant(variant, self.case.prec)
        ref = R.reference(self.cv, name, op)
        excl = ref.get("excluded")
        worst = (0.0, None)
        for k, o in outs.items():
            assert o is not None and k in ref, (name, k)
            r, ra = ref[k]
            if family in WINOGRAD and k in ("y", "dx", "dw"):
                ra = R.tile_absref(ra)
            if k in STATS:
                res = R.check_stats(o, r, ra, tau)
            else:
                assert o.dtype == torch.float32
                res = R.check(o, r, ra, tau, excluded=excl if k == "dx" else None)
            if k == "dx" and name == "dgrad_act":
                if excl is None or res[4] != 0:
                    self.failures.append((name, "dgrad_act elements excluded", res[4]))
                if not bool((ra > 0).all()):
                    self.failures.append((name, "dgrad_act absref not strictly positive"))
            if res[0] >= worst[0]:
                worst = (res[0], (k,) + res[1:4] + res[5:])
            if not res[0] <= 1.0:
                self.failures.append((name, k, "over tau", res[0] * tau, tau, res[1:4] + res[5:]))
            if k in MAIN:
                rej = _controls(o, r, ra, tau, excl if k == "dx" else None)
                if not all(v > 1.0 for v in rej.values()):
                    self.failures.append((name, k, "negative control not rejected", rej))
        label = name + ("+stats" if "stats" in outs else "")
        self.lines.append(f"{variant:44s} {label:12s} {self.case.prec:4s} {self.case.geometry():88s} worst {worst[0] * tau:9.3e} "
                          f"tau {tau:7.1e} at {worst[1][0] if worst[1] else '-'}")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_variant_vs_float64(dev, fp64_exact, case):
    import avsep_amd as P
    K = P.kernels
    saved = (K.plan_batch_scale, K.algo_mask)
    try:
        K.plan_batch_scale = case.plan_batch_scale
        K.set_algo_mask(*([case.algo] if case.algo else []))
        gate = _run(dev, K, case)
    finally:
        K.plan_batch_scale, K.algo_mask = saved
    torch.cuda.synchronize()
    print()
    for line in gate.lines:
        print("VARIANT", line)
    assert not gate.failures, gate.failures


def _run(dev, K, c):
    t = lambda z: None if z is None else z.to(dev)
    zeros = lambda ch: torch.zeros(2 * ch, dtype=torch.float64, device=dev)
    op = {k: t(v) for k, v in V.operands(c).items()}
    cv = K.Conv(op["x0"], c.Cout, c.k, c.stride, c.pad, c.dil, x1=op["x1"], sc0=op["sc0"], sh0=op["sh0"], act0=c.act0,
                sc1=op["sc1"], sh1=op["sh1"], act1=c.act1, up2x=c.up2x, prec=c.prec)
    assert cv.d.plan_n == c.plan_n and cv.d.algo == K.algo_mask, (cv.d.plan_n, cv.d.algo)

    def launched(mode, with_stats):
        g = cv._grid_geometry({"fwd": 0, "wgrad": 2}.get(mode, 1))
        return _variant(K, cv._grid_desc(g) if g is not None else cv.d, mode, with_stats)
    # ---- the variant that is really launched, before anything is ----
    routes = {"fwd": [("fwd_stats", True), ("fwd", False)], "dgrad": [("dgrad", False)], "wgrad": [("wgrad", False)]}[c.mode]
    got = {col: launched(c.mode, ws) for col, ws in routes}
    want = {col: c.expect[col] for col, _ in routes if c.expect[col] is not None}     # None: a supplement case's other route
    assert {col: got[col] for col in want} == want, (c, got)
    assert c.variant in got.values()
    assert bool(cv.head_applicable()) == bool(c.head)
    assert c.mode != "dgrad" or bool(cv.dgrad_act_fused()) == bool(c.dgrad_act_fused)
    gate = _Gate(c, cv)
    src = {k: op[k] for k in ("x0", "x1", "sc0", "sh0", "sc1", "sh1")}
    bf = lambda variant: variant.split(":")[0] in MUST_BF16
    if c.mode == "fwd":
        wp = cv.pack(op["w"], 0)
        for col, with_stats in routes:
            st = zeros(c.Cout) if with_stats else None
            y = cv.fwd(wp, op["bias"], st, out_b16=False)
            outs = {"y": y, "stats": st.clone()} if with_stats else {"y": y}
            gate.call("fwd", got[col], outs, dict(src, w=op["w"], bias=op["bias"], stats=with_stats, bf16=bf(got[col])))
            if with_stats and cv.io_formats(0)[1] and K.b16_ok(c.Cout):
                y16 = cv.fwd(wp, op["bias"], None, out_b16=True)
                assert K.is_b16(y16) and K.dims(y16) == tuple(y.shape)
                if not torch.equal(K.to_f32(y16), y.to(torch.bfloat16).float()):
                    gate.failures.append(("fwd", "B16 output != bf16(fp32 output)"))
                gate.lines[-1] += " +b16"
    elif c.mode == "wgrad":
        dw, db = cv.wgrad(op["dy"], want_bias=True)
        gate.call("wgrad", got["wgrad"], {"dw": dw, "dbias": db}, dict(src, dy=op["dy"], want_bias=True, bf16=bf(got["wgrad"])))
    elif c.head:
        h = {k: t(v) for k, v in V.head_operands(c).items()}
        base = dict(src, w=op["w"], dy=op["dy"], mean1=h["mean1"], invstd1=h["invstd1"], bstats1=True, bf16=False)
        for acc in (None, h["g0_acc"]):
            bst = zeros(c.C1)
            before = acc.clone() if acc is not None else None
            g0, g1 = cv.dgrad_up2x(op["w"], op["dy"], mean1=h["mean1"], invstd1=h["invstd1"], bstats1=bst, g0_acc=acc)
            gate.call("dgrad_up2x", got["dgrad"], {"g0": g0, "g1": g1, "bstats1": bst.clone()}, dict(base, g0_acc=before))
    else:
        wpd = cv.pack(op["w"], 1)
        b = bf(got["dgrad"])
        dx = cv.dgrad(wpd, op["dy"], out_b16=False)
        gate.call("dgrad", got["dgrad"], {"dx": dx}, dict(w=op["w"], dy=op["dy"], bf16=b))
        if cv.io_formats(1)[1] and K.b16_ok(c.Cin):
            dx16 = cv.dgrad(wpd, K.to_b16(op["dy"]), out_b16=True)
            assert K.is_b16(dx16)
            if not torch.equal(K.to_f32(dx16), dx.to(torch.bfloat16).float()):
                gate.failures.append(("dgrad", "B16 data gradient != bf16(fp32 data gradient)"))
            gate.lines[-1] += " +b16"
        del dx
        if c.dgrad_act_fused:
            a = {k: t(v) for k, v in V.act_operands(c).items()}
            bst = zeros(c.Cin)
            dx = cv.dgrad_act(wpd, op["dy"], a["y"], a["scale"], a["shift"], a["mean"], a["invstd"], R.ACT_RELU, bst,
                              residual=a["residual"], res_scale=a["res_scale"], res_shift=a["res_shift"], dz2=a["dz2"],
                              add=a["add"])
            gate.call("dgrad_act", got["dgrad"], {"dx": dx, "bstats": bst.clone()},
                      dict(a, w=op["w"], dy=op["dy"], act=R.ACT_RELU, bstats=True, bf16=b))
    return gate

