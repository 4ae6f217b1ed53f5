"""gpu: every convolution call of the benched train step, checked on its own operands against float64 (tests/convref.py).

bench.py's model (bench.build / bench.step_args) at the benched batch runs one AV and one audio-only train_step_async with
the visual trunk's sources and the U-Net's decoder pair on one stream (bench.py's instrumented pass).  Every Conv.fwd / dgrad /
dgrad_act / dgrad_up2x / wgrad call is shadowed: the library's result is compared element by element with the float64
reference of that call, |out - ref| <= tau * absref (absref: the same linear operation on |operands|), so a defect of one
launch variant at the true grid — a ragged tile, a split-K slab, a border — fails here even where the network-level
statistics of test_gpu_model.py would absorb it.

tau per (family, precision), stated once in convref.TAU: 4x the worst |out - ref| / absref measured over the four parameters
(configs 3 and 5, f32 and bf16), capped at the ceilings (2e-5 direct-form fp32 / bf16 on exactly modelled operands, 1.2e-4
Winograd).  The measured worst ratios, per family, precision and mode, are written next to each entry.  Two findings behind
the gate's form:
  * Winograd families are gated against tile_absref (convref.py): their rounding at one element scales with the terms of
    its transform tile.  With the direct-form absref, wino4_kernel (dgrad, 14x14 and 128x128) and winow4_kernel (wgrad,
    14x14, the visual fc conv whose dY is zero but at the max-pool's arg-max pixels) gave |out| of 3e-18 ... 2e-13 where
    every direct-form term is 0, and 1.47e-4 at an element of 5e-12 whose neighbours are 1e4 times larger.
  * B16 outputs are bf16(fp32 result): half a bf16 ulp is 2^-8 of the value at the bottom of a binade, so convbf_kernel's
    B16 outputs sit at ratio 0.99 of tau * absref + half an ulp for any tau; its tau is the ceiling.
"""
import ctypes
import gc
import os
import sys
import time

import pytest
import torch

import convref as R
from convref import CEIL_DIRECT, CEIL_WINO, TAU, WINOGRAD, tau_of    # noqa: F401  (the tolerances live beside the reference)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUST_F32 = ("wino4_kernel", "winow4_kernel", "wino_kernel", "wgrad4d_kernel", "conv3x3_kernel", "head_fwd_kernel",
            "head_dgrad_kernel", "head_wgrad_kernel")
MUST_BF16 = ("convbf_kernel", "wgradb_kernel")
ENTRY = {"fwd": "avsep_conv2d_fwd", "dgrad": "avsep_conv2d_dgrad", "dgrad_act": "avsep_conv2d_dgrad_act",
         "dgrad_up2x": "avsep_conv2d_dgrad_up2x", "wgrad": "avsep_conv2d_wgrad"}


class _Shadow:
    """Wraps Conv.pack (packed image -> the weight it was built from), the five Conv call methods (check every outermost call)
    and kernels.call (count what reaches the library's conv entry points); close() restores all of them."""

    def __init__(self, K, prec):
        self.K, self.prec, self.orig = K, prec, {}
        self.packed, self.rows, self.depth, self.controls = {}, [], 0, {}
        self.lib_calls, self.counting, self.checked, self.excluded, self.elements = {}, True, {}, 0, 0
        self._set(K.Conv, "pack", lambda cv, w, mode: self._pack(cv, w, mode))
        for name in ENTRY:
            self._set(K.Conv, name, self._call(name))
        self._set(K, "call", self._count)

    def _set(self, owner, name, fn):
        self.orig[(owner, name)] = getattr(owner, name)
        setattr(owner, name, fn)

    def close(self):
        for (owner, name), fn in self.orig.items():
            setattr(owner, name, fn)

    def _count(self, name, *a):
        if self.counting and name in ENTRY.values():
            self.lib_calls[name] = self.lib_calls.get(name, 0) + 1
        return self.orig[(self.K, "call")](name, *a)

    def _pack(self, cv, w, mode):
        out = self.orig[(self.K.Conv, "pack")](cv, w, mode)
        self.packed[out.data_ptr()] = (w, w._version)
        return out

    def _weight(self, w_packed):
        w, ver = self.packed[w_packed.data_ptr()]
        assert w._version == ver, "weight changed after it was packed"
        return w

    def _call(self, name):
        sh = self

        def wrapped(cv, *a, **kw):
            orig = sh.orig[(sh.K.Conv, name)]
            if sh.depth:                                       # the inner N = 1 call of a grid-image call
                return orig(cv, *a, **kw)
            sh.depth += 1
            try:
                return sh._shadow(name, orig, cv, a, kw)
            finally:
                sh.depth -= 1
        return wrapped

    # ---- one call ----------------------------------------------------------------------------------------------------------
    def _shadow(self, name, orig, cv, a, kw):
        K = self.K
        args = dict(zip(_PARAMS[name], a), **kw)
        snap = {k: args[k].clone() for k in ("stats", "bstats", "bstats1", "g0_acc") if args.get(k) is not None}
        out = orig(cv, *a, **kw)
        mode = {"fwd": "fwd", "wgrad": "wgrad"}.get(name, "dgrad")
        with_stats = args.get("stats") is not None
        family = cv.kernel_name(mode, with_stats)
        g = cv._grid_geometry({"fwd": 0, "wgrad": 2}.get(mode, 1))
        variant = _variant(K, cv._grid_desc(g) if g is not None else cv.d, mode, with_stats) + (",grid" if g is not None else "")
        bf = family in MUST_BF16
        x0, x1, sc0, sh0, sc1, sh1 = cv.keep[:6]
        op = dict(x0=x0, x1=x1, sc0=sc0, sh0=sh0, sc1=sc1, sh1=sh1, bf16=bf)
        if name == "fwd":
            op.update(w=self._weight(args["w_packed"]), bias=args.get("bias"), stats=with_stats)
            outs = {"y": out}
        elif name == "wgrad":
            op.update(dy=args["dy"], want_bias=bool(args.get("want_bias")))
            outs = {"dw": out[0], "dbias": out[1]}
        elif name == "dgrad_up2x":
            op.update(w=args["w"], dy=args["dy"], mean1=args.get("mean1"), invstd1=args.get("invstd1"),
                      bstats1=args.get("bstats1") is not None, g0_acc=snap.get("g0_acc"))
            outs = {"g0": out[0], "g1": out[1]}
        else:
            op.update(w=self._weight(args["w_packed_d"]), dy=args["dy"])
            outs = {"dx": out}
            if name == "dgrad_act":
                op.update({k: args.get(k) for k in ("y", "scale", "shift", "mean", "invstd", "residual", "res_scale", "res_shift",
                                                   "dz2", "add")})
                op.update(act=args["act"], bstats=args.get("bstats") is not None)
        for k, src in (("stats", "stats"), ("bstats", "bstats"), ("bstats1", "bstats1")):
            if k in snap:
                outs[k] = args[src] - snap[k]
        tau = tau_of(family, self.prec)
        ref = R.reference(cv, name, op)
        worst = (0.0, None)
        excl = ref.get("excluded")
        for k, o in outs.items():
            if o is None or k not in ref:
                continue
            r, ra = ref[k]
            if family in WINOGRAD and k in ("y", "dx", "dw"):
                ra = R.tile_absref(ra)
                ref[k] = (r, ra)
            res = R.check(o, r, ra, tau, b16=o.dtype == torch.bfloat16, excluded=excl if k == "dx" else None)
            if k == "dx" and excl is not None:
                self.excluded += res[4]
                self.elements += excl.numel()
            if res[0] >= worst[0]:
                worst = (res[0], (k,) + res[:4] + res[5:])
        key = (family, name)
        geom = (cv.N, cv.Cin, cv.H, cv.W, cv.Cout, cv.KH, cv.d.stride, cv.d.dil, cv.d.up2x)
        self.rows.append((family, variant, name, geom, worst[0] * tau, tau, worst[1]))
        self.checked[name] = self.checked.get(name, 0) + 1
        if key not in self.controls:
            self.controls[key] = self._controls(name, orig, cv, args, op, outs, ref, tau, snap)
        del ref
        return out

    # ---- negative controls: the gate must reject (a) a missing input channel, (b) a wrong border row, (c) one element off --
    def _controls(self, name, orig, cv, args, op, outs, ref, tau, snap):
        K = self.K
        k0 = next(k for k in ("y", "dx", "g0", "dw") if k in outs)
        out, (r, ra) = outs[k0], ref[k0]
        rejected = {}
        # (a) relaunch with input channel c of the weight zeroed for every tap (wgrad, which takes no weight: the result's
        # input channel c is dropped instead)
        if name == "wgrad":
            bad = out.clone()
            c = int(ra.sum((0, 2, 3)).argmax())
            bad[:, c] = 0
        else:
            w = op["w"]
            c = int((w.abs().sum((0, 2, 3)) * (R.nchw(op["x0"]).abs().sum((0, 2, 3)) if name == "fwd" and op["x1"] is None
                                               else 1.0)).argmax())
            w2 = w.clone()
            w2[:, c] = 0
            a2 = dict(args)
            if name == "dgrad_up2x":
                a2["w"] = w2
            else:
                a2["w_packed" if name == "fwd" else "w_packed_d"] = cv.pack(w2, 0 if name == "fwd" else 1)
            for k in ("stats", "bstats", "bstats1"):
                if a2.get(k) is not None:
                    a2[k] = torch.zeros_like(a2[k])
            if a2.get("g0_acc") is not None:
                a2["g0_acc"] = snap["g0_acc"].clone()
            self.counting = False
            try:
                o2 = orig(cv, **a2)
            finally:
                self.counting = True
            bad = {"fwd": lambda o: o, "dgrad": lambda o: o, "dgrad_act": lambda o: o, "dgrad_up2x": lambda o: o[0]}[name](o2)
            if name == "dgrad_up2x" and c >= cv.d.C0:
                bad, r, ra = o2[1], ref["g1"][0], ref["g1"][1]
        excl = ref.get("excluded") if k0 == "dx" else None
        rejected["a"] = R.check(bad, r, ra, tau, b16=bad.dtype == torch.bfloat16, excluded=excl)[0]
        # (b) one border row of the last image zeroed (the last kernel row of dw): the row whose reference is largest
        r, ra = ref[k0]
        o = R.nchw(out).to(torch.float64).reshape(r.shape).clone()
        rows = (-1, 0)
        row = max(rows, key=lambda i: float(r[-1, :, i, :].abs().sum()))
        o[-1, :, row, :] = 0
        b16 = out.dtype == torch.bfloat16
        rejected["b"] = R.check(o, r, ra, tau, b16=b16, excluded=excl)[0]
        # (c) one element off by 8 times its bound: 8 tau absref (+ 8 half bf16 ulps of a B16 output)
        o = R.nchw(out).to(torch.float64).reshape(r.shape).clone()
        i = int(ra.reshape(-1).argmax())
        o.view(-1)[i] += 8 * (tau * float(ra.reshape(-1)[i]) + (float(R.half_ulp_bf16(r.reshape(-1)[i])) if b16 else 0.0))
        rejected["c"] = R.check(o, r, ra, tau, b16=b16, excluded=excl)[0]
        return rejected


_PARAMS = {
    "fwd": ("w_packed", "bias", "stats", "out_b16"),
    "dgrad": ("w_packed_d", "dy", "out_b16"),
    "dgrad_act": ("w_packed_d", "dy", "y", "scale", "shift", "mean", "invstd", "act", "bstats", "residual", "res_scale",
                  "res_shift", "dz2", "add"),
    "dgrad_up2x": ("w", "dy", "mean1", "invstd1", "bstats1", "g0_acc"),
    "wgrad": ("dy", "want_bias", "out", "out_bias"),
}


def _variant(K, d, mode, with_stats):
    buf = ctypes.create_string_buffer(128)
    assert K.lib.load().avsep_conv_kernel_variant(ctypes.byref(d), {"fwd": 0, "dgrad": 1, "wgrad": 2}[mode], int(with_stats),
                                                   buf, 128) == 0
    return buf.value.decode()


def _fp64_path_is_exact(dev):
    """torch's float64 convolution on the GPU (native im2col + GEMM: MIOpen has no fp64 convolution) against the CPU."""
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(2, 64, 30, 34, generator=g), torch.randn(96, 64, 3, 3, generator=g)
    for s, p, d in ((1, 1, 1), (2, 1, 1), (1, 2, 2)):
        outs = []
        for t in ("cpu", dev):
            xx, ww = x.double().to(t).requires_grad_(True), w.double().to(t).requires_grad_(True)
            y = torch.nn.functional.conv2d(xx, ww, None, s, p, d)
            gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).double().to(t)
            outs.append([y] + list(torch.autograd.grad(y, (xx, ww), gy)))
        for a, b in zip(*outs):
            e = ((a - b.cpu()).abs().max() / a.abs().max()).item()
            assert e <= 1e-12, (s, p, d, e)


PARAMS = [(3, "f32"), (3, "bf16"), (5, "f32"), (5, "bf16")]


@pytest.mark.parametrize("config,prec", PARAMS, ids=[f"config{c}-{p}" for c, p in PARAMS])
def test_benched_conv_calls_vs_float64(dev, config, prec):
    import avsep_amd as P
    sys.path.insert(0, ROOT)
    import bench
    K = P.kernels
    t0 = time.time()
    _fp64_path_is_exact(dev)
    B = bench.BATCH_PER_GPU if config == 3 else bench.CONFIG5_BATCH
    K.set_precision(prec)
    sh = None
    try:
        a, snd, frm, wrap = bench.build(P, dev, 1234, "hip", config)
        wrap.fork_sources = snd.fork_pair = False
        opt = P.create_optimizer((snd, frm), a)
        raw = P.synth.make_batch(B, a.num_mix, a.num_frames, 224, a.audLen, seed=1235, device=dev)
        sh = _Shadow(K, prec)
        for use_vis in (True, False):
            batch = {"audios": list(raw["audios"]), "audio_mix": raw["audio_mix"], "frames": list(raw["frames"])}
            err, _, _ = P.net_wrapper.train_step_async(wrap, batch, opt, use_vis, a)
            assert torch.isfinite(err).all()
            torch.cuda.synchronize()
            gc.collect()
    finally:
        if sh is not None:
            sh.close()
        K.set_precision("f32")
    # ---- every conv call that reached the library was checked ----
    for name, entry in ENTRY.items():
        assert sh.checked.get(name, 0) == sh.lib_calls.get(entry, 0), (name, sh.checked, sh.lib_calls)
    assert sum(sh.checked.values()) > 150, sh.checked
    table = {}
    for family, variant, name, geom, worst, tau, where in sh.rows:
        row = table.setdefault((variant, name), [0, 0.0, tau, None])
        row[0] += 1
        if worst >= row[1]:
            row[1], row[3] = worst, (geom, where)
    print(f"\nconfig {config} {prec} batch {B}: {sum(sh.checked.values())} calls {sh.checked}, {time.time() - t0:.0f} s")
    print(f"{'variant':48s} {'mode':10s} {'calls':>5s} {'worst':>10s} {'tau':>8s}")
    for (variant, name), (n, worst, tau, _) in sorted(table.items()):
        print(f"{variant:48s} {name:10s} {n:5d} {worst:10.3e} {tau:8.1e}")
    fam = {}
    for family, variant, name, geom, worst, tau, where in sh.rows:
        f = fam.setdefault((family, name), [0.0, tau])
        f[0] = max(f[0], worst)
    print("family / mode worst ratio (|d| / absref):", {f"{k[0]}:{k[1]}": f"{v[0]:.3e}" for k, v in sorted(fam.items())})
    print(f"dgrad_act elements excluded (pre-activation within 2 ulps of 0): {sh.excluded} of {sh.elements}")
    print("negative controls (ratio, must be > 1):", {f"{k[0]}:{k[1]}": {c: f"{v:.2g}" for c, v in r.items()}
                                                     for k, r in sorted(sh.controls.items())})
    families = {r[0] for r in sh.rows}
    for must in (MUST_F32 if prec == "f32" else MUST_BF16):
        assert must in families, (must, sorted(families))
    assert sh.excluded <= 1e-6 * max(sh.elements, 1), (sh.excluded, sh.elements)
    bad = [(v, n, w, t, where) for (v, n), (cnt, w, t, where) in table.items() if not w <= t]
    for b in bad:
        print("OVER TAU:", b)
    assert not bad, bad
    fail = {k: r for k, r in sh.controls.items() if not all(v > 1.0 for v in r.values())}
    assert not fail, ("negative controls the gate did not reject", fail)


def test_winograd_shapes_at_the_top_of_the_32bit_range(dev):
    """N = 1547, C0 = Cout = 64, 45 x 241, 3x3 / s1 / p1: N*C*H*W = 2^30 - 64 elements, 4 GiB per tensor.  Every image of x and
    dY is zero except the first and the last, so the float64 reference is two single-image convolutions.  The Winograd
    kernels address through 32-bit buffer offsets (num_records 0xfffffff0) from a base moved back by up to 2W + 2 elements:
    the weight gradient, forward and data gradient of this shape must all equal the reference, the last image included."""
    import avsep_amd as P
    K = P.kernels
    N, C, H, W = 1547, 64, 45, 241
    assert N * C * H * W == 2 ** 30 - 64
    g = torch.Generator().manual_seed(9)
    ends = [torch.randn(C, H, W, generator=g) for _ in range(4)]
    w = (torch.randn(C, C, 3, 3, generator=g) / 24.0).to(dev)
    x = torch.zeros(N, C, H, W, device=dev)
    dy = torch.zeros(N, C, H, W, device=dev)
    x[0], x[-1], dy[0], dy[-1] = (t.to(dev) for t in ends)
    cv = K.Conv(x, C, 3, 1, 1, prec="f32")
    names = {m: cv.kernel_name(m, False) for m in ("fwd", "dgrad", "wgrad")}
    print("families at N = %d:" % N, names)
    geo = R.Geometry(2, C, H, W, C, 3, 1, 1)
    op = dict(x0=x[[0, -1]], w=w, dy=dy[[0, -1]], bf16=False)
    ratios = {}
    dw, _ = cv.wgrad(dy)
    ratios["wgrad"] = R.check(dw, *R.reference(geo, "wgrad", op)["dw"], tau_of(names["wgrad"], "f32"))
    y = cv.fwd(cv.pack(w, 0), None, None)
    ratios["fwd"] = R.check(y[[0, -1]], *R.reference(geo, "fwd", op)["y"], tau_of(names["fwd"], "f32"))
    inner = float(y[1:-1].abs().max())
    del y
    dx = cv.dgrad(cv.pack(w, 1), dy)
    ratios["dgrad"] = R.check(dx[[0, -1]], *R.reference(geo, "dgrad", op)["dx"], tau_of(names["dgrad"], "f32"))
    inner = max(inner, float(dx[1:-1].abs().max()))
    print("worst ratio (|d| / (tau absref), tensor index, ref, absref):", ratios, "max |zero images|:", inner)
    assert inner == 0.0
    for m, r in ratios.items():
        assert r[0] <= 1.0, (m, names[m], r)
