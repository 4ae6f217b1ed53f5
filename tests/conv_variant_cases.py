"""One test case per (mode, launch variant, precision) triple the stored conv dispatch table names (host only, no device).

tests/golden/conv_dispatch.json pins, for every descriptor of tools/conv_dispatch_table.py's sweep, the launch variant (family,
tile shape, workgroup size, split-K count) of its forward, data gradient and weight gradient.  cases() zips that sweep with
the stored index and keeps, for every distinct (mode, variant string, precision), the cheapest descriptor that takes it: the
fewest multiply-accumulates, a descriptor without an AVSEP_ALGO_NO_* bit before one with, then sweep order.  The list is
derived from the stored table alone; the library is never asked for it (tests/test_conv_variant_cases_host.py asks the
library whether it still agrees).

The cheapest descriptors are the interesting ones: a variant planned for batch 64 (plan_n) and launched at N = 1 runs on a
tiny grid, with partial last workgroups, empty split-K slabs and tiles that cross the only image.

operands(case) builds the call's tensors on the CPU from the case's seed, the way tests/test_gpu_ops.py does (randn inputs,
weights / sqrt(fan-in), scale in [0.5, 1.5], shift 0.3 randn, a bias); act_operands(case) those of dgrad_act, with every
pre-activation far from 0 (see there).
"""
import importlib.util
import json
import os
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_dispatch_table", os.path.join(ROOT, "tools", "conv_dispatch_table.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

COL = {c: i for i, c in enumerate(T.COLUMNS)}
MODES = ("fwd", "dgrad", "wgrad")
PREC_NAME = {0: "f32", 1: "bf16"}
# fixed caps on a case (conditions, not measurements): the multiply-accumulates of the call and the bytes of its largest
# fp32 tensor.  A future table that breaks one gets a smaller geometry in SUPPLEMENT, the pinned sweep is not edited.
MAX_MACS = 3_000_000_000
MAX_TENSOR_BYTES = 64 << 20
# (mode, variant, prec name) -> dict(geo=T.geo(...), n=, plan_n=, algo=, dgrad_act_fused=, head=): a geometry outside the sweep
# that reaches a triple whose every sweep descriptor breaks a cap.  The host test asks the library to confirm that each entry
# takes its variant and answers dgrad_act_fused / head as stated; its other routes are not pinned.
SUPPLEMENT = {}


class Case:
    """One (mode, variant, prec) triple and the descriptor that represents it."""

    def __init__(self, mode, variant, label, d, row, order):
        self.mode, self.variant, self.label, self.order = mode, variant, label, order
        self.geo_name = label.split(" ")[0]
        self.N, self.Cin, self.C0, self.H, self.W, self.Cout = d.N, d.Cin, d.C0, d.H, d.W, d.Cout
        self.KH, self.KW, self.stride, self.pad, self.dil = d.KH, d.KW, d.stride, d.pad, d.dil
        self.Ho, self.Wo = d.Ho, d.Wo
        self.C1 = d.Cin - d.C0
        self.aff0, self.aff1 = bool(d.scale0), bool(d.scale1)
        self.act0, self.act1, self.up2x = d.act0, d.act1, bool(d.up2x)
        self.prec, self.plan_n = PREC_NAME[d.prec], d.plan_n
        self.algo = next((k for k, v in _algo_bits().items() if v == d.algo), None) if d.algo else None
        assert (d.algo == 0) == (self.algo is None), d.algo
        # the four routes of the descriptor, as the table answers them
        self.expect = {"fwd_stats": row[COL["fwd_stats"]], "fwd": row[COL["fwd"]], "dgrad": row[COL["dgrad"]],
                       "wgrad": row[COL["wgrad"]]}
        self.dgrad_act_fused, self.head = int(row[COL["dgrad_act_fused"]]), int(row[COL["head"]])
        self.io = {m: tuple(row[COL["io%d" % i]]) for i, m in enumerate(MODES)}      # (rc, input format, B16 output allowed)
        self.family = variant.split(":")[0]
        self.macs = macs(d)
        self.tensor_bytes = tensor_bytes(d)
        self.id = f"{mode}-{self.prec}-{variant}"
        self.seed = zlib.crc32(self.id.encode()) & 0x7FFFFFFF

    @property
    def k(self):
        return self.KH if self.KH == self.KW else (self.KH, self.KW)

    @property
    def plan_batch_scale(self):
        """kernels.plan_batch_scale that makes a Conv over N images carry this case's plan_n."""
        if self.plan_n == 0:
            return 1
        assert self.plan_n % self.N == 0 and self.plan_n != self.N, (self.plan_n, self.N)
        return self.plan_n // self.N

    def desc(self):
        """The sweep's descriptor of this case (host queries only: its pointers are dummies)."""
        import avsep_amd as P
        d = P.lib.ConvDesc()
        d.N, d.Cin, d.H, d.W, d.Cout, d.Ho, d.Wo = self.N, self.Cin, self.H, self.W, self.Cout, self.Ho, self.Wo
        d.KH, d.KW, d.stride, d.pad, d.dil = self.KH, self.KW, self.stride, self.pad, self.dil
        d.C0, d.act0, d.act1, d.up2x = self.C0, self.act0, self.act1, int(self.up2x)
        d.prec, d.plan_n = {"f32": 0, "bf16": 1}[self.prec], self.plan_n
        d.algo = _algo_bits()[self.algo] if self.algo else 0
        d.x0 = T.DUMMY
        if self.aff0:
            d.scale0 = d.shift0 = T.DUMMY
        if self.C1:
            d.x1 = T.DUMMY
        if self.aff1:
            d.scale1 = d.shift1 = T.DUMMY
        return d

    def geometry(self):
        return (f"{self.geo_name} N={self.N} {self.Cin}x{self.H}x{self.W}->{self.Cout} k{self.KH}x{self.KW} s{self.stride} "
                f"p{self.pad} d{self.dil} plan_n={self.plan_n} algo={self.algo or '-'}")

    def __repr__(self):
        return f"Case({self.id}: {self.geometry()})"


def _algo_bits():
    import avsep_amd as P
    return P.lib.ALGO_NO


def macs(d):
    return d.N * d.Cin * d.Cout * d.Ho * d.Wo * d.KH * d.KW


def tensor_bytes(d):
    """Bytes of the call's largest fp32 tensor: the virtual input, the output, the weight."""
    return 4 * max(d.N * d.Cin * d.H * d.W, d.N * d.Cout * d.Ho * d.Wo, d.Cout * d.Cin * d.KH * d.KW)


def stored_table():
    with open(T.TABLE) as f:
        return json.load(f)


def triples_of(row, prec):
    """The (mode, variant, prec name) triples one answer row names."""
    out = [("fwd", row[COL["fwd_stats"]], PREC_NAME[prec]), ("dgrad", row[COL["dgrad"]], PREC_NAME[prec]),
           ("wgrad", row[COL["wgrad"]], PREC_NAME[prec])]
    if row[COL["fwd"]] != row[COL["fwd_stats"]]:
        out.append(("fwd", row[COL["fwd"]], PREC_NAME[prec]))
    return out


def table_triples(stored=None):
    """Every triple of the stored table (the closure test compares the case list with this)."""
    stored = stored or stored_table()
    descs = list(T.sweep())
    assert len(descs) == len(stored["index"]), (len(descs), len(stored["index"]))
    return {t for (_, d), i in zip(descs, stored["index"]) for t in triples_of(stored["rows"][i], d.prec)}


_cases = None


def cases():
    """[Case], one per triple, sorted by (mode, prec, variant)."""
    global _cases
    if _cases is not None:
        return _cases
    stored = stored_table()
    descs = list(T.sweep())
    assert len(descs) == len(stored["index"]), (len(descs), len(stored["index"]))
    best = {}
    for order, ((label, d), i) in enumerate(zip(descs, stored["index"])):
        row = stored["rows"][i]
        key = (macs(d), d.algo != 0, order)
        for t in triples_of(row, d.prec):
            if t not in best or key < best[t][0]:
                best[t] = (key, label, d, row, order)
    out = []
    for (mode, variant, prec), (_, label, d, row, order) in best.items():
        c = Case(mode, variant, label, d, row, order)
        if c.macs > MAX_MACS or c.tensor_bytes > MAX_TENSOR_BYTES:
            assert (mode, variant, prec) in SUPPLEMENT, \
                f"{c!r} breaks a cap ({c.macs} MAC, {c.tensor_bytes} B): add a smaller geometry that takes it to SUPPLEMENT"
            c = _supplement_case(mode, variant, prec)
        assert c.macs <= MAX_MACS and c.tensor_bytes <= MAX_TENSOR_BYTES, (c, c.macs, c.tensor_bytes)
        out.append(c)
    _cases = sorted(out, key=lambda c: (MODES.index(c.mode), c.prec, c.variant))
    assert len({c.id for c in _cases}) == len(_cases)
    return _cases


def _supplement_case(mode, variant, prec):
    """A SUPPLEMENT entry as a Case: the table has no row for it, so the other routes are unknown (None) and the host test
    asks the library for `variant` alone."""
    import avsep_amd as P
    s = SUPPLEMENT[(mode, variant, prec)]
    g = s["geo"]
    kh, kw = (g["k"], g["k"]) if isinstance(g["k"], int) else g["k"]
    d = P.lib.ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout = s["n"], g["cin"] + g["c1"], g["h"], g["w"], g["cout"]
    d.KH, d.KW, d.stride, d.pad, d.dil = kh, kw, g["stride"], g["pad"], g["dil"]
    d.Ho = (g["h"] + 2 * g["pad"] - g["dil"] * (kh - 1) - 1) // g["stride"] + 1
    d.Wo = (g["w"] + 2 * g["pad"] - g["dil"] * (kw - 1) - 1) // g["stride"] + 1
    d.C0, d.act0, d.act1, d.up2x = g["cin"], g["act0"], g["act1"], int(g["up2x"])
    d.prec, d.plan_n, d.algo = {"f32": 0, "bf16": 1}[prec], s["plan_n"], s["algo"]
    d.x0 = T.DUMMY
    if g["aff0"]:
        d.scale0 = d.shift0 = T.DUMMY
    if g["c1"]:
        d.x1 = d.scale1 = d.shift1 = T.DUMMY
    row = [None] * len(T.COLUMNS)
    row[COL[{"fwd": "fwd_stats"}.get(mode, mode)]] = variant
    row[COL["dgrad_act_fused"]], row[COL["head"]] = s.get("dgrad_act_fused", 0), s.get("head", 0)
    for i in range(3):
        row[COL["io%d" % i]] = (0, 0, 0)
    return Case(mode, variant, f"{g['name']} (supplement)", d, row, -1)


# ---- operands ---------------------------------------------------------------------------------------------------------------
def operands(case):
    """CPU fp32 tensors of the case's call: x0 [, x1] (the LOW-RES sources of an up2x conv), sc0 / sh0 [, sc1 / sh1] where the
    descriptor folds an affine, w (OIHW), bias, dy."""
    c = case
    g = torch.Generator().manual_seed(c.seed)
    hs, ws = (c.H // 2, c.W // 2) if c.up2x else (c.H, c.W)
    op = {"x0": torch.randn(c.N, c.C0, hs, ws, generator=g), "x1": None, "sc0": None, "sh0": None, "sc1": None, "sh1": None}
    if c.C1:
        op["x1"] = torch.randn(c.N, c.C1, hs, ws, generator=g)
    if c.aff0:
        op["sc0"], op["sh0"] = torch.rand(c.C0, generator=g) + 0.5, torch.randn(c.C0, generator=g) * 0.3
    if c.aff1:
        op["sc1"], op["sh1"] = torch.rand(c.C1, generator=g) + 0.5, torch.randn(c.C1, generator=g) * 0.3
    op["w"] = torch.randn(c.Cout, c.Cin, c.KH, c.KW, generator=g) / (c.Cin * c.KH * c.KW) ** 0.5
    op["bias"] = torch.randn(c.Cout, generator=g)
    op["dy"] = torch.randn(c.N, c.Cout, c.Ho, c.Wo, generator=g)
    return op


def _away_from_zero(shape, g):
    """Values of either sign with 0.25 <= |t|."""
    t = torch.randn(shape, generator=g)
    return torch.where(t >= 0, 1.0, -1.0) * (0.25 + t.abs())


def act_operands(case):
    """The extra operands of dgrad_act (ReLU, BatchNorm-backward sums, a residual behind its own affine, dz2 and add), CPU fp32.

    convref leaves out of the check every element whose pre-activation pre = fmaf(y, scale, shift) + fmaf(r, rs, rh) lies
    within 2 fp32 ulps of (|pre1| + |pre2|) around 0, where the kernel's mask is undecidable.  Here none does: a target t
    with 0.25 <= |t| is drawn per element and y = (t - shift) / scale, so pre1 = t up to a few ulps of |t| + |shift|; the
    residual's term is built the same way from a target of t's sign, so |pre| = |pre1| + |pre2| up to rounding, 2^22 times the
    exclusion band.  `add` is kept away from 0 as well, which makes absref strictly positive where the ReLU mask is 0."""
    c = case
    g = torch.Generator().manual_seed(c.seed ^ 0x5A5A5A5)
    shape = (c.N, c.Cin, c.H, c.W)
    ch = lambda t: t.view(1, -1, 1, 1)
    a = {"scale": torch.rand(c.Cin, generator=g) + 0.5, "shift": torch.randn(c.Cin, generator=g) * 0.3,
         "res_scale": torch.rand(c.Cin, generator=g) + 0.5, "res_shift": torch.randn(c.Cin, generator=g) * 0.3}
    t = _away_from_zero(shape, g)
    a["y"] = ((t - ch(a["shift"])) / ch(a["scale"])).contiguous()
    u = torch.where(t >= 0, 1.0, -1.0) * (0.25 + torch.randn(shape, generator=g).abs())
    a["residual"] = ((u - ch(a["res_shift"])) / ch(a["res_scale"])).contiguous()
    a["dz2"] = torch.randn(shape, generator=g)
    a["add"] = _away_from_zero(shape, g)
    a["mean"] = a["y"].mean((0, 2, 3))
    a["invstd"] = 1.0 / (a["y"].var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    return a


def head_operands(case):
    """dgrad_up2x's BatchNorm-backward operands for the second source, and the g0 it accumulates into."""
    c = case
    g = torch.Generator().manual_seed(c.seed ^ 0x3C3C3C3)
    x1 = operands(c)["x1"]
    return {"mean1": x1.mean((0, 2, 3)), "invstd1": 1.0 / (x1.var((0, 2, 3), unbiased=False) + 1e-5).sqrt(),
            "g0_acc": torch.randn(c.N, c.C0, c.H // 2, c.W // 2, generator=g)}
