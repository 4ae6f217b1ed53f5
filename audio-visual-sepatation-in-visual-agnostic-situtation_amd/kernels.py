"""Tensor-level wrappers over the C ABI (one Python function per entry point of include/avsep.h).

Only shape bookkeeping, output allocation and operand checks happen here; all arithmetic is in
libavsep_gfx950.so.  Tensors are dense and live on a cuda device: activations are fp32 NCHW or
B16 images (bfloat16 [N, C/16, H, W, 16], see "storage formats" below), the conv wrappers
convert between the two at a kernel's door, and the audio, frame and scoring entry points take
the dtypes their docstrings name (uint8 file bytes, int32 tables, float64 sums).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import lib
from .lib import ConvDesc, CatDesc, call, ptr


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


# ---- storage formats (include/avsep.h AVSEP_FMT_*) ------------------------------------------------------------------------
# F32: dense fp32 [N,C,H,W].  B16: torch.bfloat16 of shape [N, C/16, H, W, 16] — the channel-blocked image the bf16 kernels
# stage with one 16-byte load per (position, 8-channel half).  A tensor's dtype IS its format tag.
FMT_F32, FMT_B16 = 0, 1


def is_b16(t):
    return t is not None and t.dtype == torch.bfloat16


def fmt_of(t):
    return FMT_B16 if is_b16(t) else FMT_F32


def dims(t):
    """(N, C, H, W) of an activation tensor in either format."""
    if is_b16(t):
        N, CB, H, W, _ = t.shape
        return N, CB * 16, H, W
    return tuple(t.shape)


def channels(t):
    return t.shape[1] * 16 if is_b16(t) else t.shape[1]


def per_channel(t):
    """Elements per channel (the BatchNorm count N*H*W)."""
    return t.numel() // channels(t)


def _b16(shape_nchw, like):
    N, Cc, H, W = shape_nchw
    return torch.empty((N, Cc // 16, H, W, 16), dtype=torch.bfloat16, device=like.device)


class _Mark:
    """Where and when something was built that another HIP stream may read later: the one body of the host layer's
    multi-stream rule (the twin cache, the pack cache and the BatchNorm order of fork_streams).  `_Mark(t)` is made right
    after the launches that build it, on the current stream of t's device; a host tensor leaves an empty mark."""
    __slots__ = ("event", "stream")

    def __init__(self, t):
        self.event = self.stream = None
        if t.is_cuda:
            self.event, self.stream = torch.cuda.Event(), torch.cuda.current_stream(t.device)
            self.event.record(self.stream)

    def reach(self, *tensors):
        """Order the current stream behind the mark if it is another one than the producer's, and keep the memory of
        `tensors` from being handed out again before this stream is done with it."""
        if self.event is None:
            return
        cur = torch.cuda.current_stream(self.stream.device)
        if cur != self.stream:
            cur.wait_event(self.event)
            for t in tensors:
                t.record_stream(cur)


def _twin_hit(t):
    """The remembered other-format twin of `t` if it is current (two passes that share a tensor may run on forked streams)."""
    twin = getattr(t, "_avsep_twin", None)
    if twin is None or twin[1] != t._version:
        return None
    twin[2].reach(twin[0])
    return twin[0]


def _twin_set(t, out):
    mark = _Mark(t)
    t._avsep_twin = (out, t._version, mark)
    out._avsep_twin = (t, out._version, mark)


def to_b16(t):
    """B16 image of an fp32 NCHW tensor (one HBM pass).  The converted twin is remembered on the tensor object, so an operand
    that several kernels of a step need in the other format (the forward and the weight gradient of a conv) is converted once."""
    if t is None or is_b16(t):
        return t
    twin = _twin_hit(t)
    if twin is not None:
        return twin
    N, Cc, H, W = t.shape
    out = _b16((N, Cc, H, W), t)
    call("avsep_f32_to_b16", ptr(t), N, Cc, H * W, ptr(out))
    _twin_set(t, out)
    return out


def to_f32(t):
    if t is None or not is_b16(t):
        return t
    twin = _twin_hit(t)
    if twin is not None:
        return twin
    N, Cc, H, W = dims(t)
    out = _f32((N, Cc, H, W), t)
    call("avsep_b16_to_f32", ptr(t), N, Cc, H * W, ptr(out))
    _twin_set(t, out)
    return out


def as_fmt(t, fmt):
    return to_b16(t) if fmt == FMT_B16 else to_f32(t)


def b16_ok(c):
    """May a [N,c,H,W] tensor be kept as a B16 image?"""
    return c % 16 == 0


def want_b16(c=16):
    """Activations between the bf16 kernels are kept as B16 images when the arithmetic mode is bf16 (set_precision)."""
    return _precision == 1 and b16_ok(c)


# bf16 mode: weight gradients of the <= 8x8 maps (the deep U-Net levels) run over ONE grid image of the whole batch instead of
# one mostly empty 256-pixel chunk per image (csrc/b16.hip: avsep_b16_grid_pack)
grid_small_maps = os.environ.get("AVSEP_GRID_SMALL_MAPS", "1") != "0"


def grid_pack(x, n, c, h, w, gx, gy, py, px, sc=None, sh=None, act=0):
    """B16 grid image [1, c/16, gy*py, gx*px, 16] of the n small maps of x (fp32 NCHW or B16), act(affine(.)) applied, zeros
    everywhere else."""
    out = _b16((1, c, gy * py, gx * px), x)
    call("avsep_b16_grid_pack", ptr(x), fmt_of(x), n, c, h, w, gx, py, px, gy * py, gx * px, ptr(sc), ptr(sh), act, ptr(out))
    return out


# Operand precision of the convolutions: "f32" (exact f32 MFMA, the reference's arithmetic) or "bf16" (operands rounded
# to bf16 while they are staged, fp32 accumulation / BatchNorm statistics / outputs / master weights: BASELINE.json
# configs[2]).  Geometries without a bf16 kernel run in f32 either way.
PREC_BY_NAME = {"f32": 0, "fp32": 0, "bf16": 1}
_precision = PREC_BY_NAME[os.environ.get("AVSEP_PRECISION", "f32")]


def set_precision(name):
    global _precision
    _precision = PREC_BY_NAME[name]


def get_precision():
    return "bf16" if _precision else "f32"


# Kernel families the convolutions must NOT use (avsep_conv_desc.algo, a bit set of lib.ALGO_NO values): A/B runs and the
# gradient-error attribution (tools/grad_attribution.py).  The library itself reads no environment variable; this host
# layer takes the initial mask from AVSEP_ALGO_NO="winograd,flat,..." (or the older per-family AVSEP_NO_<FAMILY>=1 names) once,
# at import, and every descriptor built afterwards carries the module's current mask.
def _algo_from_env():
    mask = 0
    for name in os.environ.get("AVSEP_ALGO_NO", "").replace(" ", "").split(","):
        if name:
            mask |= lib.ALGO_NO[name.lower()]
    for name, bit in lib.ALGO_NO.items():
        if os.environ.get("AVSEP_NO_" + name.upper()) is not None:
            mask |= bit
    return mask


algo_mask = _algo_from_env()
conv_tune = 0      # avsep_conv_desc.tune (tools/conv_bench.py only)


def set_algo_mask(*names):
    """set_algo_mask("winograd", ...) — forbid those kernel families from now on; set_algo_mask() clears the mask."""
    global algo_mask
    algo_mask = 0
    for n in names:
        algo_mask |= lib.ALGO_NO[n]
    return algo_mask


# Batch the launch heuristics are planned for, as a multiple of the real batch (avsep_conv_desc.plan_n): the parity tests
# set 8 so that a batch-8 step takes, layer by layer, the kernel instantiations of the batch-64 step bench.py times.
plan_batch_scale = 1


_pack_cache = None


class pack_scope:
    """`with pack_scope():` — packed weight images are cached for the duration (Conv.pack).  train_step_async wraps
    forward + backward, the optimizer step comes after; an in-place update of a weight inside a scope changes the tensor's
    version counter, which is part of the cache key, so the image is rebuilt instead of going stale."""

    def __enter__(self):
        global _pack_cache
        self.prev, _pack_cache = _pack_cache, ({} if _pack_cache is None else _pack_cache)
        return self

    def __exit__(self, *exc):
        global _pack_cache
        _pack_cache = self.prev
        return False


CONV_MODES = {"fwd": 0, "dgrad": 1, "wgrad": 2}     # the `mode` of the avsep_conv_* queries


def out_size(h, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


class Conv:
    """Geometry + virtual-input description of one convolution call (avsep_conv_desc).  Operands may be fp32 NCHW or B16
    images; each call asks the library which format its kernel stages (avsep_conv_io_formats) and converts at the door
    if the tensor it was given is in the other one."""

    def __init__(self, x0, cout, k, stride, pad, dil=1, x1=None, sc0=None, sh0=None, act0=0,
                 sc1=None, sh1=None, act1=0, up2x=False, prec=None):
        lib.require_gpu(x0)
        if x1 is not None:                       # two-source descriptors exist for the fp32 kernels only
            x0, x1 = to_f32(x0), to_f32(x1)
        N, C0, Hs, Ws = dims(x0)
        C1 = x1.shape[1] if x1 is not None else 0
        H, W = (2 * Hs, 2 * Ws) if up2x else (Hs, Ws)
        kh, kw = (k, k) if isinstance(k, int) else k
        self.N, self.Cin, self.H, self.W, self.Cout = N, C0 + C1, H, W, cout
        self.KH, self.KW = kh, kw
        self.Ho, self.Wo = out_size(H, kh, stride, pad, dil), out_size(W, kw, stride, pad, dil)
        self.keep = [x0, x1, sc0, sh0, sc1, sh1]
        d = ConvDesc()
        d.N, d.Cin, d.H, d.W, d.Cout, d.Ho, d.Wo = N, C0 + C1, H, W, cout, self.Ho, self.Wo
        d.KH, d.KW, d.stride, d.pad, d.dil = kh, kw, stride, pad, dil
        d.C0, d.act0, d.act1, d.up2x = C0, act0, act1, int(up2x)
        d.prec = _precision if prec is None else PREC_BY_NAME[prec]
        d.plan_n = N * plan_batch_scale if plan_batch_scale != 1 else 0
        d.algo, d.tune = algo_mask, conv_tune
        d.x0, d.x1 = ptr(x0), ptr(x1)
        d.xfmt = fmt_of(x0)
        d.scale0, d.shift0, d.scale1, d.shift1 = ptr(sc0), ptr(sh0), ptr(sc1), ptr(sh1)
        self.d = d
        self.ref = C.byref(d)
        self.like = x0
        self._grid_xg = None

    def io_formats(self, mode):
        """(format the inputs of this call must have, may the output be B16) — mode 0 fwd, 1 dgrad, 2 wgrad."""
        a, b = C.c_int32(0), C.c_int32(0)
        rc = lib.load().avsep_conv_io_formats(self.ref, mode, C.byref(a), C.byref(b))
        if rc != 0:
            raise lib.AvsepError(f"avsep_conv_io_formats failed ({rc})")
        return a.value, bool(b.value)

    def _x_as(self, fmt):
        """Hand the kernel x0 in the format it stages."""
        if self.d.xfmt != fmt:
            x = as_fmt(self.keep[0], fmt)
            self.keep.append(x)
            self.d.x0, self.d.xfmt = ptr(x), fmt

    def _out(self, shape_nchw, want, allowed):
        b = bool(want) and allowed and b16_ok(shape_nchw[1])
        return (_b16(shape_nchw, self.like) if b else _f32(shape_nchw, self.like)), (FMT_B16 if b else FMT_F32)

    def pack(self, w, mode):
        """Operand image of `w` for this call (mode 0 forward, 1 data gradient).  Inside a `pack_scope()` — one train step,
        during which the weights do not change — the image of a (weight, geometry, mode) is built once and shared: the
        second decoder pass of an AV step and the visual trunk's second source used to repack every weight (56 of the
        114 pack launches of a step)."""
        g = self._grid_geometry(0) if mode == 0 else None
        d = self._grid_desc(g) if g is not None else self.d      # a grid forward multiplies by the N = 1 conv's weight image
        ref = C.byref(d)
        key = None
        if _pack_cache is not None:
            key = (w.data_ptr(), w._version, mode, d.N, d.Cin, d.H, d.W, d.Cout, d.KH, d.KW, d.stride, d.pad, d.dil, d.C0, d.up2x, d.prec,
                   d.plan_n, bool(d.scale0), bool(d.scale1), d.act0, d.act1, d.algo, d.tune)
            hit = _pack_cache.get(key)
            if hit is not None:
                hit[2].reach(hit[0])         # streams may share the cache (fork_streams, and the backward of such passes)
                return hit[0]
        n = lib.load().avsep_conv_packed_floats(ref, mode)
        out = _f32((n,), w)
        call("avsep_conv_pack_weights", ref, ptr(w), ptr(out), mode)
        if key is not None:
            # holding `w` keeps a temporary weight tensor's address from being reused
            _pack_cache[key] = (out, w, _Mark(out))
        return out

    def _grid_geometry(self, mode=2):
        """(images per grid row, grid rows, input pitch, output pitch) when this call runs over a grid image of the batch
        (bf16 mode, one source, maps of at most 8x8, avsep_b16_grid_pack): the weight gradient (mode 2) of 3x3 / pad 1 and
        4x4 / stride 2 / pad 1, the forward (mode 0) of 4x4 / stride 2 / pad 1.  None otherwise."""
        if mode not in (0, 2):
            return None
        key = (mode, grid_small_maps)
        memo = self.__dict__.setdefault("_grid_memo", {})
        hit = memo.get(key, 0)
        if hit != 0:
            return hit
        memo[key] = g = self._grid_geometry_of(mode)
        return g

    def _grid_geometry_of(self, mode):
        d = self.d
        if not (grid_small_maps and d.prec == 1 and self.keep[1] is None and not d.up2x and d.dil == 1 and
                self.N >= 2 and b16_ok(self.Cin) and b16_ok(self.Cout) and max(self.H, self.W) <= 8):
            return None
        geo = (self.KH, self.KW, d.stride, d.pad)
        if geo == (3, 3, 1, 1) and mode == 2:
            pin = pout = (self.H + 1, self.W + 1)
        elif geo == (4, 4, 2, 1) and self.H % 2 == 0 and self.W % 2 == 0:
            pin, pout = (self.H + 2, self.W + 2), (self.H // 2 + 1, self.W // 2 + 1)
        else:
            return None
        gx = 1
        while gx * gx < self.N:
            gx += 1
        g = (gx, (self.N + gx - 1) // gx, pin, pout)
        # only where the grid image is large enough for the bf16 kernel of that mode (two 2x2 maps are not)
        name = lib.load().avsep_conv_kernel_name(C.byref(self._grid_desc(g)), mode, 0).decode()
        return g if name == ("wgradb_kernel" if mode == 2 else "convbf_kernel") else None

    def _grid_x(self, g):
        """The grid image of this call's activated input, shared by its forward and its weight gradient."""
        x0, _, sc0, sh0 = self.keep[:4]
        hit = self._grid_xg
        if hit is not None and hit[0] is x0 and hit[1] == x0._version:
            return hit[2]
        gx, gy, (pyi, pxi), _ = g
        xg = grid_pack(x0, self.N, self.Cin, self.H, self.W, gx, gy, pyi, pxi, sc0, sh0, self.d.act0)
        self._grid_xg = (x0, x0._version, xg)
        return xg

    def _grid_inner(self, g):
        gx, gy, _, (pyo, pxo) = g
        d = self.d
        inner = Conv(self._grid_x(g), self.Cout, (self.KH, self.KW), d.stride, d.pad, d.dil, prec="bf16")
        if (inner.Ho, inner.Wo) != (gy * pyo, gx * pxo):
            raise lib.AvsepError("grid image geometry")
        return inner

    def _grid_desc(self, g):
        """Descriptor of the N = 1 convolution over the grid images (geometry only: for the dispatch queries)."""
        gx, gy, (pyi, pxi), (pyo, pxo) = g
        d = ConvDesc.from_buffer_copy(self.d)
        d.N, d.H, d.W, d.Ho, d.Wo, d.plan_n = 1, gy * pyi, gx * pxi, gy * pyo, gx * pxo, 0
        d.scale0 = d.shift0 = None
        d.act0, d.xfmt = 0, FMT_B16
        return d

    def _ws(self, query):
        nbytes = getattr(lib.load(), query)(self.ref)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=self.like.device) if nbytes else None
        return ws, nbytes

    def fwd(self, w_packed, bias=None, stats=None, out_b16=None):
        """`out_b16`: ask for the output as a B16 image (default: whenever the arithmetic mode keeps B16 activations);
        granted when this call's kernel can write one, else the result is fp32 NCHW."""
        g = self._grid_geometry(0)
        if g is not None:                            # small maps: one conv over the grid image of the batch, then the real positions
            gx, gy, _, (pyo, pxo) = g
            yg = self._grid_inner(g).fwd(w_packed, bias, None, out_b16=False)
            y, self.d.yfmt = self._out((self.N, self.Cout, self.Ho, self.Wo), want_b16(self.Cout) if out_b16 is None else out_b16, True)
            call("avsep_grid_unpack", ptr(yg), self.N, self.Cout, self.Ho, self.Wo, gx, pyo, pxo, gy * pyo, gx * pxo, ptr(y),
                 self.d.yfmt, ptr(stats))
            return y
        need, allowed = self.io_formats(0)
        self._x_as(need)
        y, self.d.yfmt = self._out((self.N, self.Cout, self.Ho, self.Wo), want_b16(self.Cout) if out_b16 is None else out_b16,
                                   allowed)
        ws, nbytes = self._ws("avsep_conv2d_fwd_workspace_bytes")
        call("avsep_conv2d_fwd", self.ref, ptr(w_packed), ptr(bias), ptr(y), ptr(stats), ptr(ws), nbytes)
        return y

    def dgrad(self, w_packed_d, dy, out_b16=None):
        need, allowed = self.io_formats(1)
        dy = as_fmt(dy, need)
        self.d.dyfmt = need
        dx, self.d.dxfmt = self._out((self.N, self.Cin, self.H, self.W), want_b16(self.Cin) if out_b16 is None else out_b16,
                                     allowed)
        ws, nbytes = self._ws("avsep_conv2d_dgrad_workspace_bytes")
        call("avsep_conv2d_dgrad", self.ref, ptr(w_packed_d), ptr(dy), ptr(dx), ptr(ws), nbytes)
        return dx

    def dgrad_act_fused(self):
        """True when dgrad_act runs as ONE kernel (the activation gradient in the data-gradient kernel's epilogue)."""
        self.d.dxfmt = FMT_F32
        return bool(lib.load().avsep_conv2d_dgrad_act_fused(self.ref))

    def dgrad_act(self, w_packed_d, dy, y, scale, shift, mean, invstd, act, bstats, residual=None, res_scale=None,
                  res_shift=None, dz2=None, add=None):
        """act'(scale*y + shift [+ res_scale*residual + res_shift]) * (dgrad(dy) [+ dz2]) [+ add] and its BatchNorm-backward
        sums: avsep_conv2d_dgrad_act (fp32 tensors; the data gradient is never written unmasked)."""
        need, _ = self.io_formats(1)
        dy = as_fmt(dy, need)
        self.d.dyfmt = need
        self.d.dxfmt = FMT_F32
        dx = _f32((self.N, self.Cin, self.H, self.W), self.like)
        for t in (y, residual, dz2, add):
            if t is not None and (is_b16(t) or tuple(t.shape) != tuple(dx.shape) or not t.is_contiguous()):
                raise lib.AvsepError("dgrad_act operands must be dense fp32 tensors of dx's shape")
        e = lib.ActBwd(ptr(y), ptr(scale), ptr(shift), ptr(residual), ptr(res_scale), ptr(res_shift), ptr(dz2), ptr(add),
                       ptr(mean), ptr(invstd), ptr(bstats), int(act))
        ws, nbytes = self._ws("avsep_conv2d_dgrad_workspace_bytes")
        call("avsep_conv2d_dgrad_act", self.ref, ptr(w_packed_d), ptr(dy), C.byref(e), ptr(dx), ptr(ws), nbytes)
        return dx

    def kernel_name(self, mode, with_stats=True):
        """Kernel family the library dispatches this call to (mode: "fwd" | "dgrad" | "wgrad")."""
        ref = self.ref
        g = self._grid_geometry(CONV_MODES[mode])
        if g is not None:                            # the call runs on the grid image of the batch
            ref = C.byref(self._grid_desc(g))
        return lib.load().avsep_conv_kernel_name(ref, CONV_MODES[mode], int(with_stats)).decode()

    def kernel_variant(self, mode, with_stats=True, plan_n=None):
        """Family + the grid-size dependent launch decisions (tile shape, workgroup size, split-K) of this call; with
        `plan_n` the answer for a descriptor planned for that batch instead."""
        d = self.d
        if plan_n is not None:
            d = ConvDesc.from_buffer_copy(self.d)
            d.plan_n = plan_n
        buf = C.create_string_buffer(128)
        rc = lib.load().avsep_conv_kernel_variant(C.byref(d), CONV_MODES[mode], int(with_stats), buf, 128)
        if rc != 0:
            raise lib.AvsepError(f"avsep_conv_kernel_variant failed ({rc})")
        return buf.value.decode()

    def head_applicable(self):
        """True when this (up2x, Cout <= 4) conv takes the fused decoder-head kernels (csrc/head.hip)."""
        return bool(lib.load().avsep_conv2d_head_applicable(self.ref))

    def dgrad_up2x(self, w, dy, mean1=None, invstd1=None, bstats1=None, g0_acc=None):
        """Gradient wrt the two LOW-RES sources of an up2x conv (dgrad + transposed bilinear + ReLU mask fused)."""
        x0, x1 = self.keep[0], self.keep[1]
        g0 = g0_acc if g0_acc is not None else torch.empty_like(x0)
        g1 = torch.empty_like(x1) if x1 is not None else None
        ws, nbytes = self._ws("avsep_conv2d_dgrad_up2x_workspace_bytes")
        call("avsep_conv2d_dgrad_up2x", self.ref, ptr(w), ptr(to_f32(dy)), ptr(g0), ptr(g1), ptr(mean1), ptr(invstd1),
             ptr(bstats1), int(g0_acc is not None), ptr(ws), nbytes)
        return g0, g1

    def wgrad(self, dy, want_bias=False, out=None, out_bias=None):
        """dw (and dbias); `out` / `out_bias`: dense destinations to write into (e.g. a parameter's flat .grad view)."""
        shape = (self.Cout, self.Cin, self.KH, self.KW)
        if out is not None and (tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != torch.float32):
            raise lib.AvsepError("wgrad destination must be a dense fp32 OIHW tensor")
        g = self._grid_geometry(2)
        if g is not None:
            gx, gy, _, (pyo, pxo) = g
            dyg = grid_pack(dy, self.N, self.Cout, self.Ho, self.Wo, gx, gy, pyo, pxo)
            return self._grid_inner(g).wgrad(dyg, want_bias, out, out_bias)
        need, _ = self.io_formats(2)
        self._x_as(need)
        dy = as_fmt(dy, need)
        self.d.dyfmt = need
        dw = out if out is not None else _f32(shape, self.like)
        db = (out_bias if out_bias is not None else _f32((self.Cout,), self.like)) if want_bias else None
        nbytes = lib.load().avsep_conv2d_wgrad_workspace_bytes(self.ref)
        ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=self.like.device)
        call("avsep_conv2d_wgrad", self.ref, ptr(dy), ptr(dw), ptr(db), ptr(ws), nbytes)
        return dw, db


class _StatsArena:
    """Zeroed fp64 statistics buffers (BatchNorm sums, 2 x C doubles each) carved out of ONE device array that a single
    memset clears, instead of one fill launch per buffer (120 per train step).  Every consumer of a buffer (bn_finalize /
    bn_bwd_coeffs) is launched right after its producers on the same stream, so when the bump pointer wraps, the memset
    that re-clears the array is ordered after all of them; a slice handed out is never live across a wrap as long as no
    more than `capacity` doubles are requested between its allocation and its last use (a step uses ~40 K of the 2 M)."""

    def __init__(self, device, capacity=1 << 21):
        self.buf = torch.zeros((capacity,), dtype=torch.float64, device=device)
        self.cap, self.off, self.stream = capacity, 0, torch.cuda.current_stream(device)

    def take(self, n):
        n = (n + 15) // 16 * 16                        # 128-byte granules: atomics of two buffers never share a line
        if n > self.cap // 4 or torch.cuda.current_stream(self.buf.device) != self.stream:
            return None
        if self.off + n > self.cap:
            self.buf.zero_()
            self.off = 0
        out = self.buf[self.off:self.off + n]
        self.off += n
        return out


_arenas = {}


def zeros_stats(c, like):
    """[2*c] zeroed doubles on like.device (see _StatsArena)."""
    dev = like.device
    key = (dev, torch.cuda.current_stream(dev))        # one arena per stream: its re-clearing memset is ordered on that stream
    arena = _arenas.get(key)
    if arena is None:
        arena = _arenas[key] = _StatsArena(dev)
    out = arena.take(2 * c)
    if out is None:
        return torch.zeros((2 * c,), dtype=torch.float64, device=dev)
    return out[:2 * c]


def channel_stats(x, stats):
    x = to_f32(x)
    N, Cc = x.shape[:2]
    call("avsep_channel_stats", ptr(x), N, Cc, x.numel() // (N * Cc), ptr(stats))


class fork_streams:
    """`with fork_streams():` — independent passes of one network (the visual trunk over source 0, source 1, ...) are being
    issued on different HIP streams.  What they share is ordered with events instead of by the stream: a packed weight image
    is waited for by the streams that did not build it (Conv.pack), and the running-statistics update of a BatchNorm layer
    waits for the previous update of the same buffers — the passes update them in the order they were issued, exactly as
    if they had run back to back (vision_net.py:126-147 is called once per source, main.py:117-121)."""

    def __enter__(self):
        global _order
        self.prev, _order = _order, ({} if _order is None else _order)
        return self

    def __exit__(self, *exc):
        global _order
        _order = self.prev
        return False


_order = None      # fork_streams: running_mean.data_ptr() -> _Mark of the last update


def bn_finalize(stats, count, gamma, beta, rmean, rvar, momentum, eps, training, like, num_batches_tracked=None, updates=1):
    Cc = gamma.numel()
    out = _f32((4, Cc), like)  # scale, shift, mean, invstd
    ordered = _order is not None and training and rmean is not None
    if ordered:
        last = _order.get(rmean.data_ptr())
        if last is not None:
            last.reach()
    call("avsep_bn_finalize", ptr(stats), float(count), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar),
         float(momentum), float(eps), Cc, int(training), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
         ptr(num_batches_tracked), int(updates))
    if ordered:
        _order[rmean.data_ptr()] = _Mark(rmean)
    return out


def bn_bwd_coeffs(bstats, count, gamma, mean, invstd, dgamma=None, dbeta=None):
    """(dgamma, dbeta, pqr); `dgamma` / `dbeta`: destinations to write into instead of fresh tensors."""
    Cc = gamma.numel()
    dgamma = dgamma if dgamma is not None else _f32((Cc,), gamma)
    dbeta = dbeta if dbeta is not None else _f32((Cc,), gamma)
    pqr = _f32((3, Cc), gamma)
    call("avsep_bn_bwd_coeffs", ptr(bstats), float(count), ptr(gamma), ptr(mean), ptr(invstd), Cc,
         ptr(dgamma), ptr(dbeta), ptr(pqr))
    return dgamma, dbeta, pqr


def _drop_twin(t):
    """`t` is about to be overwritten through a raw pointer: forget its converted twin (to_b16 / to_f32 cache)."""
    if t is not None and hasattr(t, "_avsep_twin"):
        other = t._avsep_twin[0]
        if hasattr(other, "_avsep_twin") and other._avsep_twin[0] is t:
            del other._avsep_twin
        del t._avsep_twin


def _same_fmt(main, *others):
    """The elementwise kernels take all their tensor operands in ONE format: that of `main`."""
    f = fmt_of(main)
    return [as_fmt(o, f) for o in others]


def bn_bwd_apply_(dz, y, pqr, out=None, fresh=False, to_b16_out=False):
    """dy = p*dz + q*y + r per channel, in y's storage format; in place on dz unless `out` is given or `fresh` asks for a
    new tensor.  `to_b16_out` (fp32 dz and y, C % 16 == 0): write the result as a B16 image in the same pass — its consumers
    are bf16 kernels.  Returns the result tensor."""
    N, Cc, H, W = dims(y)
    if to_b16_out and not is_b16(y) and not is_b16(dz) and b16_ok(Cc):
        dst = _b16((N, Cc, H, W), y)
        call("avsep_bn_bwd_apply_to_b16", ptr(dz), ptr(y), ptr(pqr), N, Cc, H * W, ptr(dst))
        return dst
    (dz,) = _same_fmt(y, dz)
    dst = torch.empty_like(y) if fresh else (dz if out is None else out)
    _drop_twin(dst)
    if is_b16(y):
        call("avsep_b16_bn_bwd_apply", ptr(dz), ptr(y), ptr(pqr), N, Cc, H * W, ptr(dst))
    else:
        call("avsep_bn_bwd_apply", ptr(dz), ptr(y), ptr(pqr), N, Cc, H * W, ptr(dst))
    return dst


def affine_act(y, scale, shift, residual, act, res_scale=None, res_shift=None):
    N, Cc, H, W = dims(y)
    z = torch.empty_like(y)
    (residual,) = _same_fmt(y, residual)
    if is_b16(y):
        call("avsep_b16_affine_act", ptr(y), ptr(scale), ptr(shift), ptr(residual), ptr(res_scale), ptr(res_shift), act, N, Cc,
             H * W, ptr(z))
    else:
        call("avsep_affine_act", ptr(y), ptr(scale), ptr(shift), ptr(residual), ptr(res_scale), ptr(res_shift), act, N, Cc,
             H * W, ptr(z))
    return z


def affine_act_bwd_(dz, y, scale, shift, residual, add, mean, invstd, act, bstats, res_scale=None, res_shift=None,
                    out=None, dz2=None, stats_only=False):
    """dz <- act'(scale*y+shift[+res]) * (dz [+ dz2]) (+ add) (in place unless `out`); accumulates bstats.  All tensor
    operands are brought to the format of `y`; the (possibly converted) result tensor is returned."""
    N, Cc, H, W = dims(y)
    dz, dz2, residual, add = _same_fmt(y, dz, dz2, residual, add)
    dst = dz if out is None else out
    if stats_only and is_b16(y):       # the B16 kernel can skip the write (dz itself is the result: no activation, no add)
        call("avsep_b16_affine_act_bwd", ptr(dz), ptr(dz2), ptr(y), ptr(scale), ptr(shift), ptr(residual), ptr(res_scale),
             ptr(res_shift), ptr(add), ptr(mean), ptr(invstd), act, N, Cc, H * W, None, ptr(bstats))
        return dz
    _drop_twin(dst)
    if is_b16(y):
        call("avsep_b16_affine_act_bwd", ptr(dz), ptr(dz2), ptr(y), ptr(scale), ptr(shift), ptr(residual), ptr(res_scale),
             ptr(res_shift), ptr(add), ptr(mean), ptr(invstd), act, N, Cc, H * W, ptr(dst), ptr(bstats))
    else:
        call("avsep_affine_act_bwd", ptr(dz), ptr(dz2), ptr(y), ptr(scale), ptr(shift), ptr(residual), ptr(res_scale), ptr(res_shift),
             ptr(add), ptr(mean), ptr(invstd), act, N, Cc, H * W, ptr(dst), ptr(bstats))
    return dst


class Cat:
    """relu(affine(cat(x0, x1))) -> bilinear x2 (the U-Net decoder's glue).  Two B16 sources (no broadcast vector) run the
    B16 kernels and produce / consume B16 images; anything else runs the fp32 kernels on fp32 copies."""

    def __init__(self, x0, x1, sc0=None, sh0=None, sc1=None, sh1=None, bcast0=False, hw=None):
        self.b16 = (not bcast0 and x1 is not None and (is_b16(x0) or is_b16(x1)) and b16_ok(channels(x0))
                    and b16_ok(channels(x1)))
        if self.b16:
            x0, x1 = to_b16(x0), to_b16(x1)
        else:
            x0, x1 = to_f32(x0), to_f32(x1)
        N, C0 = (x0.shape[0], x0.shape[1]) if bcast0 else dims(x0)[:2]
        C1 = channels(x1) if x1 is not None else 0
        H, W = hw if hw is not None else (dims(x1)[2:] if x1 is not None else dims(x0)[2:])
        self.shape = (N, C0, C1, H, W)
        self.keep = (x0, x1, sc0, sh0, sc1, sh1)
        d = CatDesc()
        d.N, d.C0, d.C1, d.H, d.W, d.bcast0, d.bcast1 = N, C0, C1, H, W, int(bcast0), 0
        d.x0, d.x1 = ptr(x0), ptr(x1)
        d.scale0, d.shift0, d.scale1, d.shift1 = ptr(sc0), ptr(sh0), ptr(sc1), ptr(sh1)
        self.d, self.ref, self.like, self.bcast0 = d, C.byref(d), (x1 if x1 is not None else x0), bcast0

    def fwd(self):
        N, C0, C1, H, W = self.shape
        x0, x1, sc0, sh0, sc1, sh1 = self.keep
        if self.b16:
            out = _b16((N, C0 + C1, 2 * H, 2 * W), self.like)
            call("avsep_b16_relu_up2x_fwd", ptr(x0), ptr(x1), ptr(sc0), ptr(sh0), ptr(sc1), ptr(sh1), N, C0, C1, H, W, ptr(out))
            return out
        out = _f32((N, C0 + C1, 2 * H, 2 * W), self.like)
        call("avsep_relu_up2x_fwd", self.ref, ptr(out))
        return out

    def bwd(self, dout, mean1=None, invstd1=None, bstats1=None, g0_acc=None):
        """g0_acc: an existing source-0 gradient to accumulate into (shared-encoder AV step; must be in this Cat's format)."""
        N, C0, C1, H, W = self.shape
        x0, x1, sc0, sh0, sc1, sh1 = self.keep
        if self.b16:
            dout = to_b16(dout)
            g0 = g0_acc if g0_acc is not None else _b16((N, C0, H, W), self.like)
            assert is_b16(g0), "accumulating into an fp32 skip gradient from a B16 decoder level"
            _drop_twin(g0)
            g1 = _b16((N, C1, H, W), self.like)
            call("avsep_b16_relu_up2x_bwd", ptr(x0), ptr(x1), ptr(sc0), ptr(sh0), ptr(sc1), ptr(sh1), N, C0, C1, H, W, ptr(dout),
                 ptr(g0), ptr(g1), ptr(mean1), ptr(invstd1), ptr(bstats1), int(g0_acc is not None))
            return g0, g1
        dout = to_f32(dout)
        g0 = g0_acc if g0_acc is not None else _f32((N, C0) if self.bcast0 else (N, C0, H, W), self.like)
        assert not is_b16(g0)
        _drop_twin(g0)
        g1 = _f32((N, C1, H, W), self.like) if C1 else None
        call("avsep_relu_up2x_bwd", self.ref, ptr(dout), ptr(g0), ptr(g1), ptr(mean1), ptr(invstd1),
             ptr(bstats1), int(g0_acc is not None))
        return g0, g1


def prepare(mag_mix, mags, log_freq, weighted, binary, fout=256):
    """mag_mix [B,1,F,T]; mags [S,B,1,F,T] (one buffer).  Returns mix_w, mags_w, log, weight, gt."""
    lib.require_gpu(mag_mix)
    S, B, _, Fin, T = mags.shape
    Fo = fout if log_freq else Fin
    mix_w, logm, weight = (_f32((B, 1, Fo, T), mag_mix) for _ in range(3))
    mags_w, gt = _f32((S, B, 1, Fo, T), mag_mix), _f32((S, B, 1, Fo, T), mag_mix)
    call("avsep_prepare", ptr(mag_mix), ptr(mags), S, B, Fin, T, Fo, int(bool(log_freq)), int(bool(weighted)),
         int(bool(binary)), ptr(mix_w), ptr(mags_w), ptr(logm), ptr(weight), ptr(gt))
    return mix_w, mags_w, logm, weight, gt


def warp(x, hout, wout, warp_flag):
    B, Cc, Hin, Win = x.shape
    y = _f32((B, Cc, hout, wout), x)
    call("avsep_warp", ptr(x), B * Cc, Hin, Win, hout, wout, int(warp_flag), ptr(y))
    return y


def window_prepare(mag, starts, fout=256, width=256):
    """mag [Fin,F] (one recording), starts int32 [K] on the device -> warped magnitude and its log, [K,1,fout,width] each:
    per window what ``prepare`` / inference.NetWrapper.prepare_inferdata make of mag[:, s:s+width] (zero past F)."""
    lib.require_gpu(mag)
    Fin, F = mag.shape
    Kw = starts.numel()
    mix_w, logm = _f32((Kw, 1, fout, width), mag), _f32((Kw, 1, fout, width), mag)
    call("avsep_window_prepare", ptr(mag), Fin, F, ptr(starts), Kw, fout, width, ptr(mix_w), ptr(logm))
    return mix_w, logm


def window_agreement(masks, starts):
    """masks [K,N,Fout,W], starts int32 [K] -> float64 [K-1,N,N]: L1 distance of source i of window k and source j of
    window k+1 over the frames both windows cover (bit-identical from run to run)."""
    lib.require_gpu(masks)
    Kw, N, Fo, W = masks.shape
    D = torch.empty((max(Kw - 1, 0), N, N), dtype=torch.float64, device=masks.device)
    if Kw > 1:
        call("avsep_window_agreement", ptr(masks), ptr(starts), Kw, N, Fo, W, ptr(D))
    return D


def mask_stitch(masks, starts, perm, mag, binary, thres, want_mask=False):
    """masks [K,N,Fout,W], starts int32 [K], perm int32 [K,N], mag [Fin,F] -> per-source magnitude [N,Fin,F] (and the blended
    linear-frequency mask [N,Fin,F] with want_mask): un-warp, triangular cross-fade, threshold, x mag in one pass.
    mag [C,Fin,F], a recording that keeps its channels -> [N,C,Fin,F]: the mask at (n, f, t) is blended once and multiplied
    into the C magnitudes, so out[:, c] has the bits of mask_stitch(.., mag[c])."""
    lib.require_gpu(masks)
    Kw, N, Fo, W = masks.shape
    Cc, Fin, F = mag.shape if mag.dim() == 3 else (1, *mag.shape)
    out = _f32((N, Cc, Fin, F) if mag.dim() == 3 else (N, Fin, F), mag)
    lin = _f32((N, Fin, F), mag) if want_mask else None
    call("avsep_mask_stitch", ptr(masks), ptr(starts), ptr(perm), ptr(mag), Kw, N, Fo, W, Cc, Fin, F, int(bool(binary)),
         float(thres), ptr(out), ptr(lin))
    return out, lin


mask_stitch_channels = mask_stitch     # the name callers of the channel path know: mag [C,Fin,F] -> [N,C,Fin,F]


WINDOW_REDUCE_OPS = {"mean": 0, "max": 1}


def window_reduce_check(ranges, T):
    """The row conditions of separate.frames_of_windows on a (first, count) table, checked on the host: int32 [K,2] with
    1 <= K <= 65535 and, for every row, count >= 1, 0 <= first and first + count <= T.  AvsepError otherwise."""
    if not torch.is_tensor(ranges) or ranges.is_cuda or ranges.dtype != torch.int32 or ranges.dim() != 2 or ranges.shape[1] != 2 \
            or not 1 <= ranges.shape[0] <= 65535:
        raise lib.AvsepError(f"window_reduce takes ranges as int32 [K,2] (first, count) on the CPU with K in 1 ... 65535, got {lib.got(ranges)}")
    r = ranges.to(torch.int64)
    bad = (r[:, 1] < 1) | (r[:, 0] < 0) | (r[:, 0] + r[:, 1] > int(T))
    if bool(bad.any()):
        k = int(bad.nonzero()[0])
        raise lib.AvsepError(f"window_reduce: row {k} of the table, (first, count) = {tuple(ranges[k].tolist())}, does not lie "
                             f"within the {int(T)} frames (count >= 1, 0 <= first, first + count <= T)")


def window_reduce(f, ranges, op="mean"):
    """f [T, ...] float32 contiguous on the GPU, the per-frame visual features of a clip; ranges int32 [K,2] on the CPU, row k
    = (first, count), the frames of window k (separate.frames_of_windows) -> [K, ...]: per window the mean ('mean': fp32 sum
    in ascending frame order, one division) or the maximum ('max') over its frames, all windows in one launch."""
    if op not in WINDOW_REDUCE_OPS:
        raise lib.AvsepError(f"window_reduce takes op 'mean' or 'max', got {op!r}")
    if not torch.is_tensor(f) or f.dtype != torch.float32 or f.dim() < 1 or f.numel() < 1 or not f.is_contiguous():
        raise lib.AvsepError(f"window_reduce takes f as a contiguous float32 tensor [T, ...] with T >= 1, got {lib.got(f)}")
    T = f.shape[0]
    window_reduce_check(ranges, T)
    lib.require_gpu(f)
    Kw = ranges.shape[0]
    out = _f32((Kw,) + tuple(f.shape[1:]), f)
    table = ranges.contiguous().to(f.device)
    call("avsep_window_reduce", ptr(f), ptr(table), T, Kw, f.numel() // T, WINDOW_REDUCE_OPS[op], ptr(out))
    return out


MWF_MAX_CHANNELS = 8     # avsep_mwf_*: C and N up to 8
MWF_MAX_SOURCES = 8


def _mwf_check(what, ymag, yph):
    lib.require_gpu(ymag)
    lib.require_gpu(yph)
    if ymag.dim() != 4 or ymag.dtype != torch.float32 or yph.dtype != torch.float32 or yph.device != ymag.device \
            or tuple(yph.shape) not in (tuple(ymag.shape), tuple(ymag.shape[1:])):
        raise lib.AvsepError(f"{what} takes ymag f32 [N,C,Fin,F] and yph [C,Fin,F] (shared by the sources) or [N,C,Fin,F], got "
                             f"{ymag.dtype} {tuple(ymag.shape)} and {yph.dtype} {tuple(yph.shape)}")
    N, Cc, Fin, F = ymag.shape
    if not (1 <= N <= MWF_MAX_SOURCES and 1 <= Cc <= MWF_MAX_CHANNELS and Fin >= 1 and F >= 1):
        raise lib.AvsepError(f"{what}: 1 <= N <= {MWF_MAX_SOURCES}, 1 <= C <= {MWF_MAX_CHANNELS}, Fin, F >= 1; got {tuple(ymag.shape)}")
    return N, Cc, Fin, F


MWF_MIN_SPAN, MWF_MAX_SPAN = 64, 4096     # avsep_mwf_*_tv: the span H, a multiple of 64


def mwf_span_check(what, span):
    """The rule of include/avsep.h for the span of the time-varying covariances; 0 is the time-invariant filter."""
    if isinstance(span, bool) or not isinstance(span, int) or (span != 0 and not (
            MWF_MIN_SPAN <= span <= MWF_MAX_SPAN and span % 64 == 0)):
        raise lib.AvsepError(f"{what} takes the span as an int: 0 (one covariance for the whole recording) or a multiple of 64 "
                             f"frames in {MWF_MIN_SPAN} ... {MWF_MAX_SPAN}, got {span!r}")
    return span


def mwf_centres(F, span):
    """K of include/avsep.h: centres at frames 0, span, 2 span, ..., the last one at or past frame F - 1."""
    return 1 if F == 1 else -(-(F - 1) // span) + 1


def _mwf_cov(ymag, yph, span):
    """-> f32 [N, Fin, C, C, 2], or [N, K, Fin, C, C, 2] with a span: span == 0 calls the time-invariant entries, here and in
    _mwf_apply"""
    N, Cc, Fin, F = ymag.shape
    tv, H = ("_tv", (span,)) if span else ("", ())
    nbytes = getattr(lib.load(), f"avsep_mwf{tv}_workspace_bytes")(N, Cc, Fin, F, *H)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=ymag.device)
    cov = _f32((N, mwf_centres(F, span), Fin, Cc, Cc, 2) if span else (N, Fin, Cc, Cc, 2), ymag)
    call(f"avsep_mwf_cov{tv}", ptr(ymag), ptr(yph), int(yph.dim() == 4), N, Cc, Fin, F, *H, ptr(cov), ptr(ws), nbytes)
    return cov


def _mwf_apply(xmag, xph, ymag, cov, span, reg):
    N, Cc, Fin, F = ymag.shape
    tv, H = ("_tv", (span,)) if span else ("", ())
    out_mag, out_ph = _f32((N, Cc, Fin, F), ymag), _f32((N, Cc, Fin, F), ymag)
    call(f"avsep_mwf_apply{tv}", ptr(xmag), ptr(xph), ptr(ymag), ptr(cov), N, Cc, Fin, F, *H, reg, ptr(out_mag), ptr(out_ph))
    return out_mag, out_ph


def mwf_cov(ymag, yph, span=0):
    """Spatial covariance of every source per bin row: ymag [N,C,Fin,F], yph [C,Fin,F] (one phase for all sources) or
    [N,C,Fin,F] -> complex64 [N,Fin,C,C], R_n[f] = sum_t Y Y^H / max(sum_t mean_c |Y|^2, FLT_MIN) (trace C, or 0 for a source
    that is silent in the row).  Fixed summation order: the same bits on every call.
    ``span`` > 0 (a multiple of 64 frames in 64 ... 4096): one covariance per centre k * span, both sums weighted by the hat
    max(0, 1 - |t - k span| / span) -> complex64 [N,K,Fin,C,C], K = ceil((F - 1) / span) + 1 (a source that is silent over a
    centre's support has 0 there)."""
    _mwf_check("mwf_cov", ymag, yph)
    return torch.view_as_complex(_mwf_cov(ymag.contiguous(), yph.contiguous(), mwf_span_check("mwf_cov", span)))


def mwf(xmag, xph, ymag, yph, iterations=1, reg=1e-3, span=0):
    """Multichannel Wiener filter (include/avsep.h): xmag, xph [C,Fin,F] the channels' STFT, ymag [N,C,Fin,F] the source
    images' magnitudes (mask_stitch), yph their phase, [C,Fin,F] shared or [N,C,Fin,F] -> (mag, phase), both
    [N,C,Fin,F], after ``iterations`` passes (each pass re-estimates the covariances from the previous pass's output).
    ``reg`` is relative to each bin's power: the sources sum to X / (1 + ~reg).
    ``span`` = 0: one covariance per source and bin row for the whole recording.  ``span`` > 0 (a multiple of 64 frames in
    64 ... 4096): time-varying covariances, one per centre k * span, and every frame is filtered with the blend of the two
    centres next to it; for sources that move through the image."""
    N, Cc, Fin, F = _mwf_check("mwf", ymag, yph)
    lib.require_gpu(xmag)
    lib.require_gpu(xph)
    for name, t in (("xmag", xmag), ("xph", xph)):
        if t.dtype != torch.float32 or tuple(t.shape) != (Cc, Fin, F) or t.device != ymag.device:
            raise lib.AvsepError(f"mwf takes {name} f32 [{Cc},{Fin},{F}] on {ymag.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    iterations, reg = int(iterations), float(reg)
    if iterations < 1 or not reg >= 0.0:
        raise lib.AvsepError(f"mwf needs iterations >= 1 and reg >= 0, got {iterations} and {reg}")
    mwf_span_check("mwf", span)
    xmag, xph, mag, ph = xmag.contiguous(), xph.contiguous(), ymag.contiguous(), yph.contiguous()
    for _ in range(iterations):
        mag, ph = _mwf_apply(xmag, xph, mag, _mwf_cov(mag, ph, span), span, reg)
    return mag, ph


RESAMPLE_MAX_KEPT_CHANNELS = 8     # avsep_resample_split / _join: up to 7.1


def _resample_table_check(what, filt, up, down, device):
    if up < 1 or down < 1:
        raise lib.AvsepError(f"{what}: up={up} down={down}")
    T = -(-(20 * max(up, down) + 1) // up)
    if filt.dtype != torch.float32 or tuple(filt.shape) != (T, up) or filt.device != device:
        raise lib.AvsepError(f"{what}: the table of {up}/{down} is float32 [{T},{up}] on {device}, got "
                             f"{filt.dtype} {tuple(filt.shape)} on {filt.device}")


SAMPLE_FORMATS = {"s16": (1, 2), "s24": (2, 3), "s32": (3, 4), "f32": (4, 4)}     # name -> (AVSEP_SAMPLE_* code, bytes a sample)
SAMPLE_OUT_FORMATS = ("s16", "s24", "f32")


def _sample_format(what, fmt, out=False):
    if fmt not in (SAMPLE_OUT_FORMATS if out else SAMPLE_FORMATS):
        raise lib.AvsepError(f"{what}: the {'output' if out else 'input'} sample format is one of "
                             f"{', '.join(SAMPLE_OUT_FORMATS if out else SAMPLE_FORMATS)}, got {fmt!r}")
    return SAMPLE_FORMATS[fmt]


def raw_frames(what, raw, C, nbytes):
    """The frame count of raw uint8 [L*C*nbytes] (a file's data chunk, from any byte address)."""
    if not torch.is_tensor(raw) or raw.dtype != torch.uint8 or raw.dim() != 1 or raw.numel() % (C * nbytes):
        raise lib.AvsepError(f"{what} takes raw frames as uint8 [L*{C}*{nbytes}], got {lib.got(raw)}")
    return raw.numel() // (C * nbytes)


def _raw_out(what, out, n, device):
    """The uint8 [n] a kernel writes file bytes into: ``out`` (a view at any byte address) or a new tensor."""
    if out is None:
        return torch.empty((n,), dtype=torch.uint8, device=device)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (n,) or not out.is_contiguous() or out.device != device:
        raise lib.AvsepError(f"{what}: out is contiguous uint8 [{n}] on {device}, got {lib.got(out)}")
    return out


def resample_poly(x, filt, up, down, in_ch=0, in_fmt="f32", out_fmt="f32", out=None):
    """Rational polyphase resampling (avsep_resample_poly, include/avsep.h); filt: the f32 polyphase table [T, up] of
    resample.filter_table on x's device.  in_ch = 0: x is f32 [B,L] (in_fmt 'f32'); in_ch = C >= 1: x is the raw frames of one
    recording, uint8 [L*C*bytes] of in_fmt at any byte address, down-mixed while they are staged.  -> [B, ceil(L*up/down)]
    samples of out_fmt: f32, int16, or for 's24' uint8 [B, Lout*3]; ``out`` (uint8 [B*Lout*bytes], any byte address) takes
    the bytes instead and is returned."""
    lib.require_gpu(x)
    lib.require_gpu(filt)
    up, down, in_ch = int(up), int(down), int(in_ch)
    icode, ibytes = _sample_format("resample_poly", in_fmt)
    ocode, obytes = _sample_format("resample_poly", out_fmt, out=True)
    if in_ch:
        if not 1 <= in_ch <= 256:
            raise lib.AvsepError(f"resample_poly down-mixes 1 to 256 channels, got {in_ch}")
        B, L = 1, raw_frames("resample_poly", x, in_ch, ibytes)
    else:
        if x.dtype != torch.float32 or x.dim() != 2 or in_fmt != "f32":
            raise lib.AvsepError(f"resample_poly: in_ch=0 takes float32 [B,L] with in_fmt 'f32', got {x.dtype} {tuple(x.shape)} "
                                 f"as {in_fmt!r}")
        B, L = x.shape
    _resample_table_check("resample_poly", filt, up, down, x.device)
    Lout = -(-L * up // down)
    if out is not None:
        y = _raw_out("resample_poly", out, B * Lout * obytes, x.device)
    elif out_fmt == "s24":
        y = torch.empty((B, Lout * 3), dtype=torch.uint8, device=x.device)
    else:
        y = torch.empty((B, Lout), dtype=torch.int16 if out_fmt == "s16" else torch.float32, device=x.device)
    x = x.contiguous()
    call("avsep_resample_poly", ptr(x), ptr(filt), B, L, up, down, in_ch, icode, ocode, ptr(y))
    return y


def resample_split(raw, filt, up, down, C, in_fmt):
    """avsep_resample_split (include/avsep.h): raw frames uint8 [L*C*bytes] of in_fmt at any byte address, 1 <= C <= 8
    -> f32 [1+C, ceil(L*up/down)]: row 0 the down-mix resample_poly(.., in_ch=C) gives, row 1+c channel c."""
    C = int(C)
    icode, ibytes = _sample_format("resample_split", in_fmt)
    if not 1 <= C <= RESAMPLE_MAX_KEPT_CHANNELS:
        raise lib.AvsepError(f"resample_split keeps 1 to {RESAMPLE_MAX_KEPT_CHANNELS} channels, got {C}")
    L = raw_frames("resample_split", raw, C, ibytes)
    lib.require_gpu(raw)
    lib.require_gpu(filt)
    up, down = int(up), int(down)
    _resample_table_check("resample_split", filt, up, down, raw.device)
    y = torch.empty((1 + C, -(-L * up // down)), dtype=torch.float32, device=raw.device)
    raw = raw.contiguous()
    call("avsep_resample_split", ptr(raw), ptr(filt), L, C, up, down, icode, ptr(y))
    return y


def resample_join(x, filt, up, down, out_fmt, out=None):
    """avsep_resample_join (include/avsep.h): f32 [C,L], 1 <= C <= 8 -> uint8 [ceil(L*up/down)*C*bytes], interleaved
    frames of out_fmt ('s16' | 's24' | 'f32') as they lie in a file; ``out``: a uint8 view of that size at any byte address."""
    ocode, obytes = _sample_format("resample_join", out_fmt, out=True)
    if x.dtype != torch.float32 or x.dim() != 2 or not 1 <= x.shape[0] <= RESAMPLE_MAX_KEPT_CHANNELS:
        raise lib.AvsepError(f"resample_join takes float32 [C,L] with 1 <= C <= {RESAMPLE_MAX_KEPT_CHANNELS}, got "
                             f"{x.dtype} {tuple(x.shape)}")
    lib.require_gpu(x)
    lib.require_gpu(filt)
    up, down = int(up), int(down)
    _resample_table_check("resample_join", filt, up, down, x.device)
    Cc, L = x.shape
    y = _raw_out("resample_join", out, -(-L * up // down) * Cc * obytes, x.device)
    x = x.contiguous()
    call("avsep_resample_join", ptr(x), ptr(filt), Cc, L, up, down, ocode, ptr(y))
    return y


BAND_MAX_SOURCES = 8              # avsep_band_gains / avsep_band_extend: N and G up to 8
BAND_MAX_ROWS = 8
BAND_MAX_HOP = 4096


def band_gains(stem_mag, mix_mag, lo_bin=None):
    """avsep_band_gains (include/avsep.h): stem_mag f32 [N,G,bins,F], mix_mag f32 [G,bins,F] -> f32 [N,G,F], per frame the share
    of the mixture's RMS amplitude every source holds over the bins [lo_bin, bins), at most 1; ``lo_bin`` defaults to
    bins // 2 (the top octave).  A frame that is silent in the band gives exactly 0."""
    if not torch.is_tensor(stem_mag) or not torch.is_tensor(mix_mag) or stem_mag.dtype != torch.float32 or stem_mag.dim() != 4 \
            or mix_mag.dtype != torch.float32 or tuple(mix_mag.shape) != tuple(stem_mag.shape[1:]) or mix_mag.device != stem_mag.device:
        raise lib.AvsepError(f"band_gains takes stem_mag float32 [N,G,bins,F] and mix_mag float32 [G,bins,F] on one device, got "
                             f"{lib.got(stem_mag)} and {lib.got(mix_mag)}")
    lib.require_gpu(stem_mag)
    N, G, bins, F = stem_mag.shape
    if not (1 <= N <= BAND_MAX_SOURCES and 1 <= G <= BAND_MAX_ROWS and F >= 1):
        raise lib.AvsepError(f"band_gains: 1 <= N <= {BAND_MAX_SOURCES}, 1 <= G <= {BAND_MAX_ROWS}, F >= 1; got {tuple(stem_mag.shape)}")
    if lo_bin is None:
        lo_bin = bins // 2
    if isinstance(lo_bin, bool) or not isinstance(lo_bin, int) or not 1 <= lo_bin < bins:
        raise lib.AvsepError(f"band_gains takes lo_bin as an int with 1 <= lo_bin < bins = {bins}, got {lo_bin!r}")
    gains = _f32((N, G, F), stem_mag)
    stem_mag, mix_mag = stem_mag.contiguous(), mix_mag.contiguous()
    call("avsep_band_gains", ptr(stem_mag), ptr(mix_mag), N, G, bins, F, lo_bin, ptr(gains))
    return gains


def band_extend(stems, low, file, gains, filt, up, down, hop):
    """avsep_band_extend (include/avsep.h): stems f32 [N,G,Lm] at the model's rate, low f32 [G,Ll] (Ll >= Lm) the model-rate
    mixture rows they were made from, file f32 [G,Lf] the same rows at the file's rate, gains f32 [N,G,F] (band_gains), filt
    the polyphase table of up/down > 1, hop the STFT hop of the gains' frames -> f32 [N,G,ceil(Lm*up/down)]:
    resample(stems) + gain * (file - resample(low)), the gain interpolated between the frames next to each output."""
    for name, t, nd in (("stems", stems, 3), ("low", low, 2), ("file", file, 2), ("gains", gains, 3)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != nd:
            raise lib.AvsepError(f"band_extend takes {name} as float32 with {nd} dimensions (stems [N,G,Lm], low [G,Ll], file [G,Lf], "
                                 f"gains [N,G,F]), got {lib.got(t)}")
    lib.require_gpu(stems)
    lib.require_gpu(filt)
    N, G, Lm = stems.shape
    if not (1 <= N <= BAND_MAX_SOURCES and 1 <= G <= BAND_MAX_ROWS and Lm >= 1):
        raise lib.AvsepError(f"band_extend: 1 <= N <= {BAND_MAX_SOURCES}, 1 <= G <= {BAND_MAX_ROWS}, Lm >= 1; got stems {tuple(stems.shape)}")
    for name, t in (("low", low), ("file", file), ("gains", gains)):
        if t.device != stems.device:
            raise lib.AvsepError(f"band_extend takes {name} on {stems.device}, the stems' device, got {t.device}")
    if low.shape[0] != G or low.shape[1] < Lm:
        raise lib.AvsepError(f"band_extend takes low as [{G},Ll] with Ll >= Lm = {Lm}, got {tuple(low.shape)}")
    if file.shape[0] != G or file.shape[1] < 1:
        raise lib.AvsepError(f"band_extend takes file as [{G},Lf] with Lf >= 1, got {tuple(file.shape)}")
    if tuple(gains.shape[:2]) != (N, G) or gains.shape[2] < 1:
        raise lib.AvsepError(f"band_extend takes gains as [{N},{G},F] with F >= 1, got {tuple(gains.shape)}")
    for name, v in (("up", up), ("down", down), ("hop", hop)):
        if isinstance(v, bool) or int(v) != v:
            raise lib.AvsepError(f"band_extend takes {name} as an int, got {v!r}")
    up, down, hop = int(up), int(down), int(hop)
    if not 1 <= down < up <= 1280:
        raise lib.AvsepError(f"band_extend extends upwards: 1 <= down < up <= 1280, got up={up} down={down}")
    if not 1 <= hop <= BAND_MAX_HOP:
        raise lib.AvsepError(f"band_extend takes 1 <= hop <= {BAND_MAX_HOP}, got {hop}")
    _resample_table_check("band_extend", filt, up, down, stems.device)
    Lout = -(-Lm * up // down)
    if Lout >= 2 ** 31:
        raise lib.AvsepError(f"band_extend: ceil(Lm*{up}/{down}) < 2^31, got Lm={Lm}")
    out = _f32((N, G, Lout), stems)
    stems, low, file, gains = stems.contiguous(), low.contiguous(), file.contiguous(), gains.contiguous()
    call("avsep_band_extend", ptr(stems), ptr(low), ptr(file), ptr(gains), ptr(filt), N, G, Lm, low.shape[1], file.shape[1],
         gains.shape[2], hop, up, down, ptr(out))
    return out


TRUE_PEAK_TAPS = 21               # rows of avsep_true_peak's polyphase table


def _level_rows(what, x):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or not 1 <= x.shape[0] <= 65535 or x.shape[1] < 1:
        raise lib.AvsepError(f"{what} takes float32 rows [R,L] with 1 <= R <= 65535 and L >= 1, got {lib.got(x)}")
    return x.shape


def loudness_energies(x, sos, h):
    """avsep_loudness_energies (include/avsep.h): x f32 [R,L] on the GPU, sos float64 [2,6] on the host (two biquads
    b0 b1 b2 1 a1 a2), h the sub-block length -> f64 [R, L // h] on the GPU: the energy of the filtered row per sub-block."""
    R, L = _level_rows("loudness_energies", x)
    sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64))
    if sos.shape != (2, 6) or not np.isfinite(sos).all() or (sos[:, 3] != 1.0).any():
        raise lib.AvsepError(f"loudness_energies takes sos as float64 [2,6], finite, with a0 = 1; got shape {sos.shape}")
    if isinstance(h, bool) or int(h) != h or not 1 <= h <= L or L >= 2 ** 31:
        raise lib.AvsepError(f"loudness_energies takes 1 <= h <= L < 2^31, got h={h!r} L={L}")
    h = int(h)
    lib.require_gpu(x)
    x = x.contiguous()
    nbytes = lib.load().avsep_loudness_energies_workspace_bytes(R, L, h)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    E = torch.empty((R, L // h), dtype=torch.float64, device=x.device)
    call("avsep_loudness_energies", ptr(x), sos.ctypes.data, R, L, h, ptr(E), ptr(ws), nbytes)
    return E


def true_peak(x, taps, os):
    """avsep_true_peak (include/avsep.h): x f32 [R,L], taps f64 [21, os] on x's device (the polyphase table of the
    interpolation filter), os 1 | 2 | 4 -> f64 [R,2] on the GPU: (sample peak, true peak) per row, +inf for a row that holds
    a NaN or an infinity."""
    R, L = _level_rows("true_peak", x)
    if isinstance(os, bool) or os not in (1, 2, 4) or os * L >= 2 ** 31:
        raise lib.AvsepError(f"true_peak oversamples by 1, 2 or 4 with os * L < 2^31, got os={os!r} L={L}")
    if not torch.is_tensor(taps) or taps.dtype != torch.float64 or tuple(taps.shape) != (TRUE_PEAK_TAPS, os) or taps.device != x.device:
        raise lib.AvsepError(f"true_peak: the table of os={os} is float64 [{TRUE_PEAK_TAPS},{os}] on {x.device}, got {lib.got(taps)}")
    lib.require_gpu(x)
    x, taps = x.contiguous(), taps.contiguous()
    nbytes = lib.load().avsep_true_peak_workspace_bytes(R, L)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    peaks = torch.empty((R, 2), dtype=torch.float64, device=x.device)
    call("avsep_true_peak", ptr(x), ptr(taps), R, L, int(os), ptr(peaks), ptr(ws), nbytes)
    return peaks


LIMITER_MAX_A = 2048              # the longest half-width avsep_limiter takes, samples
LIMITER_MAX_C = 64                # rows of a programme


def limiter(x, taps, w, os, pre_gain, ceiling, return_gain=False, out=None):
    """avsep_limiter (include/avsep.h): x f32 [P,C,L], P programmes of C linked rows; taps f64 [21, os] and w f64 [2A+1]
    (the smoothing weights, symmetric, sum 1) on x's device; pre_gain > 0, 0 < ceiling <= 1 (linear) -> (y f32 [P,C,L],
    gain f64 [P,L] or None, stats f64 [P,3] on the GPU: the largest detector value, the smallest gain, the count of gains
    below 1).  out: where y goes (x itself is allowed)."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 3 or not 1 <= x.shape[0] <= 65535 or \
            not 1 <= x.shape[1] <= LIMITER_MAX_C or x.shape[2] < 1:
        raise lib.AvsepError(f"limiter takes float32 [P,C,L] with 1 <= P <= 65535, 1 <= C <= {LIMITER_MAX_C} and L >= 1, got {lib.got(x)}")
    P, C, L = x.shape
    if isinstance(os, bool) or os not in (1, 2, 4) or os * L >= 2 ** 31:
        raise lib.AvsepError(f"limiter oversamples by 1, 2 or 4 with os * L < 2^31, got os={os!r} L={L}")
    if not torch.is_tensor(taps) or taps.dtype != torch.float64 or tuple(taps.shape) != (TRUE_PEAK_TAPS, os) or taps.device != x.device:
        raise lib.AvsepError(f"limiter: the table of os={os} is float64 [{TRUE_PEAK_TAPS},{os}] on {x.device}, got {lib.got(taps)}")
    if not torch.is_tensor(w) or w.dtype != torch.float64 or w.dim() != 1 or w.shape[0] % 2 != 1 or \
            not 3 <= w.shape[0] <= 2 * LIMITER_MAX_A + 1 or w.device != x.device:
        raise lib.AvsepError(f"limiter: the weights are float64 [2A+1] with 1 <= A <= {LIMITER_MAX_A} on {x.device}, got {lib.got(w)}")
    pre_gain, ceiling = float(pre_gain), float(ceiling)
    if not (np.isfinite(pre_gain) and pre_gain > 0.0 and 0.0 < ceiling <= 1.0):
        raise lib.AvsepError(f"limiter takes a finite pre_gain > 0 and 0 < ceiling <= 1, got pre_gain={pre_gain} ceiling={ceiling}")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device
                            or not out.is_contiguous()):
        raise lib.AvsepError(f"limiter: out is dense float32 {tuple(x.shape)} on {x.device}, got {lib.got(out)}")
    lib.require_gpu(x)
    x, taps, w = x.contiguous(), taps.contiguous(), w.contiguous()
    y = torch.empty_like(x) if out is None else out
    gain = torch.empty((P, L), dtype=torch.float64, device=x.device) if return_gain else None
    stats = torch.empty((P, 3), dtype=torch.float64, device=x.device)
    nbytes = lib.load().avsep_limiter_workspace_bytes(P, C, L)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    call("avsep_limiter", ptr(x), ptr(taps), ptr(w), P, C, L, int(os), w.shape[0] // 2, pre_gain, ceiling, ptr(y), ptr(gain),
         ptr(stats), ptr(ws), nbytes)
    return y, gain, stats


FRAMES_MAX_T = 65535              # frames per launch of avsep_frames_prepare (a grid dimension)


def frames_prepare(frames, tables, size, S, crop, flip, return_u8=False):
    """avsep_frames_prepare (include/avsep.h): frames uint8 [T,H,W,3] on the GPU, as frames.check_stack passes them (frames.prepare
    is the caller and checks there); tables = (hcoef int32 [w,kh], hbound int32
    [w,2], vcoef int32 [h,kv], vbound int32 [h,2], lut f32 [256,3]) on the frames' device (frames.Plan.on); size (w, h), crop
    (i, j), flip -> f32 [T,3,S,S]; with return_u8 also the cropped pixels uint8 [T,S,S,3].  Stacks of more than 65535 frames
    are cut into several launches."""
    lib.require_gpu(frames)
    T, H, W, _ = frames.shape
    hcoef, hbound, vcoef, vbound, lut = tables
    (w, h), S = size, int(S)
    want = ((hcoef, torch.int32, (w, hcoef.shape[-1])), (hbound, torch.int32, (w, 2)), (vcoef, torch.int32, (h, vcoef.shape[-1])),
            (vbound, torch.int32, (h, 2)), (lut, torch.float32, (256, 3)))
    for t, dtype, shape in want:
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != frames.device or not t.is_contiguous():
            raise lib.AvsepError(f"frames_prepare: a table must be {dtype} {shape} on {frames.device}, got {lib.got(t)}")
    out = _f32((T, 3, S, S), frames)
    u8 = torch.empty((T, S, S, 3), dtype=torch.uint8, device=frames.device) if return_u8 else None
    for a in range(0, T, FRAMES_MAX_T):
        n = min(FRAMES_MAX_T, T - a)
        call("avsep_frames_prepare", ptr(frames[a:a + n]), n, H, W, ptr(hcoef), ptr(hbound), w, hcoef.shape[1], ptr(vcoef), ptr(vbound),
             h, vcoef.shape[1], S, int(crop[0]), int(crop[1]), int(bool(flip)), ptr(lut), ptr(out[a:a + n]),
             ptr(u8[a:a + n]) if return_u8 else None)
    return (out, u8) if return_u8 else out


def frames_batch_plan(rows, S, pixel_bytes, table_words, out_floats, plane):
    """avsep_frames_batch_plan (include/avsep.h; host only, no GPU): rows = a NumPy array of dtype np.dtype(lib.FramesRow),
    at most 65535 of them -> (grid y, LDS bytes, smallest tile height); the rows' launch sizing is filled in in place.
    AvsepError for anything the library refuses."""
    launch = (C.c_int32 * 3)()
    rc = lib.load().avsep_frames_batch_plan(rows.ctypes.data_as(C.POINTER(lib.FramesRow)), len(rows), int(S), int(pixel_bytes),
                                            int(table_words), int(out_floats), int(plane), launch)
    if rc != 0:
        raise lib.AvsepError(f"avsep_frames_batch_plan refused {len(rows)} frames at S = {S}: a size, crop, tap count or a pixel, "
                             f"table or output range outside its buffer ({rc})")
    return tuple(launch)


def frames_prepare_batch(pixels, rows, tables, lut, S, out, plane, grid_y, lds_bytes):
    """avsep_frames_prepare_batch (include/avsep.h): pixels uint8 [bytes], rows uint8 [n * sizeof(avsep_frames_row)] (the planned
    rows), tables int32 [words], lut f32 [256,3] and out f32, all on one GPU; one launch for n <= 65535 frames."""
    lib.require_gpu(pixels)
    n = rows.numel() // C.sizeof(lib.FramesRow)
    for t, dtype in ((pixels, torch.uint8), (rows, torch.uint8), (tables, torch.int32), (lut, torch.float32), (out, torch.float32)):
        if t.dtype != dtype or t.device != pixels.device or not t.is_contiguous():
            raise lib.AvsepError(f"frames_prepare_batch: a buffer must be {dtype}, contiguous, on {pixels.device}, got {lib.got(t)}")
    if rows.numel() != n * C.sizeof(lib.FramesRow) or tuple(lut.shape) != (256, 3):
        raise lib.AvsepError(f"frames_prepare_batch: {rows.numel()} bytes of rows, look-up table {tuple(lut.shape)}")
    call("avsep_frames_prepare_batch", ptr(pixels), pixels.numel(), ptr(rows), n, ptr(tables), tables.numel(), int(S), ptr(lut),
         ptr(out), out.numel(), int(plane), int(grid_y), int(lds_bytes))
    return out


def jpeg_plan_check(images, segments, nbytes, table_words, pixel_bytes, ws_blocks):
    """avsep_jpeg_plan_check (include/avsep.h; host only, no GPU): images and segments = NumPy arrays of dtype
    np.dtype(lib.JpegImage) and np.dtype(lib.JpegSegment), the rows of one chunk.  AvsepError for anything the library refuses."""
    images, segments = np.ascontiguousarray(images), np.ascontiguousarray(segments)
    rc = lib.load().avsep_jpeg_plan_check(images.ctypes.data, len(images), segments.ctypes.data, len(segments), int(nbytes),
                                          int(table_words), int(pixel_bytes), int(ws_blocks))
    if rc != 0:
        raise lib.AvsepError(f"avsep_jpeg_plan_check refused {len(images)} images in {len(segments)} segments: a size, sampling "
                             f"form or MCU count outside the limits, or a byte, block, table or pixel range outside its buffer ({rc})")


def _jpeg_buffers(who, first, typed):
    lib.require_gpu(first)
    for t, dtype in typed:
        if not torch.is_tensor(t) or t.dtype != dtype or t.device != first.device or not t.is_contiguous() or t.dim() != 1:
            raise lib.AvsepError(f"{who}: a buffer must be {dtype} [n], contiguous, on {first.device}, got {lib.got(t)}")


def _jpeg_rows(who, images, sized, row=lib.JpegImage):
    """The row count of `images` (uint8 rows of `row`); sized: (tensor, name, least elements)."""
    n = images.numel() // C.sizeof(row)
    if n < 1 or images.numel() != n * C.sizeof(row):
        raise lib.AvsepError(f"{who}: {images.numel()} bytes of rows of {C.sizeof(row)}")
    for t, name, least in sized:
        if t.numel() < least:
            raise lib.AvsepError(f"{who}: {name} has {t.numel()} elements, {least} are needed")
    return n


def jpeg_entropy(data, images, segments, tables, coef, ws_blocks, status):
    """avsep_jpeg_entropy (include/avsep.h): data uint8 [bytes], images / segments uint8 (the checked rows of one chunk), tables
    int32 [words], coef int16 [>= 64 * ws_blocks], status int32 [images] (zeroed), all on one GPU.  coef[:64 * ws_blocks] is
    zeroed and filled; a lane that stops sets its image's status word."""
    _jpeg_buffers("jpeg_entropy", data, ((data, torch.uint8), (images, torch.uint8), (segments, torch.uint8), (tables, torch.int32),
                                         (coef, torch.int16), (status, torch.int32)))
    n = _jpeg_rows("jpeg_entropy", images, ((coef, "coef", 64 * int(ws_blocks)),))
    ns = _jpeg_rows("jpeg_entropy", segments, (), lib.JpegSegment)
    if status.numel() != n:
        raise lib.AvsepError(f"jpeg_entropy: {status.numel()} status words for {n} images")
    call("avsep_jpeg_entropy", ptr(data), data.numel(), ptr(images), n, ptr(segments), ns, ptr(tables), tables.numel(), ptr(coef),
         int(ws_blocks), ptr(status))


def jpeg_pixels(coef, planes, ws_blocks, images, max_blocks, max_pixels, tables, status, pixels):
    """avsep_jpeg_pixels (include/avsep.h): the coefficients of one chunk -> planes uint8 [>= 64 * ws_blocks] -> the chunk's
    frames in pixels uint8 [bytes]; images whose status word is set are skipped."""
    _jpeg_buffers("jpeg_pixels", coef, ((coef, torch.int16), (planes, torch.uint8), (images, torch.uint8), (tables, torch.int32),
                                        (status, torch.int32), (pixels, torch.uint8)))
    n = _jpeg_rows("jpeg_pixels", images, ((coef, "coef", 64 * int(ws_blocks)), (planes, "planes", 64 * int(ws_blocks))))
    if status.numel() != n:
        raise lib.AvsepError(f"jpeg_pixels: {status.numel()} status words for {n} images")
    call("avsep_jpeg_pixels", ptr(coef), ptr(planes), int(ws_blocks), ptr(images), n, int(max_blocks), int(max_pixels), ptr(tables),
         tables.numel(), ptr(status), ptr(pixels), pixels.numel())


def jpeg_scan_check(images, scans, nbytes, table_words, pixel_bytes, ws_blocks):
    """avsep_jpeg_scan_check (include/avsep.h; host only, no GPU): images and scans = NumPy arrays of dtype np.dtype(lib.JpegImage)
    and np.dtype(lib.JpegScan), the rows of one chunk.  AvsepError for anything the library refuses."""
    images, scans = np.ascontiguousarray(images), np.ascontiguousarray(scans)
    rc = lib.load().avsep_jpeg_scan_check(images.ctypes.data, len(images), scans.ctypes.data, len(scans), int(nbytes),
                                          int(table_words), int(pixel_bytes), int(ws_blocks))
    if rc != 0:
        raise lib.AvsepError(f"avsep_jpeg_scan_check refused {len(images)} images in {len(scans)} scan rows: a band, bit position, "
                             f"component mask or level outside the rules, or a byte, unit, table or pixel range outside its buffer ({rc})")


def jpeg_scans(data, images, scans, level, zero, tables, coef, ws_blocks, status):
    """avsep_jpeg_scans (include/avsep.h): the scan rows (uint8, checked) of ONE level of a chunk's progressive images, one lane
    each, into coef int16 [>= 64 * ws_blocks]; zero: zero coef[:64 * ws_blocks] first.  The other buffers as jpeg_entropy's."""
    _jpeg_buffers("jpeg_scans", data, ((data, torch.uint8), (images, torch.uint8), (scans, torch.uint8), (tables, torch.int32),
                                       (coef, torch.int16), (status, torch.int32)))
    n = _jpeg_rows("jpeg_scans", images, ((coef, "coef", 64 * int(ws_blocks)),))
    ns = _jpeg_rows("jpeg_scans", scans, (), lib.JpegScan)
    if status.numel() != n:
        raise lib.AvsepError(f"jpeg_scans: {status.numel()} status words for {n} images")
    call("avsep_jpeg_scans", ptr(data), data.numel(), ptr(images), n, ptr(scans), ns, int(level), int(bool(zero)), ptr(tables),
         tables.numel(), ptr(coef), int(ws_blocks), ptr(status))


def jpeg_coef_bound(coef, ws_blocks, images, max_blocks, tables, status):
    """avsep_jpeg_coef_bound (include/avsep.h): the finished coefficients of one chunk against AVSEP_JPEG_MAX_COEF; an image
    with one beyond it gets status bit 128."""
    _jpeg_buffers("jpeg_coef_bound", coef, ((coef, torch.int16), (images, torch.uint8), (tables, torch.int32), (status, torch.int32)))
    n = _jpeg_rows("jpeg_coef_bound", images, ((coef, "coef", 64 * int(ws_blocks)),))
    if status.numel() != n:
        raise lib.AvsepError(f"jpeg_coef_bound: {status.numel()} status words for {n} images")
    call("avsep_jpeg_coef_bound", ptr(coef), int(ws_blocks), ptr(images), n, int(max_blocks), ptr(tables), tables.numel(), ptr(status))


def jpeg_enc_plan_check(images, pixel_bytes, table_words, ws_blocks, n_intervals):
    """avsep_jpeg_enc_plan_check (include/avsep.h; host only, no GPU): images = a NumPy array of dtype np.dtype(lib.JpegImage),
    the rows of one chunk.  AvsepError for anything the library refuses."""
    images = np.ascontiguousarray(images)
    rc = lib.load().avsep_jpeg_enc_plan_check(images.ctypes.data, len(images), int(pixel_bytes), int(table_words), int(ws_blocks),
                                              int(n_intervals))
    if rc != 0:
        raise lib.AvsepError(f"avsep_jpeg_enc_plan_check refused {len(images)} images: a size, sampling form, MCU count or restart "
                             f"interval outside the limits, blocks or intervals that do not run on, or a pixel or table range outside "
                             f"its buffer ({rc})")


def jpeg_enc_coef(pixels, images, tables, coef, ws_blocks):
    """avsep_jpeg_enc_coef (include/avsep.h): pixels uint8 [bytes], images uint8 (the checked rows of one chunk), tables int32
    [words] -> coef int16 [>= 64 * ws_blocks]: every block of the chunk, scan order, zig-zag inside."""
    _jpeg_buffers("jpeg_enc_coef", pixels, ((pixels, torch.uint8), (images, torch.uint8), (tables, torch.int32), (coef, torch.int16)))
    n = _jpeg_rows("jpeg_enc_coef", images, ((coef, "coef", 64 * int(ws_blocks)),))
    call("avsep_jpeg_enc_coef", ptr(pixels), pixels.numel(), ptr(images), n, ptr(tables), tables.numel(), ptr(coef), int(ws_blocks))


def jpeg_enc_count(coef, ws_blocks, images, n_intervals, tables, bits, pos, ivl_bytes, ivl_off, tiles):
    """avsep_jpeg_enc_count: coef -> bits int32 [ws_blocks], pos int64 [ws_blocks + 1], ivl_bytes int32 [n_intervals], ivl_off
    int64 [n_intervals + 1]; tiles int64: scratch."""
    _jpeg_buffers("jpeg_enc_count", coef, ((coef, torch.int16), (images, torch.uint8), (tables, torch.int32), (bits, torch.int32),
                                           (pos, torch.int64), (ivl_bytes, torch.int32), (ivl_off, torch.int64), (tiles, torch.int64)))
    B, I = int(ws_blocks), int(n_intervals)
    n = _jpeg_rows("jpeg_enc_count", images, ((coef, "coef", 64 * B), (bits, "bits", B), (pos, "pos", B + 1),
                                              (ivl_bytes, "ivl_bytes", I), (ivl_off, "ivl_off", I + 1)))
    call("avsep_jpeg_enc_count", ptr(coef), B, ptr(images), n, I, ptr(tables), tables.numel(), ptr(bits), ptr(pos), ptr(ivl_bytes),
         ptr(ivl_off), ptr(tiles), tiles.numel())


def jpeg_enc_pack(coef, ws_blocks, images, n_intervals, tables, pos, ivl_off, stream_buf, groups, ffpos, ff0, ivl_out, out_off, tiles):
    """avsep_jpeg_enc_pack: the blocks' bits -> stream_buf uint8 [a multiple of 4: the unstuffed stream], then the 0xFF counts:
    groups int32 [ceil(bytes / 64)], ffpos int64 [groups + 1], ff0 int64 [n_intervals], ivl_out int32 [n_intervals], out_off int64
    [n_intervals + 1]."""
    _jpeg_buffers("jpeg_enc_pack", coef, ((coef, torch.int16), (images, torch.uint8), (tables, torch.int32), (pos, torch.int64),
                                          (ivl_off, torch.int64), (stream_buf, torch.uint8), (groups, torch.int32), (ffpos, torch.int64),
                                          (ff0, torch.int64), (ivl_out, torch.int32), (out_off, torch.int64), (tiles, torch.int64)))
    B, I, G = int(ws_blocks), int(n_intervals), -(-stream_buf.numel() // 64)
    n = _jpeg_rows("jpeg_enc_pack", images, ((coef, "coef", 64 * B), (pos, "pos", B + 1), (ivl_off, "ivl_off", I + 1),
                                             (groups, "groups", G), (ffpos, "ffpos", G + 1), (ff0, "ff0", I), (ivl_out, "ivl_out", I),
                                             (out_off, "out_off", I + 1)))
    call("avsep_jpeg_enc_pack", ptr(coef), B, ptr(images), n, I, ptr(tables), tables.numel(), ptr(pos), ptr(ivl_off), ptr(stream_buf),
         stream_buf.numel(), ptr(groups), ptr(ffpos), ptr(ff0), ptr(ivl_out), ptr(out_off), ptr(tiles), tiles.numel())


def jpeg_enc_stuff(stream_buf, images, n_intervals, ivl_off, ffpos, ff0, out_off, out, sizes):
    """avsep_jpeg_enc_stuff: the unstuffed stream -> out uint8 [bytes]: per image its stuffed intervals, RSTn between them, EOI
    at the end; sizes int64 [2 * images] = (first byte, bytes) of every image in out."""
    _jpeg_buffers("jpeg_enc_stuff", stream_buf, ((stream_buf, torch.uint8), (images, torch.uint8), (ivl_off, torch.int64),
                                                 (ffpos, torch.int64), (ff0, torch.int64), (out_off, torch.int64), (out, torch.uint8),
                                                 (sizes, torch.int64)))
    I, G = int(n_intervals), -(-stream_buf.numel() // 64)
    n = _jpeg_rows("jpeg_enc_stuff", images, ((ivl_off, "ivl_off", I + 1), (ffpos, "ffpos", G + 1), (ff0, "ff0", I),
                                              (out_off, "out_off", I + 1), (out, "out", 1)))
    if sizes.numel() != 2 * n:
        raise lib.AvsepError(f"jpeg_enc_stuff: {sizes.numel()} size words for {n} images")
    call("avsep_jpeg_enc_stuff", ptr(stream_buf), stream_buf.numel(), ptr(images), n, I, ptr(ivl_off), ptr(ffpos), ptr(ff0), ptr(out_off),
         ptr(out), out.numel(), ptr(sizes))


def png_plan_check(images, nbytes, table_bytes, pixel_bytes, ws_bytes):
    """avsep_png_plan_check (include/avsep.h; host only, no GPU): images = a NumPy array of dtype np.dtype(lib.PngImage), the
    rows of one chunk.  AvsepError for anything the library refuses."""
    images = np.ascontiguousarray(images)
    rc = lib.load().avsep_png_plan_check(images.ctypes.data, len(images), int(nbytes), int(table_bytes), int(pixel_bytes), int(ws_bytes))
    if rc != 0:
        raise lib.AvsepError(f"avsep_png_plan_check refused {len(images)} images: a size, colour type or channel count outside the "
                             f"limits, or a stream, scanline, palette or pixel range outside its buffer ({rc})")


def png_inflate(data, images, ws, ws_bytes, status):
    """avsep_png_inflate (include/avsep.h): data uint8 [bytes], images uint8 (the checked rows of one chunk), ws uint8
    [>= ws_bytes], status int32 [images] (zeroed), all on one GPU.  Every image's zlib stream is inflated into its scanlines in
    ws; a lane that stops sets its image's status word."""
    _jpeg_buffers("png_inflate", data, ((data, torch.uint8), (images, torch.uint8), (ws, torch.uint8), (status, torch.int32)))
    n = _jpeg_rows("png_inflate", images, ((ws, "ws", int(ws_bytes)),), lib.PngImage)
    if status.numel() != n:
        raise lib.AvsepError(f"png_inflate: {status.numel()} status words for {n} images")
    call("avsep_png_inflate", ptr(data), data.numel(), ptr(images), n, ptr(ws), int(ws_bytes), ptr(status))


def png_pixels(ws, ws_bytes, images, max_pixels, tables, status, pixels, stages=3):
    """avsep_png_pixels (include/avsep.h): the scanlines of one chunk are unfiltered in place and turned into the chunk's frames
    in pixels uint8 [bytes]; tables uint8 [bytes] holds the palettes; images whose status word is set are skipped.  stages: 1 =
    unfilter only, 2 = colour only, 3 = both."""
    _jpeg_buffers("png_pixels", ws, ((ws, torch.uint8), (images, torch.uint8), (tables, torch.uint8), (status, torch.int32),
                                     (pixels, torch.uint8)))
    n = _jpeg_rows("png_pixels", images, ((ws, "ws", int(ws_bytes)),), lib.PngImage)
    if status.numel() != n:
        raise lib.AvsepError(f"png_pixels: {status.numel()} status words for {n} images")
    call("avsep_png_pixels", ptr(ws), int(ws_bytes), ptr(images), n, int(max_pixels), ptr(tables), tables.numel(), ptr(status),
         ptr(pixels), pixels.numel(), int(stages))


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[ptr(t) for t in tensors])


def localise_maps(x, win, vs, att):
    """x [K,D,Fq,Tq] bottleneck of K windows, win int32 [T] on the device, vs: C tensors [T,Dc,h,w] (duet: the same tensor
    twice), att 'cos' | 'sig' -> maps [T,C,h,w], best int32 [T], scores [T,C!]: the CoLoc maps of every frame in one launch."""
    lib.require_gpu(x)
    Kw, D = x.shape[:2]
    T, Dc, h, w = vs[0].shape
    Cn = len(vs)
    if any(tuple(v.shape) != (T, Dc, h, w) for v in vs) or Cn not in (2, 3) or Dc != D // Cn or win.numel() != T:
        raise lib.AvsepError(f"localise_maps: {Cn} visual inputs {[tuple(v.shape) for v in vs]} against a bottleneck of {D} "
                             f"channels and {win.numel()} window indices")
    maps = _f32((T, Cn, h, w), x)
    best = torch.empty((T,), dtype=torch.int32, device=x.device)
    scores = _f32((T, 2 if Cn == 2 else 6), x)
    call("avsep_localise_maps", ptr(x), ptr(win), _ptr_array(vs), T, Kw, Cn, D, x.shape[2] * x.shape[3], h * w,
         lib.ATT_BY_NAME[att], ptr(maps), ptr(best), ptr(scores))
    return maps, best, scores


def heatmap_overlay(maps, frames, table, alpha256):
    """maps [T,C,h,w] fp32, frames: C tensors [T,3,H,W] fp32 normalised (duet: the same tensor), table uint8 [256,3] on the
    device, alpha256 in [0,256] -> uint8 [C,T,H,W,3] RGB: colour-mapped, resized, blended over the frames in one launch."""
    lib.require_gpu(maps)
    T, Cn, h, w = maps.shape
    H, W = frames[0].shape[-2:]
    if len(frames) != Cn or any(tuple(f.shape) != (T, 3, H, W) or f.dtype != torch.float32 for f in frames) \
            or tuple(table.shape) != (256, 3) or table.dtype != torch.uint8:
        raise lib.AvsepError(f"heatmap_overlay: maps {tuple(maps.shape)} need {Cn} float32 frame tensors [{T},3,H,W] and a uint8 "
                             f"[256,3] table, got {[tuple(f.shape) for f in frames]} and {tuple(table.shape)}")
    out = torch.empty((Cn, T, H, W, 3), dtype=torch.uint8, device=maps.device)
    call("avsep_heatmap_overlay", ptr(maps), _ptr_array(frames), ptr(table), T, Cn, h, w, H, W, int(alpha256), ptr(out))
    return out


SPEC_REDUCE = {"max": 0, "mean": 1}


def spec_image(mag, mask=None, thres=None, cell=1, reduce="max", log=True, scale=200.0, table=None, out=None):
    """mag [R,F,T] fp32 (mask: the same shape, or None) -> uint8 [R,F,W,3] with a uint8 [256,3] RGB ``table`` on the device,
    [R,F,W,1] (the level itself) without; W = ceil(T / cell).  One launch (``avsep_spec_image``, include/avsep.h): per pixel
    the max / mean over a cell of mag * m, m = 1 | mask > thres | mask, then log10(c + 1) * scale or c * scale, saturated at
    255 and truncated; image row 0 is the highest frequency row.  out: a dense uint8 tensor of that shape to write into."""
    if not torch.is_tensor(mag) or mag.dim() != 3 or mag.dtype != torch.float32 or mag.numel() == 0:
        raise lib.AvsepError(f"spec_image takes a float32 magnitude [R,F,T], got {lib.got(mag)}")
    if mask is not None and (not torch.is_tensor(mask) or mask.shape != mag.shape or mask.dtype != torch.float32
                             or mask.device != mag.device):
        raise lib.AvsepError(f"spec_image: the mask must be float32 {tuple(mag.shape)} beside the magnitude, got {lib.got(mask)}")
    if thres is not None and (mask is None or thres != thres):
        raise lib.AvsepError("spec_image: a threshold is a number and needs a mask (None: the mask value itself)")
    if isinstance(cell, bool) or not isinstance(cell, int) or cell < 1:
        raise lib.AvsepError(f"spec_image: cell is a whole number of frames >= 1, got {cell!r}")
    if reduce not in SPEC_REDUCE:
        raise lib.AvsepError(f"spec_image: reduce is 'max' or 'mean', got {reduce!r}")
    if not float(scale) == float(scale):
        raise lib.AvsepError("spec_image: scale is a number")
    if table is not None and (not torch.is_tensor(table) or tuple(table.shape) != (256, 3) or table.dtype != torch.uint8
                              or table.device != mag.device):
        raise lib.AvsepError(f"spec_image: the colour table is uint8 [256,3] beside the magnitude, got {lib.got(table)}")
    R, F, T = mag.shape
    shape = (R, F, -(-T // cell), 3 if table is not None else 1)
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.uint8
                            or out.device != mag.device or not out.is_contiguous()):
        raise lib.AvsepError(f"spec_image: out must be a dense uint8 {shape} beside the magnitude, got {lib.got(out)}")
    lib.require_gpu(mag)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=mag.device)
    mag = mag.contiguous()                               # dense copies of strided views: bound to names that outlive the launch
    mask = None if mask is None else mask.contiguous()
    call("avsep_spec_image", ptr(mag), ptr(mask),
         float("nan") if thres is None else float(thres), R, F, T, cell, SPEC_REDUCE[reduce], int(bool(log)), float(scale),
         ptr(table), ptr(out))
    return out


def sgd_momentum_(p, g, buf, lr, momentum, weight_decay, grad_scale, first):
    call("avsep_sgd_momentum", ptr(p), ptr(g), ptr(buf), p.numel(), float(lr), float(momentum),
         float(weight_decay), float(grad_scale), int(first))


def temporal_mean(x, B, T):
    chw = x.numel() // (B * T)
    y = _f32((B,) + tuple(x.shape[1:]), x)
    call("avsep_temporal_mean_fwd", ptr(x), B, T, chw, ptr(y))
    return y


def temporal_mean_bwd(dy, B, T):
    chw = dy.numel() // B
    dx = _f32((B * T,) + tuple(dy.shape[1:]), dy)
    call("avsep_temporal_mean_bwd", ptr(dy), B, T, chw, ptr(dx))
    return dx


def maxpool3x3s2(x, scale=None, shift=None, act=0):
    """MaxPool2d(3,2,1) of act(scale*x+shift) (the stem's BN+ReLU folded into the pooling read).  B16 in -> B16 out with a
    one-byte winning-tap image; fp32 in -> fp32 out with int32 flat indices."""
    N, Cc, H, W = dims(x)
    Ho, Wo = out_size(H, 3, 2, 1, 1), out_size(W, 3, 2, 1, 1)
    if is_b16(x):
        y = _b16((N, Cc, Ho, Wo), x)
        idx = torch.empty((N, Cc // 16, Ho, Wo, 16), dtype=torch.uint8, device=x.device)
        call("avsep_b16_maxpool3x3s2_fwd", ptr(x), ptr(scale), ptr(shift), act, N, Cc, H, W, ptr(y), ptr(idx))
        return y, idx
    y = _f32((N, Cc, Ho, Wo), x)
    idx = torch.empty((N, Cc, Ho, Wo), dtype=torch.int32, device=x.device)
    call("avsep_maxpool3x3s2_fwd", ptr(x), ptr(scale), ptr(shift), act, Cc, N * Cc, H, W, ptr(y), ptr(idx))
    return y, idx


def maxpool3x3s2_bwd(dy, idx, H, W):
    N, Cc = dy.shape[:2]
    dx = _f32((N, Cc, H, W), dy)
    call("avsep_maxpool3x3s2_bwd", ptr(dy), ptr(idx), N * Cc, H, W, ptr(dx))
    return dx


def space_to_depth2(x, cp=16, b16=None):
    """[N,C,H,W] -> [N,cp,H/2+3,W/2+3]: the 2x2 phases of x as channels, zero border (2 before, 1 after): see avsep.h.
    With `b16` (default: the arithmetic mode keeps B16 activations) the result is written as a one-block B16 image."""
    N, Cc, H, W = x.shape
    if (want_b16(cp) if b16 is None else b16) and cp == 16:
        xs = _b16((N, 16, H // 2 + 3, W // 2 + 3), x)
        call("avsep_b16_space_to_depth2", ptr(x), N, Cc, H, W, ptr(xs))
        return xs
    xs = _f32((N, cp, H // 2 + 3, W // 2 + 3), x)
    call("avsep_space_to_depth2", ptr(x), N, Cc, H, W, cp, ptr(xs))
    return xs


def maxpool_bn_relu_bwd_stats(g, idx, y, bnrow, bstats, g2=None):
    """BatchNorm-backward sums of the stem tail taken over the pooled grid (see avsep.h); bstats is accumulated into.
    `g2`: a second gradient of the pooled map, added on the fly (B16 images only; fp32 callers add it beforehand)."""
    N, Cc, H, W = dims(y)
    if is_b16(y):
        g, g2 = to_b16(g), to_b16(g2)
        call("avsep_b16_maxpool_bn_relu_bwd", ptr(g), ptr(g2), ptr(idx), ptr(y), ptr(bnrow[0]), ptr(bnrow[1]), ptr(bnrow[2]),
             ptr(bnrow[3]), None, N, Cc, H, W, ptr(bstats), None, 0)
        return
    assert g2 is None
    call("avsep_maxpool_bn_relu_bwd_stats", ptr(to_f32(g)), ptr(idx), ptr(y), ptr(bnrow[0]), ptr(bnrow[1]), ptr(bnrow[2]), ptr(bnrow[3]),
         N, Cc, H, W, ptr(bstats))


def maxpool_bn_relu_bwd_apply(g, idx, y, bnrow, pqr, g2=None, out_f32=False):
    """dL/d(raw stem conv output) from dL/d(pooled): max-pool backward + ReLU mask + folded BatchNorm backward in one pass.
    `out_f32` (B16 inputs): write the result as fp32 NCHW (its only consumer, the stem's weight gradient, is an fp32 kernel)."""
    N, Cc, H, W = dims(y)
    if is_b16(y):
        g, g2 = to_b16(g), to_b16(g2)
        dy = _f32((N, Cc, H, W), y) if out_f32 else torch.empty_like(y)
        call("avsep_b16_maxpool_bn_relu_bwd", ptr(g), ptr(g2), ptr(idx), ptr(y), ptr(bnrow[0]), ptr(bnrow[1]), None, None, ptr(pqr),
             N, Cc, H, W, None, ptr(dy), int(out_f32))
        return dy
    dy = torch.empty_like(y)
    assert g2 is None
    call("avsep_maxpool_bn_relu_bwd_apply", ptr(to_f32(g)), ptr(idx), ptr(y), ptr(bnrow[0]), ptr(bnrow[1]), ptr(pqr), N, Cc, H, W, ptr(dy))
    return dy


MISI_MAX_SOURCES = 8      # avsep_misi: N and G up to 8
MISI_MAX_GROUPS = 8


class Stft:
    """librosa-style STFT/iSTFT plan (bases built once on the device)."""

    def __init__(self, device, n_fft=1022, hop=256, pad_mode="reflect"):
        self.n_fft, self.hop, self.reflect = n_fft, hop, int(pad_mode == "reflect")
        L = lib.load()
        with torch.cuda.device(device):
            self.fwd_basis = torch.empty((L.avsep_stft_basis_floats(n_fft, 0),), dtype=torch.float32, device=device)
            self.inv_basis = torch.empty((L.avsep_stft_basis_floats(n_fft, 1),), dtype=torch.float32, device=device)
            call("avsep_stft_basis", n_fft, ptr(self.fwd_basis), ptr(self.inv_basis))

    def stft(self, wav, want_phase=True):
        """wav [R,L] -> mag, phase [R, n_fft/2+1, 1+L//hop]."""
        R, Ln = wav.shape
        bins, frames = self.n_fft // 2 + 1, 1 + Ln // self.hop
        nbytes = lib.load().avsep_stft_workspace_bytes(R, Ln, self.n_fft, self.hop)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=wav.device)
        mag = _f32((R, bins, frames), wav)
        phase = _f32((R, bins, frames), wav) if want_phase else None
        call("avsep_stft_mag", ptr(wav), R, Ln, self.n_fft, self.hop, self.reflect, ptr(self.fwd_basis), ptr(mag),
             ptr(phase), ptr(ws), nbytes)
        return mag, phase

    def istft(self, mag, phase):
        R, bins, frames = mag.shape
        out_len = self.hop * (frames - 1)
        nbytes = lib.load().avsep_istft_workspace_bytes(R, self.n_fft, frames)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=mag.device)
        wav = _f32((R, out_len), mag)
        call("avsep_istft", ptr(mag), ptr(phase), R, self.n_fft, self.hop, frames, ptr(self.inv_basis), ptr(wav),
             out_len, ptr(ws), nbytes)
        return wav

    def misi(self, mix, mag, phase, iterations, want_phase=False):
        """Mixture-consistent phase iterations (include/avsep.h, csrc/misi.hip): mix [G,out_len] the mixtures, mag
        [N,G,bins,F] the stems' target magnitudes (row (n, g) belongs to mixture g), phase the start phase, [G,bins,F]
        shared by the sources or [N,G,bins,F]; out_len = hop * (F - 1).  -> wav [N,G,out_len] after ``iterations`` passes
        (the plain iSTFT of the last spectrum: the stems are not forced to sum to the mixture), and with want_phase also the
        last phase [N,G,bins,F].  One call enqueues every pass; a second call gives the same bits."""
        for t in (mix, mag, phase):
            lib.require_gpu(t)
        bins = self.n_fft // 2 + 1
        if mag.dim() != 4 or mag.dtype != torch.float32 or mag.shape[2] != bins:
            raise lib.AvsepError(f"misi takes mag f32 [N,G,{bins},F], got {mag.dtype} {tuple(mag.shape)}")
        N, G, _, F = mag.shape
        if not (1 <= N <= MISI_MAX_SOURCES and 1 <= G <= MISI_MAX_GROUPS):
            raise lib.AvsepError(f"misi: 1 <= N <= {MISI_MAX_SOURCES}, 1 <= G <= {MISI_MAX_GROUPS}; got {tuple(mag.shape)}")
        out_len = self.hop * (F - 1)
        if out_len <= self.n_fft // 2:
            raise lib.AvsepError(f"misi needs hop * (F - 1) > n_fft / 2 samples, got F = {F} at {self.n_fft}/{self.hop}")
        if phase.dtype != torch.float32 or phase.device != mag.device \
                or tuple(phase.shape) not in (tuple(mag.shape), tuple(mag.shape[1:])):
            raise lib.AvsepError(f"misi takes phase f32 [{G},{bins},{F}] (shared by the sources) or [{N},{G},{bins},{F}] on "
                                 f"{mag.device}, got {phase.dtype} {tuple(phase.shape)} on {phase.device}")
        if mix.dtype != torch.float32 or tuple(mix.shape) != (G, out_len) or mix.device != mag.device:
            raise lib.AvsepError(f"misi takes mix f32 [{G},{out_len}] on {mag.device}, got {mix.dtype} {tuple(mix.shape)} on {mix.device}")
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise lib.AvsepError(f"misi needs iterations as an int >= 1, got {iterations!r}")
        mix, mag, phase = mix.contiguous(), mag.contiguous(), phase.contiguous()
        nbytes = lib.load().avsep_misi_workspace_bytes(N, G, self.n_fft, self.hop, F)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=mag.device)
        wav = _f32((N, G, out_len), mag)
        ph = _f32((N, G, bins, F), mag) if want_phase else None
        call("avsep_misi", ptr(mix), ptr(mag), ptr(phase), int(phase.dim() == 4), N, G, self.n_fft, self.hop, F, self.reflect,
             iterations, ptr(self.fwd_basis), ptr(self.inv_basis), ptr(wav), ptr(ph), ptr(ws), nbytes)
        return (wav, ph) if want_phase else wav
