"""The im2col kernel's loader forms and the halo kernel's 1x1 / stride-2 calls against float64 (tests/convref.py).

igemm_kernel<fwd>, <dgrad> and <wgrad> gather their im2col operand through buffer loads: a bit mask of the taps that lie
outside the image (per column; per pixel in the weight gradient), a per-row decode table in LDS (per-column registers in the
weight gradient), and an out-of-range offset that makes the load return 0 in place of a compare and a select.  The shapes below are the smallest at which each piece can go wrong: every window on a border, the
parity classes of a strided data gradient, split-K, a two-source concat with an affine whose shift must not leak into the
padding, a wave whose rows straddle the two sources, one input channel, a ragged tile in both directions.  Every call first asserts the kernel family that serves it, so
a re-routed case fails instead of passing on another kernel.  The data gradient is always written into a dX pre-filled with
NaN: a position the kernel leaves out shows.  Bound: max|d| / max|ref| <= 2e-5, that of test_gpu_ops.test_conv_fwd_dgrad_wgrad.

One host test (no GPU): a descriptor whose gathered tensor reaches the 32-bit range guard reports the 64-bit loader."""
import ctypes

import pytest
import torch

import convref
from conftest import assert_close
from recipes import pkg as _pkg

TOL = 2e-5
IGEMM = {"fwd": "igemm_kernel<fwd>", "dgrad": "igemm_kernel<dgrad>", "wgrad": "igemm_kernel<wgrad>"}
HALO = {"fwd": "conv3x3_kernel", "dgrad": "conv3x3_kernel"}

RAW = None      # no affine in front of the sources; otherwise the activation behind a per-channel affine (0 none, 1 ReLU, 2 LeakyReLU)
# name: (N, Cin, H, W, Cout, k, stride, pad, dil), C0 (None = one source), RAW or the activation behind an affine, {mode: family}
CASES = {
    "deep_4x4s2_splitk": ((8, 512, 4, 4, 512, 4, 2, 1, 1), None, RAW, IGEMM),     # every window on a border, split-K both ways
    "mid_4x4s2": ((2, 64, 16, 16, 128, 4, 2, 1, 1), None, RAW, IGEMM),
    "concat_affine_relu": ((3, 64, 4, 4, 48, 3, 1, 1, 1), 32, 1, IGEMM),          # shift != 0 must not reach the padding
    "concat_raw": ((3, 64, 4, 4, 48, 3, 1, 1, 1), 32, RAW, IGEMM),
    # 25 + 39 channels: C0 * 9 = 225 is no multiple of a wave's 4 rows, so one wave's rows of a forward K-tile straddle the switch
    # from source 0 to source 1 (the loader's mixed class); the weight gradient's straddling workgroup loads from both resources
    "concat_odd_affine_relu": ((3, 64, 4, 4, 48, 3, 1, 1, 1), 25, 1, IGEMM),
    "concat_odd_raw": ((3, 64, 4, 4, 48, 3, 1, 1, 1), 25, RAW, IGEMM),
    # one input channel behind the folded BatchNorm of the benched first conv: K = 16 keeps the forward on the 64-bit loader, the
    # weight gradient has 16 columns in a 64-column tile (48 columns take the always-invalid tap).  Without the affine the weight
    # gradient of <= 4 input channels has its own kernel.
    "cin1_affine": ((2, 1, 32, 48, 24, 4, 2, 1, 1), None, 0, {"fwd": IGEMM["fwd"], "wgrad": IGEMM["wgrad"]}),
    "cin1_raw": ((2, 1, 32, 48, 24, 4, 2, 1, 1), None, RAW, {"fwd": IGEMM["fwd"]}),
    "wgrad_1x1": ((3, 64, 14, 14, 144, 1, 1, 0, 1), None, RAW, {"wgrad": IGEMM["wgrad"]}),
    "ragged": ((3, 24, 5, 7, 40, 3, 1, 1, 1), None, RAW, IGEMM),                  # 105 columns, K = 216: partial tiles both ways
    "ragged_affine_lrelu": ((3, 24, 5, 7, 40, 3, 1, 1, 1), None, 2, IGEMM),
    # 1x1 / stride 2 on the halo kernel: the data gradient owns the zeros of the skipped pixels
    "halo_1x1s2_layer2": ((2, 64, 56, 56, 128, 1, 2, 0, 1), None, RAW, HALO),
    "halo_1x1s2_ragged": ((2, 32, 12, 40, 48, 1, 2, 0, 1), None, RAW, HALO),
}


def _dgrad_into_nan(K, cv, wp, dy, misalign=False):
    """cv.dgrad with the destination pre-filled with NaN; `misalign`: a dX that is 4- but not 8-byte aligned."""
    need, _ = cv.io_formats(1)
    assert need == K.FMT_F32
    cv.d.dyfmt = cv.d.dxfmt = K.FMT_F32
    shape = (cv.N, cv.Cin, cv.H, cv.W)
    flat = torch.full((cv.N * cv.Cin * cv.H * cv.W + 2,), float("nan"), dtype=torch.float32, device=dy.device)
    off = (2 if flat.data_ptr() % 8 else 1) if misalign else (1 if flat.data_ptr() % 8 else 0)
    dx = flat[off:off + flat.numel() - 2].view(shape)
    assert dx.data_ptr() % 8 == (4 if misalign else 0)
    ws, nbytes = cv._ws("avsep_conv2d_dgrad_workspace_bytes")
    K.call("avsep_conv2d_dgrad", cv.ref, K.ptr(wp), K.ptr(dy), K.ptr(dx), K.ptr(ws), nbytes)
    return dx


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_igemm_forms(dev, name):
    K = _pkg().kernels
    (N, Cin, H, W, Cout, k, s, p, d), C0, aff, families = CASES[name]
    g = torch.Generator().manual_seed(sum((N, Cin, H, W, Cout, k, s, p, d)) + (0 if aff is RAW else aff + 1))
    C0 = Cin if C0 is None else C0
    x = torch.randn(N, Cin, H, W, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(dev)
    b = torch.randn(Cout, generator=g).to(dev)
    x0, x1 = x[:, :C0].contiguous(), (x[:, C0:].contiguous() if C0 < Cin else None)
    kw, op = {}, {"x0": x0, "x1": x1, "w": w, "bias": b, "stats": True, "want_bias": True}
    if aff is not RAW:
        sc = (torch.rand(Cin, generator=g) + 0.5).to(dev)
        sh = (torch.randn(Cin, generator=g) * 0.3 + 0.5).to(dev)          # act(shift) != 0 on most channels
        kw = dict(sc0=sc[:C0].contiguous(), sh0=sh[:C0].contiguous(), act0=aff)
        if x1 is not None:
            kw.update(sc1=sc[C0:].contiguous(), sh1=sh[C0:].contiguous(), act1=aff)
        op.update({n: kw.get(n) for n in ("sc0", "sh0", "sc1", "sh1")})
    cv = K.Conv(x0, Cout, k, s, p, d, x1=x1, **kw)
    for mode, fam in families.items():
        assert cv.kernel_name(mode) == fam, (name, mode, cv.kernel_variant(mode))
    dy = torch.randn(N, Cout, cv.Ho, cv.Wo, generator=g).to(dev)
    op["dy"] = dy
    if "fwd" in families:
        ref = convref.reference(cv, "fwd", op)
        st = K.zeros_stats(Cout, x0)
        y = cv.fwd(cv.pack(w, 0), b, st)
        assert_close(y, ref["y"][0], TOL, "fwd")
        assert_close(st, ref["stats"][0], TOL, "BatchNorm statistics")
    if "dgrad" in families:
        ref = convref.reference(cv, "dgrad", op)
        dx = _dgrad_into_nan(K, cv, cv.pack(w, 1), dy)
        assert not torch.isnan(dx).any(), "dgrad left elements of dX unwritten"
        assert_close(dx, ref["dx"][0], TOL, "dgrad")
        if families is HALO:       # the 8-byte zero-fill stores need an 8-byte aligned dX: any other is filled first
            dx = _dgrad_into_nan(K, cv, cv.pack(w, 1), dy, misalign=True)
            assert not torch.isnan(dx).any(), "dgrad left elements of a 4-byte aligned dX unwritten"
            assert_close(dx, ref["dx"][0], TOL, "dgrad into a 4-byte aligned dX")
    if "wgrad" in families:
        ref = convref.reference(cv, "wgrad", op)
        dw, db = cv.wgrad(dy, want_bias=True)
        assert_close(dw, ref["dw"][0], TOL, "wgrad")
        assert_close(db, ref["dbias"][0], TOL, "dbias")


def _desc(N, Cin, H, W, Cout, k, pad, C0=None):
    d = _pkg().lib.ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout, d.KH, d.KW, d.stride, d.pad, d.dil = N, Cin, H, W, Cout, k, k, 1, pad, 1
    d.Ho, d.Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    d.C0 = Cin if C0 is None else C0
    d.x0 = 256                                   # a non-null address: the queries read sizes only
    if d.C0 < Cin:
        d.x1 = 256
    return d


def _variants(d):
    L = _pkg().lib.load()
    buf = ctypes.create_string_buffer(128)
    out = []
    for mode in (0, 1, 2):
        assert L.avsep_conv_kernel_variant(ctypes.byref(d), mode, 1, buf, 128) == 0
        out.append(buf.value.decode())
    return out


def test_range_guard_selects_64bit_loader():
    """The buffer loader addresses a gathered tensor with 32-bit byte offsets: it serves a call only while
    4 * elements + 16 < 0xfffffff0 holds for every gathered tensor (both sources of x; dY for the data gradient).  The
    variant string of a call beyond that names the 64-bit loader ("ld64"); sizes alone decide, nothing is allocated."""
    limit = (0xfffffff0 - 16 + 3) // 4            # the first element count that no longer fits
    assert limit == 8 * 511 * 262657
    at = _variants(_desc(1, 8, 511, 262657, 8, 5, 2))             # x and dY of exactly `limit` elements
    assert at == ["igemm_kernel<fwd>:BM64,split1,ld64", "igemm_kernel<dgrad>:BM64,split1,ld64", "igemm_kernel<wgrad>:ld64"], at
    assert limit - 1 == 5 * 214748363
    below = _variants(_desc(1, 5, 1, 214748363, 5, 5, 2))          # one element fewer
    assert below == ["igemm_kernel<fwd>:BM64,split1", "igemm_kernel<dgrad>:BM64,split1", "igemm_kernel<wgrad>"], below
    second = _variants(_desc(1, 9, 511, 262657, 8, 5, 2, C0=1))    # the second source alone is too large
    assert second[0].endswith(",ld64") and second[2].endswith("ld64"), second
