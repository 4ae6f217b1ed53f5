"""numpy restatement of the multichannel Wiener filter with time-varying spatial covariances (include/avsep.h, DESIGN.md
§24), the reference of test_mwf_tv_host.py and test_gpu_mwf_tv.py.  It stands on mwf_ref.py and changes one
definition: the covariance of a source is no longer one matrix per bin row but one per bin row and CENTRE, and the matrix
used at a frame is the blend of the two centres next to it.  ``dtype=np.float64`` is the reference; ``dtype=np.float32``
runs the same steps, weights, sums, solve and polar conversions included, in single precision: its distance from the
float64 mode sizes the tolerance of the GPU test.

H is the span in frames (a multiple of 64, 64 ... 4096).  Centres sit at frames k H, k = 0 ... K-1, K = ceil((F-1)/H) + 1
(K = 1 for F = 1).  Frame t lies in segment s = t // H at u = (t - s H) / H: centre s weighs it with 1 - u and centre s + 1
with u, which is the hat w_k(t) = max(0, 1 - |t - k H| / H).  One pass:
  1.  v_n[f,t]   = (1/C) sum_c ymag[n,c,f,t]^2
  2'. R_n[k,f]   = (sum_t w_k(t) Y_n Y_n^H) / max(sum_t w_k(t) v_n, FLT_MIN)
  3'. R_n[f,t]   = sum_k w_k(t) R_n[k,f]
  3.  S[f,t]     = sum_n v_n R_n[f,t] + (reg * tr(sum_n v_n R_n[f,t]) / C + FLT_MIN) I
  4.  S z = X
  5.  Y_n'       = v_n R_n[f,t] z   (exactly 0 where v_n = 0), written as |.| and atan2 (0 at 0)

``moving_sources`` is mwf_ref.panned_sources with pan angles that sweep over the recording: the scene the feature is for."""
import numpy as np

import mwf_ref as M
from mwf_ref import FLT_MIN, REG, complex_to_polar, mean_sdr, polar_to_complex, rel_err, value_inputs  # noqa: F401

MIN_SPAN, MAX_SPAN = 64, 4096


def span_ok(H):
    return isinstance(H, int) and not isinstance(H, bool) and MIN_SPAN <= H <= MAX_SPAN and H % 64 == 0


def centres(F, H):
    """K: the last centre is the first one at or past the last frame."""
    return 1 if F == 1 else -(-(F - 1) // H) + 1


def segments(F, H):
    """-> (s, u), both [F]: the segment of every frame and its place in it (exact in float64 and float32: a quotient of
    two small integers rounded once)."""
    t = np.arange(F)
    s = t // H
    return s, (t - s * H) / np.float64(H)


def hat_weights(F, H, dtype=np.float64):
    """-> W [K, F], W[k, t] = w_k(t); at most two entries of a column are non-zero and they sum to 1."""
    s, u = segments(F, H)
    u = u.astype(dtype)
    W = np.zeros((centres(F, H), F), dtype)
    t = np.arange(F)
    W[s, t] = dtype(1) - u
    up = u > 0                                     # u = 0: the frame sits on centre s, and centre s + 1 may not exist
    W[s[up] + 1, t[up]] = u[up]
    return W


def cov(ymag, yph, H, dtype=np.float64):
    """Steps 1-2': ymag [N,C,Fin,F], yph [C,Fin,F] or [N,C,Fin,F] -> (R complex [N,K,Fin,C,C], v [N,Fin,F])."""
    ymag = np.asarray(ymag).astype(dtype)
    yph = np.broadcast_to(np.asarray(yph).astype(dtype), ymag.shape)
    C, F = ymag.shape[1], ymag.shape[3]
    Y = polar_to_complex(ymag, yph, dtype)
    v = ((ymag * ymag).sum(1) / dtype(C)).astype(dtype)
    Wt = hat_weights(F, H, dtype).T                                            # [F, K]
    YY = np.einsum("ncft,ndft->nfcdt", Y, Y.conj())
    num = np.empty(YY.shape[:-1] + (Wt.shape[1],), M._cplx(dtype))
    num.real = YY.real @ Wt
    num.imag = YY.imag @ Wt
    den = np.maximum(v @ Wt, dtype(FLT_MIN))                                   # [N,Fin,K]
    R = num / den[:, :, None, None, :]
    return np.ascontiguousarray(R.transpose(0, 4, 1, 2, 3)).astype(M._cplx(dtype)), v


def at_frames(R, F, H, dtype=np.float64):
    """Step 3': R [N,K,Fin,C,C] -> R_n[f,t] as [N,Fin,F,C,C], (1 - u) R[s] + u R[s + 1]."""
    s, u = segments(F, H)
    u = u.astype(dtype)[None, :, None, None, None]
    nxt = np.minimum(s + 1, R.shape[1] - 1)                                    # u = 0 wherever s + 1 is past the last centre
    Rt = (dtype(1) - u) * R[:, s] + u * R[:, nxt]                              # [N,F,Fin,C,C]
    return np.ascontiguousarray(Rt.transpose(0, 2, 1, 3, 4)).astype(M._cplx(dtype))


def apply(xmag, xph, v, R, H, reg=REG, dtype=np.float64):
    """Steps 3'-5 -> Y' complex [N,C,Fin,F]."""
    X = polar_to_complex(xmag, xph, dtype)                                     # [C,Fin,F]
    C, F = X.shape[0], X.shape[2]
    Rt = at_frames(R, F, H, dtype)
    S = np.einsum("nft,nftcd->ftcd", v.astype(M._cplx(dtype)), Rt)
    tr = np.einsum("ftcc->ft", S).real.astype(dtype)
    lam = (dtype(reg) * tr / dtype(C) + dtype(FLT_MIN)).astype(dtype)
    S = (S + lam[:, :, None, None] * np.eye(C, dtype=dtype)).astype(M._cplx(dtype))
    with np.errstate(invalid="ignore", over="ignore"):                         # all sources silent at a bin the mixture is not
        z = np.linalg.solve(S, X.transpose(1, 2, 0)[..., None])[..., 0]        # [Fin,F,C]
        W = np.einsum("nftcd,ftd->ncft", Rt, z) * v[:, None].astype(dtype)
    return np.where(v[:, None] == 0, 0, W).astype(M._cplx(dtype))


def mwf(xmag, xph, ymag, yph, H, iterations=1, reg=REG, dtype=np.float64):
    """``iterations`` passes.  -> {"cov": R of the first pass [N,K,Fin,C,C], "mag", "phase": [N,C,Fin,F] as the kernel
    stores them, "Y": mag * exp(i phase) evaluated in float64}."""
    mag, ph, first = np.asarray(ymag), np.asarray(yph), None
    for _ in range(int(iterations)):
        R, v = cov(mag, ph, H, dtype)
        first = R if first is None else first
        mag, ph = complex_to_polar(apply(xmag, xph, v, R, H, reg, dtype), dtype)
    return {"cov": first, "mag": mag, "phase": ph, "Y": polar_to_complex(mag, ph, np.float64)}


# ---------------------------------------------------------------------------------------------------------------------
# the value cases of test_gpu_mwf_tv.py (here, so that the CPU test that sizes the tolerance runs exactly the same inputs)
# ---------------------------------------------------------------------------------------------------------------------
FIN = M.FIN
F_LONG = M.F_LONG           # 2 * 2048 + 77: a long odd remainder
# (C, N, F, H): every C in {1, 2, 3, 8}, every N in {1, 2, 3}, every H in {64, 128, 192} and every F in
# {1, 63, 64, 65, 257, F_LONG} at least once.  F = 1: one centre; 63: a lone partial segment; 64: the last centre just past
# the last frame; 65: the last centre on the last frame (a segment of one frame at u = 0); 257: a one-frame second tile of
# the apply kernel; H = 192 does not divide that kernel's 256-frame tile.
VALUE_SHAPES = [(1, 1, 63, 64), (1, 3, F_LONG, 192), (2, 1, 1, 64), (2, 2, 64, 64), (2, 2, 65, 64), (2, 3, 257, 128),
                (2, 2, 257, 192), (2, 2, F_LONG, 64), (3, 3, 63, 128), (3, 2, 257, 64), (3, 2, F_LONG, 128), (8, 2, 1, 192),
                (8, 2, 65, 64), (8, 1, 257, 192), (8, 3, F_LONG, 192)]
VALUE_CASES = [(C, N, F, H, it) for (C, N, F, H) in VALUE_SHAPES for it in (1, 2)]

# (C, N, F, H) at which the two apply kernels are tied to each other (one covariance repeated at every centre makes the blend
# a no-op up to rounding): a one-frame second tile, a span that does not divide the 256-frame tile, and the clamped last
# centre at the widest C
TIE_SHAPES = [(2, 2, 257, 64), (3, 2, 257, 192), (8, 2, 65, 64)]


# Worst max|d|/max|ref| of the float32 mode against the float64 mode over VALUE_CASES, measured on the CPU
# (test_mwf_tv_host.py re-measures it): 4.703e-07 for the filtered images and 8.474e-07 for the covariances (both at C = 8,
# N = 3, F = 4173, H = 192; a centre sums at most 2 H - 1 frames, so the covariances sit below §16's 2.5e-06 over 4173).
# Recorded rounded up; a kernel is given 16 x, the margin and the reasons of DESIGN.md §16: another summation order over t,
# sincosf / atan2f on both sides, and a Cholesky where LAPACK pivots.
F32_WORST_Y, F32_WORST_COV = 4.8e-7, 8.5e-7
BOUND_Y, BOUND_COV = 16 * F32_WORST_Y, 16 * F32_WORST_COV          # 7.68e-06, 1.36e-05


# ---------------------------------------------------------------------------------------------------------------------
# the scene the local covariances are for
# ---------------------------------------------------------------------------------------------------------------------
def moving_sources(C=2, N=2, Fin=48, F=640, seed=0, sweep_deg=90.0, mask_noise=0.25, noise=0.01):
    """mwf_ref.panned_sources (same draws in the same order) with sources that move: source n has pan angle
        base_n + sweep_deg * (t / (F - 1) - 1/2) * (+1 for even n, -1 for odd n),
    base_n spread evenly over 22.5 ... 67.5 degrees; even channels take cos and odd channels sin of the angle, every
    (n, c) gets one fixed phase from U(-0.5, 0.5) rad, and h_n[:, t] is normalised per frame.  sweep_deg = 0 is
    panned_sources.  -> the same dict: float32 xmag, xph [C,Fin,F], ymag [N,C,Fin,F], float64 truth "images"."""
    g = np.random.default_rng(seed)
    act = g.random((N, Fin, F)) < 0.5
    s = act * 30.0 * (g.standard_normal((N, Fin, F)) + 1j * g.standard_normal((N, Fin, F))) / np.sqrt(2.0)
    pos = np.arange(F) / max(F - 1, 1) - 0.5
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    th = np.deg2rad(np.linspace(22.5, 67.5, N)[:, None] + sweep_deg * pos[None, :] * sign[:, None])           # [N,F]
    h = np.stack([np.cos(th) if c % 2 == 0 else np.sin(th) for c in range(C)], 1) \
        * np.exp(1j * g.uniform(-0.5, 0.5, (N, C)))[:, :, None]                                              # [N,C,F]
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    images = h[:, :, None, :] * s[:, None]
    X = images.sum(0) + noise * 30.0 * (g.standard_normal((C, Fin, F)) + 1j * g.standard_normal((C, Fin, F))) / np.sqrt(2.0)
    e = np.sqrt((np.abs(images) ** 2).sum(1))                                   # [N,Fin,F]
    mask = np.clip(e / np.maximum(e.sum(0), 1e-12) + mask_noise * g.standard_normal((N, Fin, F)), 0.0, 1.0)
    xmag, xph = np.abs(X).astype(np.float32), np.angle(X).astype(np.float32)
    ymag = (mask[:, None].astype(np.float32) * xmag[None]).astype(np.float32)
    return {"xmag": xmag, "xph": xph, "ymag": ymag, "images": images}
