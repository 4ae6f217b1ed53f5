"""numpy restatement of the multichannel Wiener filter (include/avsep.h), the reference of test_mwf_host.py and
test_gpu_mwf.py.  ``dtype=np.float64`` is the reference; ``dtype=np.float32`` runs the same five steps, the polar <-> Cartesian
conversions at both ends of a pass included, in single precision (complex64 einsum and LAPACK solve): its distance from the
float64 mode on a test's inputs is the size of an honest fp32 implementation's error, and sizes the tolerance there.

One pass, X [C,Fin,F] the channels' STFT and Y [N,C,Fin,F] the current source images, both given as magnitude and phase:
  1. v_n[f,t] = (1/C) sum_c ymag[n,c,f,t]^2
  2. R_n[f]   = (sum_t Y_n Y_n^H) / max(sum_t v_n, FLT_MIN)
  3. S[f,t]   = sum_n v_n R_n + (reg * tr(sum_n v_n R_n) / C + FLT_MIN) I
  4. S z = X
  5. Y_n'     = v_n R_n z   (exactly 0 where v_n = 0), written as |.| and atan2 (0 at 0)

``panned_sources`` is the synthetic stereo scene both test files use to show what the filter is for."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
REG = 1e-3


def _cplx(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def polar_to_complex(mag, ph, dtype=np.float64):
    mag, ph = np.asarray(mag).astype(dtype), np.asarray(ph).astype(dtype)
    out = np.empty(mag.shape, _cplx(dtype))
    out.real = mag * np.cos(ph)
    out.imag = mag * np.sin(ph)
    return out


def complex_to_polar(z, dtype=np.float64):
    z = np.asarray(z).astype(_cplx(dtype))
    ph = np.arctan2(z.imag, z.real).astype(dtype)
    ph[(z.real == 0) & (z.imag == 0)] = 0
    return np.abs(z).astype(dtype), ph


def cov(ymag, yph, dtype=np.float64):
    """Steps 1-2: ymag [N,C,Fin,F], yph [C,Fin,F] or [N,C,Fin,F] -> (R complex [N,Fin,C,C], v [N,Fin,F])."""
    ymag = np.asarray(ymag).astype(dtype)
    yph = np.broadcast_to(np.asarray(yph).astype(dtype), ymag.shape)
    C = ymag.shape[1]
    Y = polar_to_complex(ymag, yph, dtype)
    v = ((ymag * ymag).sum(1) / dtype(C)).astype(dtype)
    num = np.einsum("ncft,ndft->nfcd", Y, Y.conj())
    den = np.maximum(v.sum(-1), dtype(FLT_MIN))
    return (num / den[:, :, None, None]).astype(_cplx(dtype)), v


def apply(xmag, xph, v, R, reg=REG, dtype=np.float64):
    """Steps 3-5 -> Y' complex [N,C,Fin,F]."""
    X = polar_to_complex(xmag, xph, dtype)                                     # [C,Fin,F]
    C = X.shape[0]
    S = np.einsum("nft,nfcd->ftcd", v.astype(_cplx(dtype)), R)
    tr = np.einsum("ftcc->ft", S).real.astype(dtype)
    lam = (dtype(reg) * tr / dtype(C) + dtype(FLT_MIN)).astype(dtype)
    S = (S + lam[:, :, None, None] * np.eye(C, dtype=dtype)).astype(_cplx(dtype))
    with np.errstate(invalid="ignore", over="ignore"):                         # all sources silent at a bin the mixture is not
        z = np.linalg.solve(S, X.transpose(1, 2, 0)[..., None])[..., 0]        # [Fin,F,C]
        W = np.einsum("nfcd,ftd->ncft", R, z) * v[:, None].astype(dtype)
    return np.where(v[:, None] == 0, 0, W).astype(_cplx(dtype))


def mwf(xmag, xph, ymag, yph, iterations=1, reg=REG, dtype=np.float64):
    """``iterations`` passes.  -> {"cov": R of the first pass [N,Fin,C,C], "mag", "phase": [N,C,Fin,F] as the kernel stores
    them, "Y": mag * exp(i phase) evaluated in float64}."""
    mag, ph, first = np.asarray(ymag), np.asarray(yph), None
    for _ in range(int(iterations)):
        R, v = cov(mag, ph, dtype)
        first = R if first is None else first
        mag, ph = complex_to_polar(apply(xmag, xph, v, R, reg, dtype), dtype)
    return {"cov": first, "mag": mag, "phase": ph, "Y": polar_to_complex(mag, ph, np.float64)}


# ---------------------------------------------------------------------------------------------------------------------
# the value cases of test_gpu_mwf.py (here, so that the CPU test that sizes the tolerance runs exactly the same inputs)
# ---------------------------------------------------------------------------------------------------------------------
FIN = 5                     # no multiple of any row tile
F_LONG = 2 * 2048 + 77      # two whole covariance chunks of 2048 frames and an odd remainder
# (C, N, F): every C in {1, 2, 3, 8}, every N in {1, 2, 3}, every F in {1, 63, F_LONG} at least once
VALUE_SHAPES = [(1, 1, 63), (1, 3, F_LONG), (2, 1, 1), (2, 2, F_LONG), (3, 3, 63), (3, 2, F_LONG), (8, 2, 1), (8, 2, 63),
                (8, 3, F_LONG)]
VALUE_CASES = [(C, N, F, it) for (C, N, F) in VALUE_SHAPES for it in (1, 2)]


# Worst max|d|/max|ref| of the float32 mode against the float64 mode over VALUE_CASES, measured on the CPU (complex64 einsum
# and LAPACK; test_mwf_host.py re-measures it): 1.897e-06 for the filtered images, 2.462e-06 for the covariances (numpy's
# sequential float32 sum over F_LONG frames).  Recorded rounded up; a kernel is given 16 x: another summation order over t,
# sincosf / atan2f on both sides, and a Cholesky where LAPACK pivots.
F32_WORST_Y, F32_WORST_COV = 1.9e-6, 2.5e-6
BOUND_Y, BOUND_COV = 16 * F32_WORST_Y, 16 * F32_WORST_COV          # 3.04e-05, 4.0e-05


def value_inputs(C, N, F, seed=None):
    """Random masks in (0, 1) on a random complex mixture of magnitude about 30 (|30 * complex normal|), float32:
    -> xmag, xph [C,FIN,F], ymag [N,C,FIN,F] = mask * xmag (the first pass's phase is xph)."""
    g = np.random.default_rng(1000 * C + 100 * N + F if seed is None else seed)
    X = 30.0 * (g.standard_normal((C, FIN, F)) + 1j * g.standard_normal((C, FIN, F))) / np.sqrt(2.0)
    xmag, xph = np.abs(X).astype(np.float32), np.angle(X).astype(np.float32)
    mask = g.random((N, FIN, F)).astype(np.float32)
    return xmag, xph, (mask[:, None] * xmag[None]).astype(np.float32)


def rel_err(got, ref):
    """max |got - ref| / max |ref| (complex or real arrays)."""
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(got) - ref).max() / max(np.abs(ref).max(), FLT_MIN))


# ---------------------------------------------------------------------------------------------------------------------
# the scene the filter is for
# ---------------------------------------------------------------------------------------------------------------------
def panned_sources(C=2, N=2, Fin=48, F=160, seed=0, mask_noise=0.25, noise=0.01):
    """N sources, each at a fixed place in a C-channel image.
    * source n: s_n[f,t] = a_n[f,t] * 30 * (g + i g') / sqrt(2), g, g' ~ N(0,1), a_n ~ Bernoulli(1/2) per bin (sources
      overlap on about a quarter of the bins and are alone on another quarter each);
    * its image: I_n[c,f,t] = h_n[c] * s_n[f,t] with one complex gain per channel: the sources are panned at angles
      spread evenly over 22.5 ... 67.5 degrees, even channels take cos and odd channels sin of the angle, every gain gets a
      phase drawn once from U(-0.5, 0.5) rad and h_n is normalised: the spatial covariance of source n is h_n h_n^H in
      every bin row;
    * mixture: X = sum_n I_n + noise * 30 * complex normal;
    * what a mono separator hands over: the ideal ratio mask of the image energies, |I_n| / sum_m |I_m| (|.| over the
      channels), plus N(0, mask_noise^2) per bin, clipped to [0, 1].
    -> dict of float32 arrays xmag, xph [C,Fin,F], ymag [N,C,Fin,F] (= mask * xmag: per-channel masking, on phase xph) and
    the float64 truth "images" [N,C,Fin,F] complex."""
    g = np.random.default_rng(seed)
    act = g.random((N, Fin, F)) < 0.5
    s = act * 30.0 * (g.standard_normal((N, Fin, F)) + 1j * g.standard_normal((N, Fin, F))) / np.sqrt(2.0)
    th = np.deg2rad(np.linspace(22.5, 67.5, N))
    h = np.stack([np.cos(th) if c % 2 == 0 else np.sin(th) for c in range(C)], 1) * np.exp(1j * g.uniform(-0.5, 0.5, (N, C)))
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    images = h[:, :, None, None] * s[:, None]
    X = images.sum(0) + noise * 30.0 * (g.standard_normal((C, Fin, F)) + 1j * g.standard_normal((C, Fin, F))) / np.sqrt(2.0)
    e = np.sqrt((np.abs(images) ** 2).sum(1))                                   # [N,Fin,F]
    mask = np.clip(e / np.maximum(e.sum(0), 1e-12) + mask_noise * g.standard_normal((N, Fin, F)), 0.0, 1.0)
    xmag, xph = np.abs(X).astype(np.float32), np.angle(X).astype(np.float32)
    ymag = (mask[:, None].astype(np.float32) * xmag[None]).astype(np.float32)
    return {"xmag": xmag, "xph": xph, "ymag": ymag, "images": images}


def mean_sdr(est, images):
    """Mean over the sources of 10 log10(|image|^2 / |image - estimate|^2), sums over channels, bins and frames."""
    num = (np.abs(images) ** 2).sum((1, 2, 3))
    den = (np.abs(images - est) ** 2).sum((1, 2, 3))
    return float(np.mean(10.0 * np.log10(num / den)))


def masking_sdr(scene):
    """SDR of per-channel masking: ymag on the mixture's phase."""
    return mean_sdr(polar_to_complex(scene["ymag"], np.broadcast_to(scene["xph"], scene["ymag"].shape)), scene["images"])
