"""Per-entry and per-bin float64 gates for the Wiener filter's launchers (csrc/mwf.hip), used by
test_mwf_gates_host.py (no device) and test_gpu_mwf_gates.py.  It stands on mwf_ref.py / mwf_tv_ref.py (§16, §24) and adds what
a gate per element needs and those restatements do not return:
  * ``cov_ref``: the covariances AND ``absref``, the same sums over absolute values;
  * ``apply_ref``: steps 3-5 on a GIVEN fp32 covariance tensor (cast exactly), and per bin kappa_2(S), ||v_n R_n||_2, ||z||_2;
  * ``K`` / ``k_cov`` / ``k_apply``: the constants of the two bounds, counted from the source lines beside them;
  * ``cov_control`` / ``apply_control``: float32 NumPy evaluations (the covariance one adds in the kernel's order), which must
    pass the gates, and the mutants of them, which must not.
H = 0 is the time-invariant filter (TV = false), H > 0 the span of the time-varying one (TV = true).  All bounds are in units of
U = 2^-24, the fp32 unit roundoff; one ulp is 2 U.  Subnormal intermediates are out of scope (mwf_cases.py keeps the rows out
of them and test_mwf_gates_host.py asserts it)."""
import math

import numpy as np

import mwf_ref as M
import mwf_tv_ref as T
from recipes import cdiv

U = 2.0 ** -24
FLT_MIN = M.FLT_MIN
BLOCK, CHUNK, WAVES = 256, 2048, 4                  # MWF_BLOCK, MWF_CHUNK, MWF_WAVES
FN = 4                                              # a math function at 2 ulp (sincosf, sqrtf, atan2f), in U
SQRT2 = math.sqrt(2.0)
f32, f64 = np.float32, np.float64


def chunks(F):
    return cdiv(F, CHUNK)


def nacc(C):
    return C * (C + 1) + 1


def nout(C):
    """registers a lane of the TV partial kernel stores: (2 NACC + 63) / 64"""
    return (2 * nacc(C) + 63) // 64


def workspace_bytes(N, C, Fin, F, H=0):
    """one slab of NACC floats per (chunk, source, bin row), or two per (segment, source, bin row)"""
    return (2 * cdiv(F, H) if H else chunks(F)) * N * Fin * nacc(C) * 4


# ---------------------------------------------------------------------------------------------------------------------
# the constants, counted
# ---------------------------------------------------------------------------------------------------------------------
def k_weight(H, j=None):
    """The hat weight of a frame, `u = (float)j / fH, w = 1.f - u` (mwf_cov_partial_kernel, and `u = (float)(t - seg * H) /
    (float)H, w = 1.f - u` in mwf_apply_kernel), against the exact j / H and 1 - j / H.  H a power of two: both are exact, 0.
    Otherwise u carries one rounding, and w = fl(1 - u(1 + d)) is off by at most U (u + w) = U: relative to w = (H - j) / H
    that is H / (H - j), H at the most.  (The issue counted `u` and `1 - u` as one rounding each; the second is one rounding
    of w but inherits u's ABSOLUTE error, which is the line that was missed.)  With ``j`` (the frames' places in their
    segments) the count per frame, else the worst frame's."""
    if H == 0 or H & (H - 1) == 0:
        return 0 if j is None else np.zeros(len(j))
    return H if j is None else np.ceil(H / (H - np.asarray(j, f64)))


# k per launcher: fp32 roundings on the longest path in units of U, with the source lines they were counted from.  Measured on
# an MI355X (worst |error| / bound over the rows of mwf_cases.py; per row in mwf_cases.MEASURED): avsep_mwf_cov 0.111,
# avsep_mwf_cov_tv 0.111, avsep_mwf_apply 0.055, avsep_mwf_apply_tv 0.050.
K = {
    # mwf_cov_partial_kernel, one frame's term.  `sincosf(p[..], &sn, &cs)` FN on each of cs, sn; `re[c] = a * cs` 1: 5 on each
    # factor, 10 on a product; `im[r] * im[c]` rounded 1 and the `fmaf(re[r], re[c], ...)` 1 (imaginary part: two rounded
    # products and `-`, the same count): 12, on |re re| + |im im| <= |Y_r| |Y_c|
    "cov.term": 2 * (FN + 1) + 2,
    # TV: `acc[i] += w * x; accB[i] += u * x`: the product 1, and at a span that is no power of two the weight's own rounding 1
    # (`(float)j / fH` for u, the `1.f - u` for w).  What w inherits from u, U u |x| per frame, is counted per ENTRY by
    # cov_ref (``kw``): the sum of u |x| over the centre's own segment against the entry's absref, H at the most
    "cov.weight": lambda H: (1 + (k_weight(H) > 0)) if H else 0,
    # the longest chain of `acc[i] += ...` in one thread: `j += MWF_BLOCK` over a chunk of at most 2048 frames, or
    # `j += 64` over a segment of H frames
    "cov.chain": lambda F, H: cdiv(H, 64) if H else cdiv(min(F, CHUNK), BLOCK),
    # common.h wave_sum: `for (o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64)`
    "cov.butterfly": 6,
    # TV = false: `for (w = 1; w < MWF_WAVES; ++w) s += s_part[w][..]`
    "cov.waves": lambda H: 0 if H else WAVES - 1,
    # mwf_cov_finish_kernel `re += s[i]` once per chunk; mwf_cov_tv_finish_kernel `re += b[i]`: A + B
    "cov.finish": lambda F, H: 1 if H else chunks(F),
    # real and imaginary parts each within k U absref: the modulus within sqrt(2) k U absref
    "cov.complex": SQRT2,
    # the denominator's term `sq += a * a` C products and additions, `sq * (1.f / C)` the constant and the product
    "cov.v": lambda C: C + 2,
    # `o[0] = re / den`
    "cov.division": 1,
    # mwf_apply_kernel `sq += a * a; v[n] = sq * (1.f / C)` as above; `Sr[..] += v[n] * R(n, ..)` one product and N additions;
    # TV `w * Ra[..] + u * Rb[..]`: the weights, two products, one addition
    "apply.blend": lambda H, j=None: (k_weight(H, j) + 2) if H else 0,
    "apply.S": lambda C, N, H, j=None: (C + 2) + 1 + N + K["apply.blend"](H, j),
    # `tr += Sr[..]` C, `lam = reg * tr * (1.f / C) + FLT_MIN` 4, `Sr[..] += lam` 1
    "apply.lam": lambda C: C + 5,
    # Cholesky, forward and backward substitution: Higham, Accuracy and Stability, Theorem 10.4, gamma_{3C+1}; complex
    # arithmetic from real operations: 2 sqrt(2) (Lemma 3.5: a complex product is within sqrt(2) gamma_2)
    "apply.solve": lambda C: math.ceil(2 * SQRT2 * (3 * C + 1)),
    # `sincosf(xph[..])` FN, `zr[c] = a * cs` 1
    "apply.X": FN + 1,
    # `wr += rr * zr[c] - ri * zi[c]` two products, a difference, C additions; the blend again; `v[n] * wr` with v's own C + 2
    # and the product; both components: sqrt(2)
    "apply.Rz": lambda C, H, j=None: np.ceil(SQRT2 * ((C + 3) + K["apply.blend"](H, j) + (C + 2) + 1)),
    # `sqrtf(wr * wr + wi * wi)`: two products and a sum under a root 3 / 2 -> 1, sqrtf FN; `atan2f(wi, wr)` at 2 ulp of a
    # phase near pi, whose ulp is 2^-22 (§21): 2 * 2^-22 = 8 U of the complex value
    "apply.polar": 1 + FN + 8,
}


def k_cov(C, F, H=0):
    num = K["cov.term"] + K["cov.weight"](H) + K["cov.chain"](F, H) + K["cov.butterfly"] + K["cov.waves"](H) + K["cov.finish"](F, H)
    den = K["cov.v"](C) + K["cov.weight"](H) + K["cov.chain"](F, H) + K["cov.butterfly"] + K["cov.waves"](H) + K["cov.finish"](F, H)
    return math.ceil(K["cov.complex"] * num) + den + K["cov.division"]


def k_apply(C, N, H=0, F=None):
    """One constant, or with ``F`` one per frame [F] (they differ only where the span is no power of two: k_weight)."""
    j = None if F is None else np.arange(F) % max(H, 1)
    k = K["apply.S"](C, N, H, j) + K["apply.lam"](C) + K["apply.solve"](C) + K["apply.X"] + K["apply.Rz"](C, H, j) + K["apply.polar"]
    return int(k) if F is None else k + np.zeros(F)


def gamma(k):
    """k U: the bounds are first-order counts, as the issue states them (k U < 4e-5 here: the higher orders of (1 + U)^k
    are below 4e-5 of a bound the kernels use a tenth of)"""
    return k * U


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------
def cov_ref(ymag, yph, H=0):
    """-> (R complex128 [N,Fin,C,C] or [N,K,Fin,C,C], absref float64 of the same shape, v [N,Fin,F], kw).
    absref = sum_t w |Y_r| |Y_c| / max(sum_t w v, FLT_MIN).  kw is what an entry adds to k_cov at a span that is no power of
    two (0 otherwise): ceil(sqrt 2 * sum_seg u |Y_r| |Y_c| / sum_t w |Y_r| |Y_c|) + ceil(sum_seg u v / sum_t w v), the sums
    in the numerators over the centre's own segment (see K["cov.weight"])."""
    a = np.asarray(ymag).astype(f64)
    p = np.broadcast_to(np.asarray(yph).astype(f64), a.shape)
    C, F = a.shape[1], a.shape[3]
    Y = M.polar_to_complex(a, p)
    v = (a * a).sum(1) / f64(C)
    YY = np.einsum("ncft,ndft->nfcdt", Y, Y.conj())
    AA = np.einsum("ncft,ndft->nfcdt", a, a)
    if not H:
        den = np.maximum(v.sum(-1), FLT_MIN)[:, :, None, None]
        return YY.sum(-1) / den, AA.sum(-1) / den, v, 0.0
    Wt = T.hat_weights(F, H).T                                                   # [F,K]
    num = np.empty(YY.shape[:-1] + (Wt.shape[1],), np.complex128)
    num.real, num.imag = YY.real @ Wt, YY.imag @ Wt
    den = np.maximum(v @ Wt, FLT_MIN)[:, :, None, None, :]
    tr = (0, 4, 1, 2, 3)
    absn, kw = AA @ Wt, 0.0
    if k_weight(H):
        s, u = T.segments(F, H)
        Wb = np.zeros_like(Wt)
        Wb[np.arange(F), s] = u
        with np.errstate(invalid="ignore", divide="ignore"):
            rn = np.where(absn > 0, (AA @ Wb) / absn, 0.0)
            rd = np.where(v @ Wt > 0, (v @ Wb) / (v @ Wt), 0.0)
        kw = np.ascontiguousarray((np.ceil(SQRT2 * rn) + np.ceil(rd)[:, :, None, None, :]).transpose(tr))
    return np.ascontiguousarray((num / den).transpose(tr)), np.ascontiguousarray((absn / den).transpose(tr)), v, kw


def apply_ref(xmag, xph, ymag, cov, H=0, reg=M.REG):
    """Steps 3-5 in float64 on the fp32 covariance tensor ``cov`` (complex [N,Fin,C,C] or [N,K,Fin,C,C], cast exactly).
    -> {"Y" [N,C,Fin,F], "scale" [N,Fin,F] = (1 + kappa_2(S)) ||v_n R_n(f,t)||_2 ||z||_2, "kappa" [Fin,F], "v" [N,Fin,F],
    "small": the smallest non-zero magnitude among v, lam, the diagonal of S and ||z||}.  ``reg`` is what the kernel receives: a float."""
    a = np.asarray(ymag).astype(f64)
    X = M.polar_to_complex(xmag, xph)                                            # [C,Fin,F]
    C, F = X.shape[0], X.shape[2]
    v = (a * a).sum(1) / f64(C)
    R = np.asarray(cov).astype(np.complex128)
    if H:
        Rt = T.at_frames(R, F, H)                                                # [N,Fin,F,C,C]
        nrm = v * np.linalg.norm(Rt, 2, axis=(-2, -1))
    else:
        Rt = R[:, :, None]
        nrm = v * np.linalg.norm(R, 2, axis=(-2, -1))[:, :, None]
    A = v[..., None, None] * Rt
    S = A.sum(0)
    lam = f64(f32(reg)) * np.einsum("ftcc->ft", S).real / f64(C) + FLT_MIN
    S = S + lam[:, :, None, None] * np.eye(C)
    z = np.linalg.solve(S, X.transpose(1, 2, 0)[..., None])[..., 0]              # [Fin,F,C]
    W = np.where(v[:, None] == 0, 0, np.einsum("nftcd,ftd->ncft", A, z))
    ev = np.linalg.eigvalsh(S)
    kappa = ev[..., -1] / np.maximum(ev[..., 0], np.finfo(f64).tiny)
    scale = (1.0 + kappa)[None] * nrm * np.linalg.norm(z, axis=-1)[None]
    live = lam > FLT_MIN                                                         # a silent bin has S = FLT_MIN I by definition
    small = min(float(q[q > 0].min()) if (q > 0).any() else np.inf
                for q in (v, lam[live], np.einsum("ftcc->ftc", S).real[live], np.linalg.norm(z, axis=-1)))
    return {"Y": W, "scale": scale, "kappa": kappa, "v": v, "small": small}


# ---------------------------------------------------------------------------------------------------------------------
# gates: worst |error| / bound, and the number of elements whose bound is 0 and which are not exactly 0
# ---------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    zero = bound == 0
    r = np.divide(err, bound, out=np.zeros_like(err), where=~zero)
    return (float(r.max()) if r.size else 0.0), int((err[zero] != 0).sum())


def cov_gate(got, ref, absref, k, kw=0.0):
    return _ratio(np.abs(np.asarray(got).astype(np.complex128) - ref), gamma(k + kw) * absref)


def apply_gate(got, ref, k):
    """got: complex [N,C,Fin,F], the device's mag e^{i phase} evaluated in float64"""
    err = np.sqrt((np.abs(np.asarray(got) - ref["Y"]) ** 2).sum(1))
    return _ratio(err, gamma(k) * ref["scale"])


# ---------------------------------------------------------------------------------------------------------------------
# float32 controls and their mutants
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    1: "off-diagonal imaginary sign flipped",
    2: "triangle pair index taken as r C + c",
    3: "last frame of a 2048-frame chunk dropped",
    4: "TV: u formed with H + 1",
    5: "TV: last centre clamped to K - 2",
    6: "TV: A and B slabs swapped in the finish",
    7: "lam left out",
    8: "source n + 1's covariance read for source n with weight 1e-4",
    9: "channel 5 read for channel 6 at C = 7",
    10: "1e-5 of the peak added at a bin 80 dB down",
}
_XOR = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def _units(x, span, step):
    """x float32 [..., F] -> [..., units]: per unit of ``span`` frames, ``step`` threads' chains in ascending t, the xor
    butterfly of each wave of 64, the waves in ascending order."""
    F = x.shape[-1]
    n = cdiv(F, span)
    pad = np.zeros(x.shape[:-1] + (n * span,), f32)
    pad[..., :F] = x
    pad = pad.reshape(x.shape[:-1] + (n, span // step, step))
    acc = np.zeros(pad.shape[:-2] + (step,), f32)
    for i in range(span // step):
        acc = acc + pad[..., i, :]
    acc = acc.reshape(acc.shape[:-1] + (step // 64, 64))
    for idx in _XOR:
        acc = acc + acc[..., idx]
    out = acc[..., 0, 0]
    for w in range(1, step // 64):
        out = out + acc[..., w, 0]
    return out


def _weights32(F, H, mutant=None):
    j = (np.arange(F) % H).astype(f32)
    u = j / f32(H + 1 if mutant == 4 else H)
    return f32(1) - u, u


def _v32(a):
    sq = np.zeros(a.shape[:1] + a.shape[2:], f32)
    for c in range(a.shape[1]):
        sq = sq + a[:, c] * a[:, c]
    return sq * (f32(1) / f32(a.shape[1]))


def cov_control(ymag, yph, H=0, mutant=None):
    """float32, sums in the kernel's order -> complex64 [N,Fin,C,C] or [N,K,Fin,C,C]."""
    a = np.array(ymag, f32)
    p = np.array(np.broadcast_to(np.asarray(yph, f32), a.shape))
    N, C, Fin, F = a.shape
    if mutant == 9 and C == 7:
        a[:, 6], p[:, 6] = a[:, 5], p[:, 5]
    re, im = a * np.cos(p), a * np.sin(p)
    r, c = np.tril_indices(C)                                                    # row-major: pair r (r + 1) / 2 + c
    rr = (re[:, r].astype(f64) * re[:, c] + (im[:, r] * im[:, c]).astype(f64)).astype(f32)       # fmaf: [N,P,Fin,F]
    ii = im[:, r] * re[:, c] - re[:, r] * im[:, c]
    v = _v32(a)
    if not H:
        if mutant == 3:
            last = np.arange(CHUNK - 1, F, CHUNK)
            rr[..., last], ii[..., last], v[..., last] = 0, 0, 0
        tot = []
        for x in (rr, ii, v):
            part = _units(x, CHUNK, BLOCK)
            s = np.zeros(part.shape[:-1], f32)
            for k in range(part.shape[-1]):
                s = s + part[..., k]
            tot.append(s)
        sre, sim, den = (t[..., None] for t in tot)                                # [N,P,Fin,1], [N,Fin,1]
    else:
        w, u = _weights32(F, H, mutant)
        Kc, tot = T.centres(F, H), []
        for x in (rr, ii, v):
            A, B = _units(w * x, H, 64), _units(u * x, H, 64)
            if mutant == 6:
                A, B = B, A
            Ap, Bp = np.zeros(A.shape[:-1] + (Kc,), f32), np.zeros(A.shape[:-1] + (Kc,), f32)
            Ap[..., :min(A.shape[-1], Kc)] = A[..., :Kc]
            Bp[..., 1:] = B[..., :Kc - 1]
            tot.append(Ap + Bp)
        sre, sim, den = tot                                                      # [N,P,Fin,K], [N,Fin,K]
    den = np.maximum(den, f32(FLT_MIN))[:, None]
    qre, qim = sre / den, sim / den                                              # [N,P,Fin,K']
    out = np.zeros((N, sre.shape[-1], Fin, C, C), np.complex64)
    P = len(r)
    for i in range(C):
        for j in range(C):
            lo, hi = max(i, j), min(i, j)
            pi = (lo * C + hi) % P if mutant == 2 else lo * (lo + 1) // 2 + hi
            sgn = 0.0 if i == j else (1.0 if i > j else -1.0) * (-1.0 if mutant == 1 else 1.0)
            out[:, :, :, i, j] = (qre[:, pi] + 1j * sgn * qim[:, pi]).transpose(0, 2, 1)
    if mutant == 8:
        out[:-1] = out[:-1] + np.complex64(1e-4) * out[1:]
    return out if H else out[:, 0]


def apply_control(xmag, xph, ymag, cov, H=0, reg=M.REG, mutant=None):
    """float32 / complex64 NumPy (LAPACK solve), polar conversions at both ends -> (mag, phase) float32 [N,C,Fin,F]."""
    xm, xp, a = np.array(xmag, f32), np.array(xph, f32), np.array(ymag, f32)
    R = np.array(cov, np.complex64)
    N, C, Fin, F = a.shape
    if mutant == 9 and C == 7:
        xm[6], xp[6] = xm[5], xp[5]
    X = (xm * np.cos(xp) + 1j * (xm * np.sin(xp))).astype(np.complex64)
    v = _v32(a)
    if H:
        w, u = _weights32(F, H)
        s = np.arange(F) // H
        last = R.shape[1] - 1 - (1 if mutant == 5 and R.shape[1] >= 2 else 0)
        sa, sb = np.minimum(s, last), np.minimum(s + 1, last)
        Rt = (w[None, :, None, None, None] * R[:, sa] + u[None, :, None, None, None] * R[:, sb]).astype(np.complex64)
        Rt = np.ascontiguousarray(Rt.transpose(0, 2, 1, 3, 4))                   # [N,Fin,F,C,C]
    else:
        Rt = np.ascontiguousarray(np.broadcast_to(R[:, :, None], (N, Fin, F, C, C)))
    if mutant == 8:
        Rt = Rt.copy()
        Rt[:-1] = Rt[:-1] + np.complex64(1e-4) * Rt[1:]
    A = (v[..., None, None] * Rt).astype(np.complex64)
    S = np.zeros(A.shape[1:], np.complex64)
    for n in range(N):
        S = S + A[n]
    tr = np.einsum("ftcc->ft", S).real.astype(f32)
    lam = (f32(0) * tr if mutant == 7 else f32(reg) * tr * (f32(1) / f32(C))) + f32(FLT_MIN)
    S = (S + lam[:, :, None, None] * np.eye(C, dtype=f32)).astype(np.complex64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = np.linalg.solve(S, np.ascontiguousarray(X.transpose(1, 2, 0))[..., None])[..., 0]
        Wc = np.einsum("nftcd,ftd->ncft", A, z).astype(np.complex64)
    Wc = np.where(v[:, None] == 0, np.complex64(0), Wc)
    mag = np.sqrt(Wc.real * Wc.real + Wc.imag * Wc.imag).astype(f32)
    ph = np.arctan2(Wc.imag, Wc.real).astype(f32)
    ph[(Wc.real == 0) & (Wc.imag == 0)] = 0
    return mag, ph


def quiet_bin_error(Yref, got):
    """Mutant 10: ``got`` (complex [N,C,Fin,F]) with 1e-5 of max|Yref| added to the element whose reference magnitude is
    nearest to 1e-4 of the peak (80 dB down)."""
    peak = np.abs(Yref).max()
    mag = np.abs(Yref)
    idx = np.unravel_index(np.argmin(np.abs(np.log(np.maximum(mag, 1e-300) / (1e-4 * peak)))), mag.shape)
    out = np.array(got, np.complex128)
    out[idx] += 1e-5 * peak
    return out, float(mag[idx] / peak)
