"""gpu: every launcher of csrc/mwf.hip against float64, per entry and per bin.  The rows of mwf_cases.py reach
all 32 instantiations of mwf_cov_partial_kernel<C, TV> / mwf_apply_kernel<C, TV> and both finishing kernels; each row calls
kernels._mwf_cov and kernels._mwf_apply directly and gates them one at a time:
  * covariances: |cov - ref| <= k_cov 2^-24 absref per entry, float64 on the same fp32 inputs;
  * images: ||Y'_n(f,t) - ref||_2 <= k_apply 2^-24 (1 + kappa_2(S)) ||v_n R_n||_2 ||z||_2 per source and bin, the float64
    steps 3-5 fed the covariance tensor the device produced, cast exactly.
The constants are counted in mwf_gates_ref.K; test_mwf_gates_host.py shows on the CPU that float32 controls pass these gates
and ten mutants do not.  Nothing is excluded from either gate.  Run with -s for the worst |error| / bound per launcher and
row (recorded in mwf_cases.MEASURED)."""
import numpy as np
import pytest
import torch

import avsep_amd as P

import mwf_cases as Cs
import mwf_gates_ref as G
import mwf_ref as M
import mwf_tv_ref as T

pytestmark = pytest.mark.gpu

K = P.kernels


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("rid", sorted(Cs.ROWS))
def test_launchers_against_float64(dev, rid):
    r, x = Cs.row(rid), Cs.inputs(rid)
    H, C, N, F, reg = r["H"], r["C"], r["N"], r["F"], r["reg"]
    xmag, xph, ymag, yph = x["xmag"], x["xph"], x["ymag"], x["yph"]
    xm, xp, ym, yp = (_dev(a, dev) for a in (xmag, xph, ymag, yph))
    # -- the covariance launcher ------------------------------------------------------------------------------------------
    cov = K._mwf_cov(ym, yp, H)
    assert cov.dtype == torch.float32 and cov.shape == ((N, T.centres(F, H), Cs.FIN, C, C, 2) if H else (N, Cs.FIN, C, C, 2))
    assert torch.equal(K._mwf_cov(ym, yp, H), cov)                                  # fixed summation order: the same bits
    c = cov.cpu().numpy()
    re, im = c[..., 0], c[..., 1]
    ref_c, absref, v, kw = G.cov_ref(ymag, yph, H)
    rc, zc = G.cov_gate(re.astype(np.float64) + 1j * im.astype(np.float64), ref_c, absref, G.k_cov(C, F, H), kw)
    assert np.isfinite(c).all()
    assert (np.diagonal(im, axis1=-2, axis2=-1) == 0).all()                         # a real diagonal
    assert np.array_equal(re, np.swapaxes(re, -1, -2)) and (im == -np.swapaxes(im, -1, -2)).all()    # bitwise Hermitian
    # -- the apply launcher, on the covariances the device produced -------------------------------------------------------
    mag, ph = K._mwf_apply(xm, xp, ym, cov, H, reg)
    mag2, ph2 = K._mwf_apply(xm, xp, ym, cov, H, reg)
    assert torch.equal(mag, mag2) and torch.equal(ph, ph2)
    assert mag.shape == ph.shape == (N, C, Cs.FIN, F) and mag.dtype == ph.dtype == torch.float32
    mag, ph = mag.cpu().numpy(), ph.cpu().numpy()
    ref = G.apply_ref(xmag, xph, ymag, re.astype(np.float64) + 1j * im.astype(np.float64), H, reg)
    ra, za = G.apply_gate(M.polar_to_complex(mag, ph), ref, G.k_apply(C, N, H, F))
    print(f"{rid} H={H} C={C} N={N} F={F} {r['kind']}: cov {rc:.3g} of its bound, apply {ra:.3g} (kappa <= {ref['kappa'].max():.3g}); "
          f"{zc} + {za} elements that must be exactly 0 are not")
    assert np.isfinite(mag).all() and np.isfinite(ph).all() and (mag >= 0).all() and (np.abs(ph) <= np.float32(np.pi)).all()
    silent = np.broadcast_to(v[:, None] == 0, mag.shape)
    assert (mag[silent] == 0).all() and (ph[silent] == 0).all()
    assert zc == 0 and rc <= 1
    assert za == 0 and ra <= 1
    if reg == 0.0:
        assert ref["kappa"].max() < 1e3
    a, b = Cs.silent_run(F, H)
    if H and F > 2 * H:                                                             # silent over centre 1's whole support
        assert (c[N - 1, 1] == 0).all() and (mag[N - 1, :, :, a:b] == 0).all()
    if rid in ("L01", "L03"):
        off = np.arange(N) != Cs.LEAK_SOURCE
        assert (c[off] == 0).all() and (mag[off] == 0).all() and (ph[off] == 0).all() and np.abs(c[Cs.LEAK_SOURCE]).max() > 0.1
    if rid in ("L02", "L04"):
        q = Cs.LEAK_CHANNEL
        assert (c[..., q, :, :] == 0).all() and (c[..., :, q, :] == 0).all() and (mag[:, q] == 0).all() and (ph[:, q] == 0).all()
        assert np.abs(mag).max() > 1.0

