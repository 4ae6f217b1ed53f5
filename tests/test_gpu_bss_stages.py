"""gpu: the three entry points of csrc/bss_windows.hip one stage at a time, each on inputs of its own (tests/bss_cases.py, pinned
on the CPU by test_bss_stages_host.py) against tests/bss_stage_ref.py: every lagged correlation within 1e-11 of its sum of
absolute products, every solved system (general block-Toeplitz matrices that make the LU swap rows in nearly every column)
against a long-double elimination next to numpy.linalg.solve's own error, every one of the eight energy sums of every range
against long double at 1e-11 relative; the singular paths, and the independence of the systems and ranges of one call.
Each test counts what it compared: the count must be the full size of the output."""
import numpy as np
import pytest
import torch

import bss_cases as BC
import bss_stage_ref as BR

pytestmark = pytest.mark.gpu
CORR_TOL = 1e-11              # of sum |a| |b|: the project's bound for this stage (n * 2^-53 = 4.5e-13 at the largest n here, 4097)
SOLVE_MARGIN = 16.0           # the kernel and LAPACK are both LU with partial pivoting: their errors are two draws from one bound
EN_TOL = 1e-11                # relative, per sum (n * 2^-53 = 7e-12 at 66004 samples; the reference's own float64 error is <= 1e-13)


def _pkg():
    import avsep_amd as P
    return P


def _rows(x, guard, dev):
    """The rows on the device; with `guard`, as the middle rows of a buffer whose first and last rows hold bss_cases.GUARD."""
    if not guard:
        return torch.from_numpy(x).to(dev)
    return torch.from_numpy(BC.guarded(x)).to(dev)[1:x.shape[0] + 1]


# ---- 1. correlations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.CORR_CASES, ids=BC.case_id)
def test_every_correlation_against_its_sum_of_absolute_products(dev, case):
    from avsep_amd import bss_eval as PB
    Pn, L, flen, starts, n, guard = case
    s, e, ref = BC.corr_inputs(case)
    rr, er = _rows(s, guard, dev), _rows(e, guard, dev)
    assert rr.is_contiguous() and rr.shape == (Pn, L)
    R, D = PB.seg_corr(rr, er, flen, list(starts), n)
    assert R.shape == (len(starts), Pn, Pn, 2 * flen - 1) and D.shape == (len(starts), Pn, Pn, flen)
    count, worst, empty = 0, 0.0, 0
    for i, (Rn, Dn, aR, aD) in enumerate(ref):
        for what, got, want, scale in (("R", R[i].cpu().numpy(), Rn, aR),
                                       ("D", D[i].cpu().numpy(), Dn.transpose(1, 0, 2), aD.transpose(1, 0, 2))):
            d = np.abs(got - want)
            some = scale > 0
            assert (d[~some] == 0).all() and (got[~some] == 0).all(), f"{what} of segment {i}: an empty sum is exactly zero"
            ratio = d[some] / scale[some]
            worst, empty = max(worst, float(ratio.max())), empty + int((~some).sum())
            assert (d <= CORR_TOL * scale).all(), f"{what} of segment {i}: max |d| / sum|a||b| = {ratio.max():.3e} > {CORR_TOL}"
            count += d.size
    print(f"{case}: max |d| / sum|a||b| = {worst:.3e} over {count} correlations ({empty} of them empty sums)")
    assert count == R.numel() + D.numel()
    # R[s, p, q, tau] and R[s, q, p, -tau] are one sum, written twice
    assert torch.equal(R, R.transpose(1, 2).flip(3)), "R[p][q][tau] and R[q][p][-tau] are the same bits"
    assert R.transpose(1, 2).flip(3).numel() == R.numel()


# ---- 2 - 5. solves ------------------------------------------------------------------------------------------------------------
def _solve(dev, R, D, G):
    """avsep_bss_solve_groups by lib.call (bss_eval.solve_groups replaces a singular system's zeros by a host solve and keeps
    info to itself): -> C [systems, M, G], info [systems]; both prefilled with what the kernel never writes."""
    P = _pkg()
    R, D = R.contiguous(), D.contiguous()
    nseg, Pn, NL = R.shape[0], R.shape[1], R.shape[3]
    flen, nsys = (NL + 1) // 2, nseg * (Pn // G)
    nbytes = P.lib.load().avsep_bss_solve_groups_workspace_bytes(nseg, Pn, G, flen)
    assert nbytes == 8 * nsys * (G * flen) ** 2
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    C = torch.full((nsys, G * flen, G), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((nsys,), -7, dtype=torch.int32, device=dev)
    P.lib.call("avsep_bss_solve_groups", P.lib.ptr(R), P.lib.ptr(D), nseg, Pn, G, flen, P.lib.ptr(ws), nbytes, P.lib.ptr(C), P.lib.ptr(info))
    return C, info


def _case_on(dev, case):
    R, D = BC.solve_inputs(case)
    return torch.from_numpy(R).to(dev), torch.from_numpy(D).to(dev)


@pytest.mark.parametrize("case", BC.SMALL_SOLVES, ids=BC.case_id)
def test_solved_systems_against_long_double_next_to_numpy(dev, case):
    """Per system max |x - x_ld| / max |x_ld| of the kernel and of numpy.linalg.solve on the same matrix: the kernel's is at
    most 16 times numpy's (or 16 * 2^-52 where numpy's is smaller).  A wrong swap is an error of order 1."""
    nseg, Pn, G, flen, _ = case
    C, info = _solve(dev, *_case_on(dev, case), G)
    assert info.tolist() == [0] * len(info)
    got = C.cpu().numpy()
    count = 0
    for sys, ref in enumerate(BC.solved_systems(case)):
        x, swaps, zero = ref["ld"]
        scale = np.abs(x).max()
        err = float(np.abs(got[sys] - x).max() / scale)
        err_np = float(np.abs(ref["np"] - x).max() / scale)
        print(f"{case} system {sys}: M = {G * flen}, {swaps} swaps, kernel {err:.3e}, numpy {err_np:.3e}")
        assert err <= SOLVE_MARGIN * max(err_np, 2.0 ** -52), (sys, err, err_np)
        count += got[sys].size
    assert count == C.numel() == nseg * Pn * flen * G


@pytest.mark.parametrize("case", BC.LARGE_SOLVES, ids=BC.case_id)
def test_large_systems_by_their_backward_error(dev, case):
    """|| A x - b || / (|| A || || x || + || b ||) in long double, of the kernel's solution against numpy.linalg.solve's."""
    nseg, Pn, G, flen, _ = case
    C, info = _solve(dev, *_case_on(dev, case), G)
    assert info.tolist() == [0] * len(info)
    got = C.cpu().numpy()
    count = 0
    for sys, ref in enumerate(BC.solved_systems(case)):
        assert np.isfinite(got[sys]).all()
        be, be_np = BR.backward_error(ref["A"], got[sys], ref["b"]), BR.backward_error(ref["A"], ref["np"], ref["b"])
        print(f"{case} system {sys}: M = {G * flen}, backward error kernel {be:.3e}, numpy {be_np:.3e}")
        assert be <= SOLVE_MARGIN * be_np, (sys, be, be_np)
        count += got[sys].size
    assert count == C.numel() == nseg * Pn * flen * G


def test_systems_of_one_call_are_independent(dev):
    """Each of the six systems, solved in a call of its own (one segment, its group's blocks of R and D as a P = G problem),
    has the bits it has in the joint call."""
    case = BC.SOLVE_CASES[2]
    nseg, Pn, G, flen, _ = case
    R, D = _case_on(dev, case)
    C, info = _solve(dev, R, D, G)
    assert info.tolist() == [0] * 6 and torch.isfinite(C).all()
    count = 0
    for sys in range(6):
        seg, base = sys // (Pn // G), (sys % (Pn // G)) * G
        one, info1 = _solve(dev, R[seg:seg + 1, base:base + G, base:base + G], D[seg:seg + 1, base:base + G, base:base + G], G)
        assert info1.tolist() == [0] and one.shape == (1, G * flen, G)
        assert torch.equal(one[0], C[sys]), f"system {sys} alone and among the six"
        count += one.numel()
    assert count == C.numel()


def test_singular_systems_report_their_pivot_and_leave_the_others_alone(dev):
    """Block row and block column i of one system's R zeroed: info is the long-double elimination's first zero-pivot column
    plus 1, the filters are zeros and the other system's bits are unchanged.  A system of NaNs: info 1 and zeros."""
    nseg, Pn, G, flen = 2, 3, 3, 4
    rs = np.random.RandomState(77)
    R, D = rs.randn(nseg, Pn, Pn, 2 * flen - 1), rs.randn(nseg, Pn, Pn, flen)
    Rt, Dt = torch.from_numpy(R).to(dev), torch.from_numpy(D).to(dev)
    C0, info0 = _solve(dev, Rt, Dt, G)
    assert info0.tolist() == [0, 0] and torch.isfinite(C0).all()
    count = 0
    for w, i in ((1, 1), (0, 0), (0, 2), (1, None)):
        R2 = R.copy()
        if i is None:
            R2[w] = np.nan
        else:
            R2[w, i, :, :] = 0.0
            R2[w, :, i, :] = 0.0
        A, b = BC.system(R2, D, Pn, G, flen, w)
        x, swaps, zero = BR.solve_ld(A, b)
        assert zero == (0 if i is None else i * flen), "the zero pivot the case is made for"
        C, info = _solve(dev, torch.from_numpy(R2).to(dev), Dt, G)
        assert info[w].item() == zero + 1 and info[1 - w].item() == 0, (w, i, info.tolist(), zero)
        assert (C[w] == 0).all(), "a singular system's filters are written as zeros"
        assert torch.equal(C[1 - w], C0[1 - w]), "the other system of the call has not changed a bit"
        count += C.numel()
    assert count == 4 * nseg * G * flen * G


# ---- 6. energies --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.EN_CASES, ids=lambda c: c[0])
def test_every_energy_sum_against_long_double(dev, case):
    from avsep_amd import bss_eval as PB
    name, S, C, flen, L, starts, n, ranges, rlen, guard = case
    s, e, C_all, C_own, terms = BC.en_inputs(case)
    rr, er = _rows(s, guard, dev), _rows(e, guard, dev)
    Ca, Co = torch.from_numpy(C_all).to(dev), torch.from_numpy(C_own).to(dev)
    segs, offs = [seg for seg, _ in ranges], [off for _, off in ranges]
    sums = PB.window_energies(rr, er, C, flen, list(starts), n, Ca, Co, segs, offs, rlen)
    assert sums.shape == (len(ranges), S, 8)
    got, ld = sums.cpu().numpy().astype(np.longdouble), terms["ld"]
    d = np.abs(got - ld)
    some = ld > 0
    rel = (d[some] / ld[some]).astype(np.float64)
    print(f"{name}: max relative error of an energy sum = {rel.max():.3e} over {d.size} sums ({int((~some).sum())} of them exactly zero)")
    assert (d <= EN_TOL * ld).all(), (name, rel.max(), np.argwhere(d > EN_TOL * ld)[:8].tolist())
    assert d.size == len(ranges) * S * 8 == sums.numel()
    valid = [i for i, seg in enumerate(segs) if 0 <= seg < len(starts)]
    invalid = [i for i in range(len(ranges)) if i not in valid]
    assert (sums[invalid] == 0).all(), "a range of a segment that does not exist is eight exact zeros"
    if invalid:
        # the valid ranges alone: the same bits
        alone = PB.window_energies(rr, er, C, flen, list(starts), n, Ca, Co, [segs[i] for i in valid], [offs[i] for i in valid], rlen)
        assert alone.shape == (len(valid), S, 8) and torch.equal(alone, sums[valid])
    else:
        assert name != "invalid"
