"""The case list of tests/conv_variant_cases.py against the stored dispatch table and the library (host code only: the library
loads without a device and no query dereferences a pointer)."""
import ctypes

import pytest
import torch

import conv_variant_cases as V
import convref as R

CASES = V.cases()
# dgrad_act's operand conditions are checked here, through convref on the CPU, for the cases of at most this many
# multiply-accumulates; the larger ones (ACT_ON_GPU_ONLY, asserted below to be exactly those) are checked by
# tests/test_gpu_conv_variants.py alone, which asserts the same two conditions for every dgrad_act call it makes
ACT_CPU_MACS = 300_000_000
ACT_CASES = [c for c in CASES if c.mode == "dgrad" and c.dgrad_act_fused]
ACT_ON_GPU_ONLY = ["dgrad-f32-wino4_kernel:8x8x8,sub"]


def _variant(L, d, mode, with_stats):
    buf = ctypes.create_string_buffer(128)
    assert L.avsep_conv_kernel_variant(ctypes.byref(d), mode, int(with_stats), buf, 128) == 0
    return buf.value.decode()


def test_cases_equal_the_triples_of_the_stored_table():
    have = {(c.mode, c.variant, c.prec) for c in CASES}
    want = V.table_triples()
    assert have == want, ("triples without a case", sorted(want - have), "cases without a triple", sorted(have - want))
    assert len(CASES) == len(have)
    print(f"{len(CASES)} cases = {len(want)} (mode, variant, precision) triples of the stored table")


def test_library_takes_every_case_to_its_variant():
    import avsep_amd as P
    L = P.lib.load()
    wrong = []
    for c in CASES:
        d = c.desc()
        now = {"fwd_stats": _variant(L, d, 0, True), "fwd": _variant(L, d, 0, False), "dgrad": _variant(L, d, 1, False),
               "wgrad": _variant(L, d, 2, False)}
        want = {k: v for k, v in c.expect.items() if v is not None}        # a supplement case knows its own route only
        if {k: now[k] for k in want} != want:
            wrong.append((c, now))
        assert c.variant in (([want["fwd_stats"], want["fwd"]] if "fwd" in want else [want["fwd_stats"]]) if c.mode == "fwd"
                             else [want[c.mode]]), c
        assert (L.avsep_conv2d_dgrad_act_fused(ctypes.byref(d)), L.avsep_conv2d_head_applicable(ctypes.byref(d))) == \
            (c.dgrad_act_fused, c.head), c
    assert not wrong, wrong


def test_caps():
    for c in CASES:
        assert c.macs == c.N * c.Cin * c.Cout * c.Ho * c.Wo * c.KH * c.KW <= V.MAX_MACS == 3_000_000_000, c
        assert c.tensor_bytes <= V.MAX_TENSOR_BYTES == 64 << 20, c
        assert c.plan_n == 0 or c.plan_n == c.N * c.plan_batch_scale != c.N, c     # reachable through kernels.plan_batch_scale
    assert not V.SUPPLEMENT or all(k in {(c.mode, c.variant, c.prec) for c in CASES} for k in V.SUPPLEMENT)


def test_operands_are_deterministic():
    c = next(c for c in CASES if c.geo_name == "smallco.plain")
    a, b = V.operands(c), V.operands(c)
    assert all(torch.equal(a[k], b[k]) for k in a if a[k] is not None)
    assert a["w"].shape == (c.Cout, c.Cin, c.KH, c.KW) and a["dy"].shape == (c.N, c.Cout, c.Ho, c.Wo)


def test_which_dgrad_act_cases_are_checked_on_the_gpu_only():
    assert ACT_CASES, "no fused dgrad_act descriptor among the cases"
    assert sorted(c.id for c in ACT_CASES if c.macs > ACT_CPU_MACS) == sorted(ACT_ON_GPU_ONLY)


@pytest.mark.parametrize("case", [c for c in ACT_CASES if c.macs <= ACT_CPU_MACS], ids=lambda c: c.id)
def test_dgrad_act_operands_exclude_nothing(case):
    c = case
    geo = R.Geometry(c.N, c.Cin, c.H, c.W, c.Cout, c.k, c.stride, c.pad, c.dil, C0=c.C0, act0=c.act0, act1=c.act1, up2x=c.up2x)
    op = V.operands(c)
    a = V.act_operands(c)
    ref = R.reference(geo, "dgrad_act", dict(a, w=op["w"], dy=op["dy"], act=R.ACT_RELU, bstats=True, bf16=False))
    assert ref["excluded"] is not None and int(ref["excluded"].sum()) == 0
    dx, absref = ref["dx"]
    assert dx.shape == (c.N, c.Cin, c.H, c.W) and bool((absref > 0).all())
    passed = float(((dx - a["add"].double()) != 0).double().mean())
    assert 0.25 < passed < 0.75, ("the ReLU mask passes about half of the elements", passed)
    assert bool((ref["bstats"][1] > 0).all())
