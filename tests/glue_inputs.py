"""Operands of the glue-kernel sweep (tests/glue_cases.py), built on the CPU from a seed that is a function of the row alone, so
that the host test and the GPU test see the same tensors.  A plain module: no test lives here."""
import zlib

import torch

import convref as R
import glue_cases as S
import glueref as G


def gen(row, salt=""):
    return torch.Generator().manual_seed(zlib.crc32(f"{row[0]}-{S.case_id(row)}-{salt}".encode()))


def randn(g, *shape):
    return torch.randn(shape, generator=g)


def chan(g, c, signed=True):
    """A per-channel row of magnitude 0.5 .. 1.5 (and random sign)."""
    v = 0.5 + torch.rand((c,), generator=g)
    if signed:
        v = v * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()
    return v


def is_b16(row):
    return row[1].startswith("b16_")


def act_input(g, row):
    """An activation-like tensor of the row's shape, at bf16 values for a B16 kernel."""
    x = randn(g, *row[2])
    return R.bf16(x) if is_b16(row) else x


def pool_operands(row, act):
    """(x, scale, shift) of a pooling row: x fp32 NCHW (bf16 values for the B16 kernel)."""
    g = gen(row, f"pool{act}")
    Cc = row[2][1]
    return act_input(g, row), chan(g, Cc), 0.3 * randn(g, Cc)


def decidable(y, row, scale, shift, res=None, res_scale=None, res_shift=None):
    """y with every element whose activation mask is undecidable moved by 1 (see glueref.make_decidable)."""
    y, moved = G.make_decidable(y, lambda t: G.pre_act(t, scale, shift, res, res_scale, res_shift),
                                R.bf16 if is_b16(row) else None)
    return y
