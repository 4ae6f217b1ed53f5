"""Bottleneck audio-visual fusion on the HIP kernels (reference: models/fusion_net.py:7-311).

``get_fusion_net(mtype)`` keeps the reference's switch (``hidsep`` -> CoLoc, ``CoLoc_Sel``,
``MixVis``; anything else asserts).  Each class is parameter free.  ``run_forward`` /
``run_backward`` are what the U-Net autograd node calls; ``forward(x, v_ls)`` is the standalone
module interface ``(cat(tiles, x), (match_loss, att_maps))`` of the reference.
"""
import math

import torch
import torch.nn as nn

from .. import lib
from ..kernels import _ptr_array
from ..lib import ATT_BY_NAME as _ATT, call, ptr

_KIND = {"hidsep": 0, "CoLoc_Sel": 1, "MixVis": 2}


class _FusionBase(nn.Module):
    kind_name = "hidsep"

    def __init__(self, **kwargs):
        super().__init__()
        self.att_type = kwargs.get("att_type", "cos")
        if self.att_type not in _ATT:
            raise ValueError(f"att_type {self.att_type!r}")
        self.kind = _KIND[self.kind_name]
        self.ao_draws = None

    # ------------------------------------------------------------------ C > 2 sources (BASELINE.json configs[4])
    # BUILD-DEFINED generalisation, no reference counterpart (the reference hard-codes C = P = 2, fusion_net.py:35,43-46);
    # the rules are stated in DESIGN.md §9 and in csrc/fusion_n.hip (restated on the CPU by the test infrastructure):
    # Dc = D // C, the audio blocks are the first C*Dc pooled channels, the remainder's tile channels are zero (the fused
    # tensor keeps 2*D channels, so the U-Net's parameter shapes do not depend on C), all C! permutations in itertools
    # order, first maximum wins.  One launch forward, one backward (avsep_fusion_n_*), like the two-source kernels.
    num_src = 2
    _ptr_array = staticmethod(_ptr_array)

    def _run_forward_n(self, x, vs, draws):
        B, D, Fq, T = x.shape
        C = len(vs) if vs else self.num_src
        dev = x.device
        out = {"n": C, "feat": torch.empty((B, D), dtype=torch.float32, device=dev),
               "pool_idx": torch.empty((B, D), dtype=torch.int32, device=dev)}
        if not vs:
            out["draws"] = draws.to(device=dev, dtype=torch.int32).contiguous()
            call("avsep_fusion_n_ao_fwd", ptr(x), ptr(out["draws"]), B, C, D, Fq * T, ptr(out["feat"]), ptr(out["pool_idx"]))
            return out
        Dc = D // C
        if any(v.shape[1] != Dc for v in vs):
            raise lib.AvsepError(f"visual channels {vs[0].shape[1]} != bottleneck // {C} = {Dc}")
        H, W = vs[0].shape[-2:]
        out.update(a_pool=torch.empty((B, D), dtype=torch.float32, device=dev),
                   sel_idx=torch.empty((B, D), dtype=torch.int32, device=dev),
                   att_maps=torch.empty((B, C, H, W), dtype=torch.float32, device=dev),
                   match_part=torch.empty((B,), dtype=torch.float32, device=dev),
                   best=torch.empty((B,), dtype=torch.int32, device=dev), HW=H * W)
        call("avsep_fusion_n_av_fwd", ptr(x), self._ptr_array(vs), B, C, D, Fq * T, H * W, _ATT[self.att_type],
             ptr(out["a_pool"]), ptr(out["pool_idx"]), ptr(out["feat"]), ptr(out["sel_idx"]), ptr(out["att_maps"]),
             ptr(out["match_part"]), ptr(out["best"]))
        return out

    def _run_backward_n(self, x, vs, fus, dfeat, dx_accum, dmatch):
        B, D, Fq, T = x.shape
        C = fus["n"]
        if not vs:
            call("avsep_fusion_n_ao_bwd", ptr(fus["draws"]), B, C, D, Fq * T, ptr(fus["pool_idx"]), ptr(dfeat), ptr(dx_accum))
            return []
        dvs = [torch.empty_like(v) for v in vs]
        dm = dmatch.reshape(1).contiguous().float() if dmatch is not None else None
        call("avsep_fusion_n_av_bwd", ptr(x), self._ptr_array(vs), B, C, D, Fq * T, fus["HW"], _ATT[self.att_type],
             ptr(fus["a_pool"]), ptr(fus["pool_idx"]), ptr(fus["sel_idx"]), ptr(fus["best"]), ptr(dfeat), ptr(dm),
             1.0 / B if dm is not None else 0.0, ptr(dx_accum), self._ptr_array(dvs))
        return dvs

    # ------------------------------------------------------------------ kernels
    def run_forward(self, x, vs, draws):
        """x [B,D,F,T] bottleneck; vs list of visual maps or [] for audio-only."""
        if len(vs) > 2 or (not vs and self.num_src > 2):
            if self.kind != 0:
                raise NotImplementedError("only CoLoc (hidsep) is generalised beyond two sources")
            return self._run_forward_n(x, vs, draws)
        B, D, Fq, T = x.shape
        Dc, FT = D // 2, Fq * T
        dev = x.device
        out = {"feat": torch.empty((B, D), dtype=torch.float32, device=dev),
               "pool_idx": torch.empty((B, D), dtype=torch.int32, device=dev)}
        if not vs:
            d8 = draws.to(torch.uint8)
            all_zero = int(int(d8.max()) == 0)  # one_hot width quirk, fusion_net.py:96 (draws live on the host)
            out["draws"], out["all_zero"] = d8.to(dev), all_zero
            call("avsep_fusion_ao_fwd", ptr(x), ptr(out["draws"]), all_zero, B, Dc, FT, ptr(out["feat"]),
                 ptr(out["pool_idx"]))
            return out
        if self.kind == 2:
            assert len(vs) == 1                      # fusion_net.py:287: one mixed visual map
            vs = [vs[0], vs[0]]
        elif len(vs) != 2:
            raise AssertionError("CoLoc fusion takes one visual map per source (C = 2)")
        H, W = vs[0].shape[-2:]
        HW = H * W
        if vs[0].shape[1] != Dc:
            raise lib.AvsepError(f"visual channels {vs[0].shape[1]} != bottleneck/2 = {Dc}")
        out.update(a_pool=torch.empty((B, D), dtype=torch.float32, device=dev),
                   sel_idx=torch.empty((B, D), dtype=torch.int32, device=dev),
                   att_maps=torch.empty((B, 2, H, W), dtype=torch.float32, device=dev),
                   match_part=torch.empty((B,), dtype=torch.float32, device=dev),
                   best=torch.empty((B,), dtype=torch.int32, device=dev), HW=HW)
        call("avsep_fusion_av_fwd", ptr(x), ptr(vs[0]), ptr(vs[1]), B, Dc, FT, HW, self.kind, _ATT[self.att_type],
             ptr(out["a_pool"]), ptr(out["pool_idx"]), ptr(out["feat"]), ptr(out["sel_idx"]), ptr(out["att_maps"]),
             ptr(out["match_part"]), ptr(out["best"]))
        return out

    def run_backward(self, x, vs, fus, dfeat, dx_accum, _unused, dmatch):
        """Adds the gradient wrt x into dx_accum; returns the visual-map gradients."""
        if "n" in fus:
            return self._run_backward_n(x, vs, fus, dfeat, dx_accum, dmatch)
        B, D, Fq, T = x.shape
        Dc, FT = D // 2, Fq * T
        if not vs:
            call("avsep_fusion_ao_bwd", ptr(fus["draws"]), fus["all_zero"], B, Dc, FT, ptr(fus["pool_idx"]),
                 ptr(dfeat), ptr(dx_accum))
            return []
        dvs = [torch.empty_like(v) for v in vs]
        v1, dv1 = (vs[0], None) if self.kind == 2 else (vs[1], dvs[1])
        dm = None
        if dmatch is not None:
            dm = dmatch.reshape(1).contiguous().float()
        call("avsep_fusion_av_bwd", ptr(x), ptr(vs[0]), ptr(v1), B, Dc, FT, fus["HW"], self.kind,
             _ATT[self.att_type], ptr(fus["a_pool"]), ptr(fus["pool_idx"]), ptr(fus["sel_idx"]),
             ptr(fus["att_maps"]), ptr(fus["best"]), ptr(dfeat), None, ptr(dm), 1.0 / B if dm is not None else 0.0,
             ptr(dx_accum), ptr(dvs[0]), ptr(dv1))
        return dvs

    def draw(self, B):
        """The audio-only random draw: the reference's swap coin (fusion_net.py:94) for two sources, a uniformly random
        permutation index for more."""
        if self.num_src > 2:
            return torch.randint(0, math.factorial(self.num_src), (B,))
        return torch.rand(B) > 0.5

    # ------------------------------------------------------------------ module interface
    def forward(self, x, v_ls, option=None):
        if option is not None:
            raise NotImplementedError("option='duet' is unreachable from Unet in the reference")
        lib.require_gpu(x)
        if v_ls is None:
            B = x.shape[0]
            draws = self.ao_draws if self.ao_draws is not None else self.draw(B)
            y, _m = _FusionFn.apply(self, draws, 0, x.contiguous())
            return y, (None, None)
        vs = [v.contiguous().float() for v in v_ls]
        y, match, att = _FusionFn.apply(self, None, len(vs), x.contiguous(), *vs)
        return y, (match, att)


class _FusionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, draws, nv, x, *vs):
        vs = list(vs)
        fus = mod.run_forward(x, vs, draws)
        B, D, Fq, T = x.shape
        tiles = fus["feat"].reshape(B, D, 1, 1).expand(B, D, Fq, T)
        y = torch.cat([tiles, x], 1)
        ctx.mod, ctx.fus, ctx.nv = mod, fus, nv
        ctx.save_for_backward(x, *vs)
        if not nv:
            return y, x.new_zeros(())
        ctx.mark_non_differentiable(fus["att_maps"])
        return y, fus["match_part"].mean(), fus["att_maps"]

    @staticmethod
    def backward(ctx, dy, dmatch, *_):
        x, *vs = ctx.saved_tensors
        B, D = x.shape[:2]
        dy = dy.contiguous()
        dfeat = dy[:, :D].sum(dim=(2, 3)).contiguous()
        dx = dy[:, D:].contiguous().clone()
        dvs = ctx.mod.run_backward(x, list(vs), ctx.fus, dfeat, dx, None, dmatch if ctx.nv else None)
        return (None, None, None, dx, *dvs)


class CoLoc(_FusionBase):
    kind_name = "hidsep"


class CoLoc_Sel(_FusionBase):
    kind_name = "CoLoc_Sel"


class MixVis(_FusionBase):
    kind_name = "MixVis"


def get_fusion_net(mtype):
    if mtype == "hidsep":
        return CoLoc
    elif mtype == "CoLoc_Sel":
        return CoLoc_Sel
    elif mtype == "MixVis":
        return MixVis
    else:
        assert False
