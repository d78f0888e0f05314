"""PatchGAN discriminator on the HIP ops: mirror of /root/reference/models/modules/discriminators.py
(`NLayerDiscriminator` :10-118) for InstanceNorm (affine=False -> conv bias=True), no spectral norm / wavelets.
Same nn.Sequential indices as the reference (`model.0.weight` ... `model.11.bias`; with `use_dropout` an nn.Dropout(0.5) placeholder follows
every LeakyReLU and the later layers move up, as in the reference: modules/dropout.py).  The 4x4 stride-2 convolutions run on the
generic MFMA implicit-GEMM kernel; their input gradients as stride-1 convolutions over the zero-dilated output gradient;
InstanceNorm + LeakyReLU(0.2) is one fused normalisation pass.  The 1-channel logit map is stored with 8 channels (7 zero)."""
from __future__ import annotations

import torch.nn as nn

from .. import ops
from ..ops import JG_ACT_LRELU, JG_ACT_NONE
from .dropout import DropoutOwner, DropoutState, FusedDropout, bind_dropout
from .layers import JGConv2d


class NLayerDiscriminator(DropoutOwner, nn.Module):
    def __init__(self, input_nc, ndf=64, n_layers=3, use_dropout=False, use_spectral=False, freq_space=False):
        super().__init__()
        if use_spectral or freq_space:
            raise NotImplementedError("spectral norm / wavelet input of the PatchGAN are outside the built path")
        kw, padw = 4, 1
        drop = lambda: [FusedDropout(0.5)] if use_dropout else []
        seq = [JGConv2d(input_nc, ndf, kw, padding=padw, stride=2), nn.LeakyReLU(0.2, True)] + drop()
        nf_mult = 1
        for n in range(1, n_layers):
            nf_prev, nf_mult = nf_mult, min(2 ** n, 8)
            seq += [JGConv2d(ndf * nf_prev, ndf * nf_mult, kw, padding=padw, stride=2), nn.InstanceNorm2d(ndf * nf_mult),
                    nn.LeakyReLU(0.2, True)] + drop()
        nf_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        seq += [JGConv2d(ndf * nf_prev, ndf * nf_mult, kw, padding=padw, stride=1), nn.InstanceNorm2d(ndf * nf_mult),
                nn.LeakyReLU(0.2, True)] + drop()
        seq += [JGConv2d(ndf * nf_mult, 1, kw, padding=padw, stride=1)]
        self.model = nn.Sequential(*seq)
        self.arena = None
        self.dropout_state = DropoutState()       # the step's Philox key and invocation counts; `dropout_rand` injects uniforms (DropoutOwner)
        bind_dropout(self, self.dropout_state)

    def jg_finalize(self, device, act_dtype):
        from ..arena import ParamArena

        if self.arena is None:
            self.act_dtype = act_dtype
            self.arena = ParamArena(self, device, act_dtype, priority=())
        return self.arena

    def forward(self, x):
        """x: [B,H,W,8] 16-bit NHWC (image channels zero-padded) -> logits [B,H',W',8] (channel 0 valid)."""
        if self.arena is not None:
            self.arena.ensure_fresh()
        mods = list(self.model)
        # the placeholder behind the activation at index j, in training mode: [InstanceNorm, LeakyReLU, Dropout] and [LeakyReLU, Dropout] are one pass
        drop_at = lambda j: mods[j + 1] if j + 1 < len(mods) and isinstance(mods[j + 1], FusedDropout) and mods[j + 1].training else None
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, JGConv2d):
                x = m(x)
            elif isinstance(m, nn.InstanceNorm2d):
                fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.LeakyReLU)
                drop = drop_at(i + 1) if fuse else None
                if drop is not None:
                    x = ops.group_norm(x, x.shape[-1], None, None, None, JG_ACT_LRELU, m.eps, **drop.args(x))
                    i += 2
                else:
                    x = ops.group_norm(x, x.shape[-1], None, None, None, JG_ACT_LRELU if fuse else JG_ACT_NONE, m.eps)
                    i += 1 if fuse else 0
            elif isinstance(m, nn.LeakyReLU):
                drop = drop_at(i)
                if drop is not None:
                    x = ops.activation_dropout(x, JG_ACT_LRELU, **drop.args(x))
                    i += 1
                else:
                    x = ops.activation(x, JG_ACT_LRELU)
            elif isinstance(m, FusedDropout):       # eval(): the identity
                pass
            else:
                raise NotImplementedError(type(m))
            i += 1
        return x
