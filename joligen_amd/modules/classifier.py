"""Image classifier of the semantic-consistency branch on the HIP ops: mirror of the reference's models/modules/classifiers.py
(`Classifier` :12-54, built by semantic_networks.define_C :19-42 for train_sem_cls_template 'basic' and initialised by init_net).
Same nn.Sequential indices as the reference (`before_linear.0.weight`, `before_linear.3.running_mean`, ..., `after_linear.1.bias`), so
`latest_net_CLS.pth` loads strictly both ways.

log2(size) - 1 unpadded 3x3 stride-2 convolutions take the image to a 1x1 map (128: 63, 31, 15, 7, 3, 1); all but the first and the last
are followed by BatchNorm2d(affine) + LeakyReLU(0.2) (one fused normalisation pass over the batch statistics, which also updates the running
ones), the first and the last by LeakyReLU alone; then Linear(C, 1024) and Linear(1024, nclasses) with no activation between, in fp32.
The convolutions run on the generic MFMA implicit-GEMM kernel; the input gradient of the first one onto the 8-channel image takes the gather
form, the others the stride-1 convolution over the zero-dilated output gradient -- for an even input size the last row and column belong to
no window and come out exactly zero.  With the parameters' requires_grad off (the generator's step) the backward launches no weight-gradient
kernel and leaves the gradient arena untouched."""
from __future__ import annotations

import math

import torch.nn as nn

from .. import ops, ops_segformer
from ..ops import JG_ACT_LRELU
from .layers import JGConv2d


class Classifier(nn.Module):
    def __init__(self, input_nc, ndf, nclasses, img_size, init_type="normal", init_gain=0.02):
        super().__init__()
        log_size = int(math.log(img_size, 2))
        if img_size < 8 or 2 ** log_size != img_size:      # the reference reaches no 1x1 map and fails in its first Linear
            raise ValueError(f"Classifier: img_size={img_size!r} must be a power of two >= 8")
        if ndf % 8:
            raise NotImplementedError(f"Classifier: ndf={ndf!r} must be a multiple of 8 (channel granularity of the 16-bit maps)")
        if init_type != "normal":
            raise NotImplementedError("only init_type='normal' (the reference default) is built")
        kw = 3
        seq = [JGConv2d(input_nc, ndf, kw, stride=2), nn.LeakyReLU(0.2, True)]
        nf_mult = 1
        last = log_size - 3
        for n in range(log_size - 2):
            nf_prev, nf_mult = nf_mult, min(2 ** n, 8)
            seq += [JGConv2d(ndf * nf_prev, ndf * nf_mult, kw, stride=2)]
            if n != last:
                seq += [nn.BatchNorm2d(ndf * nf_mult, affine=True)]
            seq += [nn.LeakyReLU(0.2, True)]
        self.before_linear = nn.Sequential(*seq)
        self.after_linear = nn.Sequential(nn.Linear(ndf * nf_mult, 1024), nn.Linear(1024, nclasses))
        self.img_size, self.nclasses = img_size, nclasses
        self.arena = None
        # models/modules/utils.py:33-71 init_net 'normal': conv / linear weights ~ N(0, gain), biases 0, BatchNorm weight ~ N(1, gain)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.normal_(m.weight, 0.0, init_gain)
                nn.init.constant_(m.bias, 0.0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.normal_(m.weight, 1.0, init_gain)
                nn.init.constant_(m.bias, 0.0)

    def jg_finalize(self, device, act_dtype):
        from ..arena import ParamArena

        if self.arena is None:
            self.act_dtype = act_dtype
            self.arena = ParamArena(self, device, act_dtype, priority=())
        return self.arena

    def forward(self, x):
        """x: [B, S, S, 8] 16-bit NHWC (image channels zero-padded) -> logits fp32 [B, nclasses]"""
        if x.shape[1] != self.img_size or x.shape[2] != self.img_size:
            raise ValueError(f"Classifier built for {self.img_size} x {self.img_size} images, got {tuple(x.shape)}")
        if self.arena is not None:
            self.arena.ensure_fresh()
        mods = list(self.before_linear)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, JGConv2d):
                x = m(x)
            elif isinstance(m, nn.BatchNorm2d):      # always followed by the LeakyReLU: fused into the apply pass
                x = ops_segformer.batch_norm(x, m, JG_ACT_LRELU)
                i += 1
            else:
                x = ops.activation(x, JG_ACT_LRELU)
            i += 1
        x = x.reshape(x.shape[0], -1).float()
        for lin in self.after_linear:
            x = ops.linear(x, lin.weight, lin.bias)
        return x
