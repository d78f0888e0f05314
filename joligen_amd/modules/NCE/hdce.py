"""SRC_hDCE contrastive criterion on the fused HIP kernel: /root/reference/models/modules/NCE/hDCE.py (`PatchHDCELoss`) with the
weights of NCE/SRC.py (`SRC_Loss.forward` :46-75, `only_weight` part) computed inside the kernel from the key Gram matrix -- the reference
hands them over as a [B, P, P] tensor, here they never reach memory.  `weighted=False` is the reference's `weight=None` call (the identity
term).  Both classes of the reference split the batch, one by `train_batch_size` and one by `current_batch`; `current_batch` is used for
both.  The diagonal mask is eye(P) (the reference builds eye(feature width), which equals it wherever the reference runs at all).
Returns the per-patch loss vector like the reference."""
from __future__ import annotations

import torch.nn as nn

from ... import ops


class PatchHDCELoss(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        if not float(opt.alg_cut_HDCE_gamma) > 0.0:
            raise ValueError(f"alg_cut_HDCE_gamma={opt.alg_cut_HDCE_gamma!r}: the hDCE weights are exp(similarity / gamma), gamma must be > 0")

    def forward(self, feat_q, feat_k, current_batch, weighted=True, **unused_args):
        nimg = 1 if self.opt.alg_cut_nce_includes_all_negatives_from_minibatch else current_batch
        return ops.patch_hdce_loss(feat_q, feat_k, nimg, self.opt.alg_cut_nce_T, self.opt.alg_cut_HDCE_gamma, 1, 1 if weighted else 0)
