"""GAN objectives of the CUT path on the HIP ops: /root/reference/models/modules/loss.py `GANLoss` (:11-85) for
gan_mode='lsgan' (the train_gan_mode default: MSE against 1 / 0), 'vanilla' (BCE with logits), 'wgangp' (-/+ mean; the reference never
adds its gradient penalty) and 'projected' (the hinge objective :77-84 that
`set_discriminators_info` forces for projected discriminators, base_gan_model.py:544-545), and `DiscriminatorGANLoss` (:249-313)
with adaptive pseudo augmentation (APA, `DiscriminatorLoss` :199-246) and the update of the D-diffusion augmentation (:315-331).
lsgan predictions are NHWC logit maps whose channel 0 is valid (PatchGAN output padded to 8 channels); projected predictions are the
concatenated logits [B, N] of the mini-discriminators (every element valid)."""
from __future__ import annotations

import torch.nn as nn

import os

import torch

from .. import ops

BATCH_REAL_FAKE = os.environ.get("JG_D_BATCH_REAL_FAKE", "1") != "0"


class GANLoss(nn.Module):
    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        if gan_mode not in ("lsgan", "vanilla", "wgangp", "projected"):
            raise NotImplementedError("gan mode %s not implemented" % gan_mode)
        self.gan_mode = gan_mode
        self.real_label, self.fake_label = float(target_real_label), float(target_fake_label)

    def __call__(self, prediction, target_is_real, relu=True):
        """loss.py:59-85: lsgan: nn.MSELoss()(prediction, label.expand_as(prediction)); projected: hinge (`relu`) / -mean (generator)."""
        if self.gan_mode == "projected":
            from .projected_d import hinge_loss

            return hinge_loss(prediction, target_is_real, relu)
        if self.gan_mode == "wgangp":       # :72-76: the sign is the label, whatever real_label / fake_label are
            return ops.gan_loss(prediction, "wgangp", 1.0 if target_is_real else 0.0)
        return ops.gan_loss(prediction, self.gan_mode, self.real_label if target_is_real else self.fake_label)


class DiscriminatorGANLoss(nn.Module):
    """loss.py:249-313 (`compute_loss_D` :288-307, `compute_loss_G` :309-313)."""

    def __init__(self, netD, device, train_gan_mode="lsgan", dataaug_D_label_smooth=False, dataaug_APA=False,
                 dataaug_D_diffusion=False, dataaug_APA_p=0.0, dataaug_APA_target=0.6, train_batch_size=1, dataaug_APA_nimg=50,
                 dataaug_APA_every=4, apa_stream=1, dataaug_D_diffusion_every=4):
        super().__init__()
        self.dataaug_D_diffusion, self.dataaug_D_diffusion_every = bool(dataaug_D_diffusion), int(dataaug_D_diffusion_every or 0)
        if self.dataaug_D_diffusion:
            # loss.py:328-331 reaches into netD.freeze_feature_network.diffusion: only the convolutional projected discriminator built with
            # diffusion_aug has one
            if getattr(getattr(netD, "freeze_feature_network", None), "diffusion", None) is None:
                raise NotImplementedError("the D-diffusion augmentation needs an EfficientNet projected discriminator built with diffusion_aug")
            if self.dataaug_D_diffusion_every < 1:
                raise ValueError(f"dataaug_D_diffusion_every={dataaug_D_diffusion_every!r}: >= 1 is required")
        self.netD, self.device = netD, device
        self.gan_mode = train_gan_mode
        self.criterionGAN = GANLoss(train_gan_mode, target_real_label=0.9 if dataaug_D_label_smooth else 1.0)
        self.dataaug_APA, self.dataaug_APA_target = bool(dataaug_APA), float(dataaug_APA_target)
        self.train_batch_size, self.dataaug_APA_nimg, self.dataaug_APA_every = int(train_batch_size), dataaug_APA_nimg, int(dataaug_APA_every)
        # APA: (p, adjust, s) live on the device -- the substitution reads p there and `update` rewrites it there, so a step never waits
        # for the host.  p is not part of a checkpoint (as in the reference: a plain attribute of the loss calculator)
        self.apa_state = torch.tensor([float(dataaug_APA_p), 0.0, 0.0], device=device, dtype=torch.float32) if self.dataaug_APA else None
        self.apa_stream = int(apa_stream)      # Philox stream id of this discriminator's flags (jg_d_aug)
        self.apa_u = None                      # parity runs: the fp32 [B] uniforms of the next substitution (else drawn in the kernel)
        self.apa_flags = None                  # int32 [B]: the samples the last substitution replaced
        self.pred_real = None

    # loss.py:189-190,336-337: read by get_current_APA_prob through float(); the views below cost no host read until someone asks
    @property
    def adaptive_pseudo_augmentation_p(self):
        return self.apa_state[0] if self.dataaug_APA else 0.0

    @property
    def adjust(self):
        return self.apa_state[1] if self.dataaug_APA else 0

    def adaptive_pseudo_augmentation(self, real, fake):
        """loss.py:199-212: real[b] replaced by fake[b] where rand() < p; the reference's blend with 0 / 1 flags is this select for finite
        inputs, and its "no flag set: return real" shortcut has the same value"""
        (out,), flags = ops.d_aug(real, real.shape[-1], alts=[fake], ps=[self.apa_state[0:1]], us=None if self.apa_u is None else [self.apa_u],
                                  streams=[self.apa_stream], key=None if self.apa_u is not None else ops.d_aug_key(real.device))
        self.apa_flags = flags[0]
        return out

    def compute_loss_D(self, netD, real, fake, fake_2=None):
        """`fake_2` (APA): the batch the flagged samples of `real` are taken from; None: `real` is used as given (the model has formed the
        real operands of all its discriminators in one launch)"""
        if self.dataaug_APA and fake_2 is not None:
            real = self.adaptive_pseudo_augmentation(real, fake_2)
        self.real, self.fake = real, fake
        if BATCH_REAL_FAKE and getattr(netD, "per_sample", False) and real.shape == fake.shape and real.dtype == fake.dtype:
            # round 6: a discriminator that is a per-sample function with no state tied to the call (no BatchNorm statistics, no spectral-norm
            # power iteration: the ViT projector with its MLP heads) sees real and fake as ONE batch -- half the launches of the
            # discriminator half, GEMMs of twice the rows; the two losses are taken on the halves of the logits (loss.py:288-307 calls
            # netD twice; same function, the weight gradients of the heads are summed inside one GEMM instead of over two)
            n = real.shape[0]
            pred = netD(torch.cat((self.real, self.fake.detach()), dim=0))
            self.pred_real = pred[:n]
            self.loss_D_real = self.criterionGAN(self.pred_real, True)
            return (self.loss_D_real + self.criterionGAN(pred[n:], False)) * 0.5
        self.pred_real = netD(self.real)
        self.loss_D_real = self.criterionGAN(self.pred_real, True)
        pred_fake = netD(self.fake.detach())
        loss_D_fake = self.criterionGAN(pred_fake, False)
        return (self.loss_D_real + loss_D_fake) * 0.5

    def compute_loss_G(self, netD, real, fake):
        self.real, self.fake = real, fake
        return self.criterionGAN(netD(self.fake), True, relu=False)

    def update(self, niter):
        """loss.py:214-231,244-246: one launch on the prediction of the (substituted) real batch; nothing is read on the host"""
        if self.dataaug_APA and niter % self.dataaug_APA_every < self.train_batch_size:
            ops.apa_update(self.pred_real, self.apa_state, self.dataaug_APA_target, self.train_batch_size * self.dataaug_APA_every,
                           self.dataaug_APA_nimg * 1000, channel0=self.gan_mode != "projected")
        if self.dataaug_D_diffusion and niter % self.dataaug_D_diffusion_every < self.train_batch_size:
            # loss.py:315-331: p moves with sign(loss_D_real - 0.9), then update_T; one launch on the device scalar, no host read
            self.netD.freeze_feature_network.diffusion.update(self.loss_D_real, self.train_batch_size * self.dataaug_D_diffusion_every)
