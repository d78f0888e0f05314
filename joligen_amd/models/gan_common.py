"""What the models with discriminators share (cut_model, cm_gan_model): the networks of gan_networks.define_D, their loss calculators
(base_gan_model.set_discriminators_info) and fused optimizers, the option checks and the loss-scale node of a GAN branch."""
from __future__ import annotations

import warnings

from .._autograd import JGFunction
from ..modules.discriminators import NLayerDiscriminator
from ..modules.loss import DiscriminatorGANLoss


class _ScaleGradFn(JGFunction):
    """identity on the loss value; multiplies the gradient by the static fp16 loss scale (1 for bf16)."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def check_discriminator_options(opt):
    """the D_netDs entries this build accepts.  Host-only (no device)."""
    bad = [d for d in opt.D_netDs if d not in ("basic", "projected_d")]
    if bad or not opt.D_netDs:
        raise NotImplementedError(f"D_netDs={opt.D_netDs!r}: 'basic' (PatchGAN) and 'projected_d' are built ('vision_aided' and the "
                                  "depth / mask / sam / temporal discriminators need pretrained networks)")


def check_d_diffusion_options(opt):
    """dataaug_D_diffusion (Diffusion-GAN noise on the projected discriminator's backbone features: gan_networks.py:416,
    base_gan_model.py:551-556, loss.py:315-331) as this build accepts it; returns True when a discriminator takes it.  Host-only (no device)."""
    if not hasattr(opt, "dataaug_D_diffusion_every"):
        opt.dataaug_D_diffusion_every = 4
    if not getattr(opt, "dataaug_D_diffusion", False):
        return False
    if "vit" in str(getattr(opt, "D_proj_network_type", "efficientnet")):      # options/train_options.py:776
        raise ValueError("ViT type projectors are not compatible with diffusion augmentation of the discriminator (dataaug_D_diffusion)")
    if int(opt.dataaug_D_diffusion_every) < 1:
        raise ValueError(f"dataaug_D_diffusion_every={opt.dataaug_D_diffusion_every!r}: >= 1 is required")
    if not any("projected" in d for d in opt.D_netDs):      # the reference hands the flag to projected discriminators only and says nothing
        warnings.warn(f"dataaug_D_diffusion has no effect: D_netDs={opt.D_netDs!r} holds no projected discriminator")
        return False
    return True


def define_discriminators(model, opt):
    """gan_networks.define_D (:330-446): one network per entry of D_netDs, set as `model.netD_B_<entry>`; returns the names D_B_<entry>"""
    names = []
    for d in opt.D_netDs:
        if d == "basic":
            # D_dropout reaches the PatchGAN only (cut_model.check_dropout_options; cm_gan refuses it)
            net = NLayerDiscriminator(opt.model_output_nc, opt.D_ndf, n_layers=opt.D_n_layers, use_dropout=bool(getattr(opt, "D_dropout", False)))
        else:
            from ..modules.projected_d import ProjectedDiscriminator

            # jg_projd_backbone: "lite0" (tf_efficientnet_lite0, the reference's feature network) | "standin" (tests);
            # jg_projd_pretrained: path of a timm tf_efficientnet_lite0 state_dict (the weights cannot be downloaded here)
            net = ProjectedDiscriminator(getattr(opt, "D_proj_network_type", "efficientnet"), interp=getattr(opt, "D_proj_interp", -1),
                                         # gan_networks.py:349,415: the discriminators see data_crop_size + the context margin
                                         img_size=opt.data_crop_size + 2 * int(getattr(opt, "data_online_context_pixels", 0) or 0), backbone=getattr(opt, "jg_projd_backbone", "lite0"),
                                         pretrained_path=getattr(opt, "jg_projd_pretrained", ""),
                                         diffusion_aug=bool(getattr(opt, "dataaug_D_diffusion", False)))
        setattr(model, "netD_B_" + d, net)
        names.append("D_B_" + d)
    return names


def define_D_optimizers(model, opt, kw):
    """the reference chains every discriminator's parameters into ONE Adam (cut_model.py:378-395); one fused optimizer per discriminator
    arena with the same hyper-parameters `kw` is the same update.  Sets `optimizer_<name>`, `<name>_loss_calculator` and
    `model.optimizer_D` (the first), appends to `model.optimizers` / `model.objects_to_update`; returns the optimizers' attribute names."""
    optD = []
    for dn in model.discriminators_names:
        o = model.make_optimizer(getattr(model, "net" + dn), **kw)
        setattr(model, "optimizer_" + dn, o)
        optD.append("optimizer_" + dn)
        model.optimizers.append(o)
        # base_gan_model.set_discriminators_info (:538-640): projected discriminators always train with the hinge objective
        mode = "projected" if "projected" in dn else opt.train_gan_mode
        calc = DiscriminatorGANLoss(getattr(model, "net" + dn), model.device, mode, opt.dataaug_D_label_smooth,
                                    dataaug_APA=getattr(opt, "dataaug_APA", False), dataaug_APA_p=getattr(opt, "dataaug_APA_p", 0.0),
                                    dataaug_APA_target=getattr(opt, "dataaug_APA_target", 0.6), train_batch_size=opt.train_batch_size,
                                    dataaug_APA_nimg=getattr(opt, "dataaug_APA_nimg", 50), dataaug_APA_every=getattr(opt, "dataaug_APA_every", 4),
                                    apa_stream=len(optD),      # Philox stream 1 + index: stream 0 is the noise's
                                    # base_gan_model.py:551-556: only a projected discriminator's calculator moves the diffusion strength
                                    dataaug_D_diffusion=bool(getattr(opt, "dataaug_D_diffusion", False)) and "projected" in dn,
                                    dataaug_D_diffusion_every=getattr(opt, "dataaug_D_diffusion_every", 4))
        setattr(model, dn + "_loss_calculator", calc)
        model.objects_to_update.append(calc)
    model.optimizer_D = getattr(model, optD[0])
    return optD
