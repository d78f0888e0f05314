"""cm_gan_model (consistency training with discriminators) on MI355X: mirror of the reference's models/cm_gan_model.py (`__init__` :15-91,
`compute_G_loss` :93-96, `compute_cm_gan_loss` :98-106) on top of cm_model, with base_gan_model.py's `compute_G_loss_GAN` (:421-503) and
`compute_D_loss(_generic)` (:341-419) for D_netDs in {'basic', 'projected_d'}.

Per iteration (reference order): group G = {G_A}: the two UNet passes of cm_model; loss_G_cm = compute_cm_loss; fake_B = pred_x = the
student's full prediction c_skip x_noisy + c_out F_next (not masked, not blended with the ground truth); loss_G_tot = loss_G_cm +
alg_gan_lambda * sum_D loss_G(D(fake_B)) with alg_gan_lambda FORCED to 0.01 (:22); backward; AdamW step and EMA of G_A.  Group D: every
discriminator draws its own fake batch from the history pool, loss_D_tot = sum_D loss_D(D(real_B), D(fake)); backward; step of every D.

The seam between the two halves is one fused kernel each way (`ops.cm_gan_head`): forward = the consistency loss, its gradient and
`pred` as the discriminators' 16-bit NHWC input in one pass over the UNet outputs; backward = g_loss * dFn_cm + c_out * dpred in one pass.
`fake_B` is that NHWC tensor during training (NCHW fp32 after `inference`, as in cm_model); the reference's extra visual groups
(real_A / fake_B / real_B) are not published.  The D step does not depend on the generator's backward and runs after it here."""
from __future__ import annotations

import torch

from .. import ops
from ..options import CM_GAN_DEFAULTS
from ..util.image_pool import ImagePool
from .base_model import NetworkGroup
from .cm_model import CMModel
from .gan_common import _ScaleGradFn, check_discriminator_options, define_D_optimizers, define_discriminators

GAN_LAMBDA = 0.01          # cm_gan_model.py:22: set in __init__ whatever the config says


def check_cm_gan_options(opt):
    """the options of cm_gan this build accepts; fills the defaults a bare namespace lacks, forces alg_gan_lambda and returns the
    discriminators' names (D_B_<entry> in the order of D_netDs).  Host-only (no device)."""
    for k, v in CM_GAN_DEFAULTS.items():
        if not hasattr(opt, k):
            setattr(opt, k, v)
    if getattr(opt, "alg_ddpm_ft_mode", "cm") == "ect":
        raise NotImplementedError("alg_ddpm_ft_mode='ect' with model_type='cm_gan': the reference cannot run it either -- compute_cm_gan_loss "
                                  "always calls compute_cm_loss, which unpacks 7 values from a generator that returns 6 in that mode")
    check_discriminator_options(opt)
    for flag in ("dataaug_APA", "dataaug_D_diffusion", "train_semantic_mask", "train_semantic_cls", "train_mask_out_mask",
                 "train_temporal_criterion"):
        if getattr(opt, flag, False):
            raise NotImplementedError(f"{flag} is outside the SURVEY.md 8 hot path")
    if opt.dataaug_D_noise > 0:
        raise NotImplementedError("dataaug_D_noise: noisy-D terms are outside the built path")
    if int(getattr(opt, "data_online_context_pixels", 0) or 0) > 0:      # the fused head (ops.cm_gan_head) hands the discriminators the crop: no frame
        raise NotImplementedError("data_online_context_pixels > 0 with model_type='cm_gan': the seam kernel has no context frame (cut_model has)")
    for name, built in (("D_dropout", False), ("D_spectral", False), ("D_norm", "instance")):
        if getattr(opt, name, built) != built:
            raise NotImplementedError(f"{name}={getattr(opt, name)!r}: only {built!r} is built for the PatchGAN")
    if getattr(opt, "model_output_nc", 3) > 8:
        raise NotImplementedError("model_output_nc > 8: the fused head moves one 8-channel vector per pixel")
    opt.alg_gan_lambda = GAN_LAMBDA
    return ["D_B_" + d for d in opt.D_netDs]


def cm_gan_loss_names(discriminators_names):
    """(loss_names_G, loss_names_D) in the reference's order (cm_gan_model.py:76-89).  Host-only (no device)."""
    return (["G_tot", "G_cm"] + ["G_GAN_" + dn for dn in discriminators_names],
            ["D_tot"] + ["D_GAN_" + dn for dn in discriminators_names])


class CMGanModel(CMModel):
    overlap_exchange = False

    def __init__(self, opt, rank):
        names = check_cm_gan_options(opt)
        super().__init__(opt, rank)
        self.loss_functions_G = ["compute_G_loss_GAN"]
        if not opt.isTrain:
            return
        if self.act_dtype == torch.float16 and not float(getattr(opt, "jg_loss_scale", 0.0) or 0.0):
            # as in cut_model: the gradient through the discriminators is orders larger than the diffusion path's, 65536 overflows fp16
            # activation gradients, 1024 keeps both ends of the range; poll_overflow stays in charge afterwards
            self.loss_scale = 1024.0
            for o in self.optimizers:
                o.grad_scale = 1.0 / self.loss_scale
        self.discriminators_names = define_discriminators(self, opt)
        assert self.discriminators_names == names
        self.model_names += self.discriminators_names
        self.fake_B_pool = ImagePool(opt.train_pool_size)      # forward_GAN is never called: the real pools are never touched
        kw = dict(lr=opt.train_D_lr, betas=(opt.train_beta1, opt.train_beta2), weight_decay=opt.train_optim_weight_decay,
                  eps=opt.train_optim_eps)
        optD = define_D_optimizers(self, opt, kw)
        self.group_G.backward_functions = ["compute_cm_gan_loss"]
        self.group_D = NetworkGroup(networks_to_optimize=list(self.discriminators_names), forward_functions=None,
                                    backward_functions=["compute_D_loss"], loss_names_list=["loss_names_D"], optimizer=optD,
                                    loss_backward=["loss_D_tot"])
        self.networks_groups.append(self.group_D)
        self.loss_names_G, self.loss_names_D = cm_gan_loss_names(self.discriminators_names)
        self.loss_names = self.loss_names_G + self.loss_names_D
        self.iter_calculator_init()

    def parallelize(self, rank):
        raise NotImplementedError("model_type='cm_gan' on more than one GPU: data parallelism of the discriminator half is not built yet")

    def set_pool_rng(self, rng):
        """parity runs: the host RNG (uniform / randint) of the fake pool, like the reference's `random` module"""
        self.fake_B_pool.rng = rng

    def set_input(self, data):
        super().set_input(data)
        if self.opt.isTrain:
            self.real_B_nhwc = ops.to_nhwc(self.gt_image.float(), self.act_dtype, 8)

    # cm_gan_model.py:98-106
    def compute_cm_gan_loss(self):
        net = self._net("G_A")
        noise = timesteps = None
        if self.rng_injection is not None:
            noise, timesteps = self.rng_injection(self.gt_image.shape[0])
        r = net.forward_nhwc(self.gt_image, self.total_t, self.mask, self.cond_image, noise, timesteps)
        self.next_noisy_x, self.current_noisy_x = r["next_noisy_x"], r["current_noisy_x"]
        self.loss_G_tot, pred = ops.cm_gan_head(r["F_next"], r["F_cur"], r["next_noisy_x"], r["current_noisy_x"], r["cs_n"], r["co_n"],
                                                r["cs_c"], r["co_c"], self.mask, r["loss_weights"],
                                                lam=self.opt.alg_diffusion_lambda_G, grad_scale=self.loss_scale)
        self.loss_G_cm = self.loss_G_tot.detach().clone()
        self.fake_B = pred
        self.compute_G_loss()

    # cm_gan_model.py:93-96: loss_G_tot is NOT reset
    def compute_G_loss(self):
        for f in self.loss_functions_G:
            getattr(self, f)()

    def compute_G_loss_GAN(self):
        """base_gan_model.py:421-503: alg_gan_lambda * compute_loss_G of every discriminator on fake_B; the static loss scale enters this
        branch's gradient here (the cm branch carries it as `grad_scale`)"""
        gan = 0
        for dn in self.discriminators_names:
            val = self.opt.alg_gan_lambda * getattr(self, dn + "_loss_calculator").compute_loss_G(self._net(dn), self.real_B_nhwc, self.fake_B)
            setattr(self, "loss_G_GAN_" + dn, val)
            gan = gan + val
        self.loss_G_tot = self.loss_G_tot + _ScaleGradFn.apply(gan, self.loss_scale)

    def compute_D_loss(self):
        """base_gan_model.py:341-419: every discriminator draws ITS OWN fake batch from the history pool"""
        tot = 0
        for dn in self.discriminators_names:
            fake = self.fake_B_pool.query(self.fake_B)
            val = getattr(self, dn + "_loss_calculator").compute_loss_D(self._net(dn), self.real_B_nhwc, fake, None)
            setattr(self, "loss_D_GAN_" + dn, val)
            tot = tot + val
        self.loss_D_tot = _ScaleGradFn.apply(tot, self.loss_scale)
