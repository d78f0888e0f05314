"""Plain-torch restatement of cm_gan (consistency training with discriminators), test helper.

The seam (jg_cm_gan_head / jg_cm_gan_head_bwd), per element of sample b with the label mask m AS IS (None = 1):
  pred = cs_n x_n + co_n F_n,   targ = cs_c x_c + co_c F_c,   d = m pred - m targ,   c = 0.00054 sqrt(C H W),
  loss_cm = lam * mean( w_b (sqrt(d^2 + c^2) - c) ),   dFn_cm = grad_scale * lam * w_b / N * d / sqrt(d^2 + c^2) * m * co_n,
  dF_n = g * dFn_cm + co_n * dpred                     (g = d loss_G_tot / d loss_cm, dpred = the gradient through the discriminators)
and the model's generator loss  loss_G_tot = loss_cm + gan_lambda * sum_D loss_G(D(pred))  with pred NOT masked.
Everything here is float64 unless the caller's tensors say otherwise; `OracleCMGanTrainer` is the fp32 CPU oracle of the whole step."""
import math
from collections import OrderedDict

import torch

import jg_oracle as O

GAN_LAMBDA = 0.01


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cm_gan_loss(pred, target, mask, loss_weights, discriminators, lambda_G=1.0, gan_lambda=GAN_LAMBDA, fake=None):
    """(loss_G_tot, loss_G_cm, [loss_G_GAN per discriminator]) of compute_cm_gan_loss; `discriminators`: callables fake_B -> lsgan input;
    fake_B = pred unless `fake` is given (tests that cut or scale the gradient of the GAN branch).  Differentiable with respect to pred."""
    G_cm = O.cm_loss(pred, target, mask, loss_weights, lambda_G)
    gans = [gan_lambda * O.lsgan(D(pred if fake is None else fake), 1.0) for D in discriminators]
    tot = G_cm
    for v in gans:
        tot = tot + v
    return tot, G_cm.detach(), gans


def head_nhwc(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, w, lam=1.0, grad_scale=1.0):
    """what jg_cm_gan_head computes, in float64 on the kernel's own inputs: Fn, Fc [B,H,W,Cpad] (16-bit), noisy fp32 NCHW [B,C,H,W], the
    scalings and weights [B].  Returns (loss, pred [B,H,W,Cpad], dFn_cm [B,H,W,Cpad]), zero pad channels, all float64."""
    B, C, H, W = noisy_n.shape
    v = lambda t: t.double().reshape(B, 1, 1, 1)
    nchw = lambda F: F.double()[..., :C].permute(0, 3, 1, 2)
    pred = v(cs_n) * noisy_n.double() + v(co_n) * nchw(Fn)
    targ = v(cs_c) * noisy_c.double() + v(co_c) * nchw(Fc)
    m = 1.0 if mask is None else mask.double()
    d = m * pred - m * targ
    c = 0.00054 * math.sqrt(C * H * W)
    r = torch.sqrt(d * d + c * c)
    loss = (v(w) * (r - c)).mean() * lam
    dpred = lam * v(w) / d.numel() * d / r * m
    out_pred, dFn = torch.zeros(Fn.shape, dtype=torch.float64), torch.zeros(Fn.shape, dtype=torch.float64)
    out_pred[..., :C] = pred.permute(0, 2, 3, 1)
    dFn[..., :C] = (grad_scale * dpred * v(co_n)).permute(0, 2, 3, 1)
    return loss, out_pred, dFn


def head_bwd(dFn_cm, dpred, g, co_n, C):
    """what jg_cm_gan_head_bwd computes, float64: (dF, |g dFn_cm| + |co_n dpred|), zero pad channels"""
    B = dFn_cm.shape[0]
    a = float(g) * dFn_cm.double()
    b = torch.zeros_like(a) if dpred is None else co_n.double().reshape(B, 1, 1, 1) * dpred.double()
    out, mag = a + b, a.abs() + b.abs()
    out[..., C:] = 0
    mag[..., C:] = 0
    return out, mag


def cfg_of(c, task="inpainting"):
    return O.UNetCfg(in_channel=6 if task == "pix2pix" else 3, inner_channel=c["ngf"], out_channel=3, res_blocks=c["res_blocks"],
                     attn_res=c["attn_res"], channel_mults=c["mults"], efficient=c["efficient"], cond_embed_dim=256)


class OracleCMGanTrainer(O.OracleCMTrainer):
    """CMGanModel.optimize_parameters() with D_netDs = ["basic"], lsgan, iter_size 1: group G = the cm step of OracleCMTrainer with
    gan_lambda * lsgan(D(pred_x), 1) added to the loss (D's weights take no gradient), AdamW / Adam + EMA of G; group D = one draw from the
    history pool, (lsgan(D(real_B), 1) + lsgan(D(fake), 0)) / 2, its own optimizer of the same kind at lr_D."""

    def __init__(self, sdG, sdD, cfg, total_t, lr_G=1e-4, lr_D=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, ema_beta=0.999,
                 lambda_G=1.0, optim="adamw", gan_lambda=GAN_LAMBDA, n_layers=3, pool_size=50, pool_rng=None, task="inpainting"):
        super().__init__(sdG, cfg, total_t, lr=lr_G, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, ema_beta=ema_beta,
                         lambda_G=lambda_G, optim=optim)
        self.D = OrderedDict((k, v.detach().clone().float()) for k, v in sdD.items())
        self.mD = {k: torch.zeros_like(v) for k, v in self.D.items()}
        self.vD = {k: torch.zeros_like(v) for k, v in self.D.items()}
        self.stepD = 0
        self.hpD = dict(self.hp, lr=lr_D)
        self.gan_lambda, self.n_layers, self.task = gan_lambda, n_layers, task
        self.pool = O.OracleImagePool(pool_size, pool_rng)
        self.gan_scale = 1.0          # tests: 0 cuts the GAN term's gradient (its value stays in the loss)

    def g_loss_and_grads(self, y_0, mask, noise, timesteps, y_cond=None):
        P = OrderedDict()
        for k, v in self.P.items():
            P[k] = v.detach().clone().requires_grad_(True) if k in self.m else v
        if self.task == "pix2pix":
            mask = None
        out = O.cm_generator_forward(P, y_0, mask, noise, timesteps, self.current_t, self.total_t, self.cfg, x_cond=y_cond)
        self.current_t += y_0.shape[0]
        pred = out[0]
        fake = None if self.gan_scale == 1.0 else pred.detach() + self.gan_scale * (pred - pred.detach())
        tot, G_cm, (G_GAN,) = cm_gan_loss(pred, out[1], mask, out[4], [lambda x: O.nlayer_discriminator(self.D, x, self.n_layers)],
                                          self.lambda_G, self.gan_lambda, fake=fake)
        gs = getattr(self, "grad_scale", 1.0)      # static loss scale of the fp16 rounding yardstick (1: plain fp32 reference)
        (tot * gs).backward()
        grads = {k: (P[k].grad / gs if P[k].grad is not None else torch.zeros_like(P[k])) for k in self.train_names}
        losses = dict(G_tot=tot.detach(), G_cm=G_cm, G_GAN_D_B_basic=G_GAN.detach())
        return losses, grads, pred.detach()

    def d_loss_and_grads(self, real_B, fake):
        D = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in self.D.items())
        loss = (O.lsgan(O.nlayer_discriminator(D, real_B, self.n_layers), 1.0) + O.lsgan(O.nlayer_discriminator(D, fake, self.n_layers), 0.0)) * 0.5
        gs = getattr(self, "grad_scale", 1.0)
        keys = list(D)
        grads = dict(zip(keys, [g / gs for g in torch.autograd.grad(loss * gs, [D[k] for k in keys])]))
        return loss.detach(), grads

    def optimize_parameters(self, y_0, mask, noise, timesteps, y_cond=None):
        losses, grads, fake_B = self.g_loss_and_grads(y_0, mask, noise, timesteps, y_cond)
        self.step += 1
        names = self.train_names
        O.adamw_step([self.P[k] for k in names], [grads[k] for k in names], [self.m[k] for k in names], [self.v[k] for k in names],
                     self.step, decoupled=self.decoupled, **self.hp)
        if self.ema_beta is not None:
            if self.ema is None:
                self.ema = {k: self.P[k].clone() for k in self.param_names}
            O.ema_step([self.ema[k] for k in self.param_names], [self.P[k] for k in self.param_names], self.ema_beta)
        loss_D, gD = self.d_loss_and_grads(y_0, self.pool.query(fake_B))
        self.stepD += 1
        keys = list(self.D)
        O.adamw_step([self.D[k] for k in keys], [gD[k] for k in keys], [self.mD[k] for k in keys], [self.vD[k] for k in keys], self.stepD,
                     decoupled=self.decoupled, **self.hpD)
        losses.update(D_tot=loss_D, D_GAN_D_B_basic=loss_D)
        self.fake_B = fake_B
        return losses
