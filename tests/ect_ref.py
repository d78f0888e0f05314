"""Plain-torch restatement of easy consistency tuning (cm_model with alg_ddpm_ft_mode = "ect"), test helper.

Per sample b, with pred = D_yt (student, carries the gradient), targ = D_yr (teacher), the label mask m AS IS (None = 1), dt = t - r:
  d = m pred - m targ,   S_b = sum_{c,h,w} d^2,   loss = lam * mean_b( (sqrt(S_b + c^2) - c) / dt_b ),
  d loss / d pred = lam / B * d / (sqrt(S_b + c^2) dt_b) * m
Everything here is float64 unless the caller's tensors say otherwise; `OracleECTTrainer` is the fp32 CPU oracle of the whole step."""
from collections import OrderedDict

import torch

import jg_oracle as O

ECT_C = 1e-6
P_MEAN, P_STD, K, B_, Q = -1.1, 2.0, 8.0, 1.0, 2.0


def t_to_r(t, stage=0):
    return torch.clamp(t * (1 - (1 / Q ** (stage + 1)) * (1 + K * torch.sigmoid(-B_ * t))), min=0)


def skip_train(sigma, sigma_data=O.CM_SIGMA_DATA):
    return sigma_data ** 2 / (sigma ** 2 + sigma_data ** 2)


def out_train(sigma, sigma_data=O.CM_SIGMA_DATA):
    return (sigma_data * sigma) / (sigma_data ** 2 + sigma ** 2) ** 0.5


def ect_loss(pred, targ, mask, dt, c=ECT_C, lam=1.0):
    """the scalar, differentiable with respect to pred"""
    if mask is not None:
        pred, targ = mask * pred, mask * targ
    S = ((pred - targ) ** 2).reshape(pred.shape[0], -1).sum(-1)
    return ((torch.sqrt(S + c ** 2) - c) / dt.flatten()).mean() * lam


def ect_grad(pred, targ, mask, dt, c=ECT_C, lam=1.0):
    """d ect_loss / d pred in closed form"""
    B = pred.shape[0]
    m = 1.0 if mask is None else mask.to(pred.dtype)
    d = m * pred - m * targ
    S = (d ** 2).reshape(B, -1).sum(-1)
    return lam / B * d / (torch.sqrt(S + c ** 2) * dt.flatten()).view(B, 1, 1, 1) * m


def ect_loss_nhwc(Fn, Fc, noisy_n, noisy_c, cs_n, co_n, cs_c, co_c, mask, dt, c=ECT_C, lam=1.0, grad_scale=1.0):
    """what jg_ect_loss computes, in float64 on the kernel's own inputs: Fn, Fc [B,H,W,Cpad] (16-bit), noisy fp32 NCHW [B,C,H,W], the
    scalings and dt [B].  Returns (loss, dFn [B,H,W,Cpad] with zero pad channels), both float64."""
    B, C = noisy_n.shape[:2]
    v = lambda t: t.double().view(B, 1, 1, 1)
    nchw = lambda F: F.double()[..., :C].permute(0, 3, 1, 2)
    pred = v(cs_n) * noisy_n.double() + v(co_n) * nchw(Fn)
    targ = v(cs_c) * noisy_c.double() + v(co_c) * nchw(Fc)
    md = None if mask is None else mask.double()
    loss = ect_loss(pred, targ, md, dt.double(), c, lam)
    dpred = ect_grad(pred, targ, md, dt.double(), c, lam)
    dFn = torch.zeros(Fn.shape, dtype=torch.float64)
    dFn[..., :C] = (grad_scale * dpred * v(co_n)).permute(0, 2, 3, 1)
    return loss, dFn


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def ect_forward(P, x, sigma, cfg):
    """CMGenerator.ect_forward in training mode: the `_train` scalings, no conditioning image"""
    emb = O.cm_noise_level_embedding(P, sigma)
    return skip_train(sigma).view(-1, 1, 1, 1) * x + out_train(sigma).view(-1, 1, 1, 1) * O.unet_forward(P, x, emb, cfg, prefix="cm_model.")


def ect_generator_forward(P, x, mask, noise, rnd_normal, cfg, stage=0):
    """the ECT branch of CMGenerator.forward with its two draws injected: (D_yt, D_yr, t_noisy_x, r_noisy_x, t, r)"""
    t = (rnd_normal * P_STD + P_MEAN).exp()
    r = t_to_r(t, stage)
    m = None if mask is None else torch.clamp(mask, min=0.0, max=1.0)
    t_noisy_x = x + t.view(-1, 1, 1, 1) * noise
    if m is not None:
        t_noisy_x = t_noisy_x * m + (1 - m) * x
    D_yt = ect_forward(P, t_noisy_x, t, cfg)
    with torch.no_grad():
        r_noisy_x = x + r.view(-1, 1, 1, 1) * noise
        if m is not None:
            r_noisy_x = r_noisy_x * m + (1 - m) * x
        D_yr = ect_forward(P, r_noisy_x, r, cfg)
    return D_yt, D_yr, t_noisy_x, r_noisy_x, t, r


class OracleECTTrainer(O.OracleCMTrainer):
    """CMModel.optimize_parameters() with ft_mode "ect": the optimizer and EMA of OracleCMTrainer, the ECT forward and loss"""

    stage = 0

    def loss_and_grads(self, y_0, mask, noise, rnd_normal):
        P = OrderedDict()
        for k, v in self.P.items():
            P[k] = v.detach().clone().requires_grad_(True) if k in self.m else v
        out = ect_generator_forward(P, y_0, mask, noise, rnd_normal, self.cfg, self.stage)
        self.current_t += y_0.shape[0]
        loss = ect_loss(out[0], out[1], mask, out[4] - out[5], ECT_C, self.lambda_G)
        gs = getattr(self, "grad_scale", 1.0)
        (loss * gs).backward()
        grads = {k: (P[k].grad / gs if P[k].grad is not None else torch.zeros_like(P[k])) for k in self.train_names}
        return loss.detach(), grads, out
