"""Float64 restatement of the paired / identity pixel losses of the CUT model (jg_pixel_loss), test helper.

x [S*M, H, W, Cpad] in S segments of M images, every segment compared with the same y [M, H, W, Cpad] over the C valid channels; per
segment a mode (0 off, 1 L1, 2 MSE) and a weight:
  d = x_s - y,   loss_s = lambda_s * mean_{m,c,h,w}(|d| or d^2),   d loss_s / d x_s = lambda_s / (M C H W) * (sign(d) or 2 d)
The pad channels C.. never enter; an off segment is 0 with a zero gradient.  Everything is float64 on the caller's (16-bit) values."""
import torch

OFF, L1, MSE = 0, 1, 2


def _diff(x, y, C, S):
    M = y.shape[0]
    assert x.shape[0] == S * M and x.shape[1:] == y.shape[1:]
    xs = x.double()[..., :C].reshape(S, M, *x.shape[1:3], C)
    return xs - y.double()[..., :C][None]


def pixel_loss(x, y, C, modes, lambdas):
    """the S weighted losses, float64 [S]"""
    d = _diff(x, y, C, len(modes))
    out = []
    for s, (mode, lam) in enumerate(zip(modes, lambdas)):
        out.append(torch.zeros((), dtype=torch.float64) if mode == OFF else lam * (d[s].abs() if mode == L1 else d[s] ** 2).mean())
    return torch.stack(out)


def pixel_grad(x, y, C, modes, lambdas, g):
    """d (sum_s g[s] loss_s) / dx in closed form, float64 in the layout of x with zero pad channels"""
    S = len(modes)
    d = _diff(x, y, C, S)
    n = d[0].numel()
    dx = torch.zeros(S, *d.shape[1:4], x.shape[-1], dtype=torch.float64)
    for s, (mode, lam) in enumerate(zip(modes, lambdas)):
        if mode != OFF:
            dx[s][..., :C] = float(g[s]) * lam / n * (torch.sign(d[s]) if mode == L1 else 2.0 * d[s])
    return dx.reshape(x.shape)


def ordered_bits(x):
    """16-bit float -> integers in the order of the values (+0 and -0 both 0): neighbours differ by one"""
    b = x.cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))
