"""Plain-torch restatement of the SRC_hDCE loss (test helper; runs on any device and in any float dtype).

Per problem (one image, or the whole minibatch with all negatives): q, k [P, D], temperature T, gamma.
  weights (detached):  kh_i = k_i / (|k_i| + 1e-7),  Gh = kh kh^T,  m_i = max_{j != i} Gh_ij,  w_ij = exp((Gh_ij - m_i) / gamma)  (j != i)
  logits:              S = q k^T,  a_ij = S_ij w_ij / T (j != i),  a_ii = -10 / T,  pos_i = q_i . detach(k_i) / T,  A_i = logsumexp_j a_ij
  value:               loss_i = log(e^A_i + e^pos_i) - pos_i  =  softplus(A_i - pos_i)
  gradient:            that of A_i - pos_i
An unweighted problem runs with w == 1."""
import torch


def _eye(P, like):
    return torch.eye(P, dtype=torch.bool, device=like.device)[None]


def hdce_weights(k, nimg, gamma):
    """[nimg, P, P], zero on the diagonal"""
    R, D = k.shape
    P = R // nimg
    k3 = k.detach().view(nimg, P, D)
    kh = k3 / (k3.pow(2).sum(2, keepdim=True).sqrt() + 1e-7)
    G = torch.bmm(kh, kh.transpose(1, 2))
    eye = _eye(P, k)
    if P == 1:
        return torch.zeros_like(G)
    m = G.masked_fill(eye, float("-inf")).max(dim=2, keepdim=True).values
    return torch.exp((G - m) / gamma).masked_fill(eye, 0.0)


def weighted_problems(nimg, wperiod, wcount, device=None):
    return torch.tensor([(b % wperiod) < wcount for b in range(nimg)], dtype=torch.bool, device=device)


def hdce_loss(q, k, nimg, T, gamma, wperiod=1, wcount=1):
    """per-patch loss [nimg * P] whose autograd gradient is the one the reference propagates"""
    R, D = q.shape
    P = R // nimg
    eye = _eye(P, q)
    w = hdce_weights(k, nimg, gamma)
    mask = weighted_problems(nimg, wperiod, wcount, q.device).view(nimg, 1, 1)
    w = torch.where(mask, w, torch.ones_like(w))
    S = torch.bmm(q.view(nimg, P, D), k.view(nimg, P, D).transpose(1, 2))
    a = (S * w / T).masked_fill(eye, -10.0 / T)
    A = torch.logsumexp(a, dim=2).view(-1)
    pos = (q * k.detach()).sum(1) / T
    v = A - pos
    # log(e^A + e^pos) - pos = softplus(A - pos), written without the cancellation of the first form where the loss is tiny (P = 1: e^-50)
    value = (v.clamp(min=0) + torch.log1p(torch.exp(-v.abs()))).detach()
    return value + (v - v.detach())


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))
