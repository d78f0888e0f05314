"""The project's own restatement, in pure torch, of the semantic-consistency class branch (train_semantic_cls): the `basic` classifier
(3x3 stride-2 unpadded convolutions to a 1x1 map, BatchNorm2d on batch statistics + LeakyReLU(0.2), two Linear layers with no activation
between) and the three class losses with the gate and the argmax of `jg_cls_loss`.  Everything runs in the dtype of its inputs (float64 in
the GPU tests, float32 against the reference's fixture).  With `dtype` given the classifier becomes the project's rounding yardstick: every
inter-layer tensor, every back-propagated activation gradient and the convolution weights are rounded to that 16-bit type, where the HIP
network stores 16-bit values, and the two Linear layers run in float32, forward and backward, as they do there."""
import torch
import torch.nn.functional as F

CE, MSE, L1 = 0, 1, 2


class _Round(torch.autograd.Function):
    """store-and-reload through a 16-bit type, in the forward and in the backward"""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


class _RoundValue(torch.autograd.Function):
    """the 16-bit working copy of an fp32 master weight: rounded in the forward, the gradient passes unrounded (it is accumulated in fp32)"""

    @staticmethod
    def forward(ctx, w, dtype):
        return w.to(dtype).to(w.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def _r(x, dtype):
    return x if dtype is None else _Round.apply(x, dtype)


def conv_indices(sd):
    return sorted(int(k.split(".")[1]) for k, v in sd.items() if k.startswith("before_linear.") and k.endswith(".weight") and v.dim() == 4)


def bias_before_batchnorm(sd):
    """the convolution biases that a BatchNorm on batch statistics follows: their gradient is zero in real arithmetic (the norm removes the
    channel mean), so what any implementation returns for them is rounding noise"""
    return [f"before_linear.{i}.bias" for i in conv_indices(sd) if f"before_linear.{i + 1}.running_mean" in sd]


def classifier_forward(sd, x, training=True, dtype=None, momentum=0.1, eps=1e-5):
    """sd: the reference's state_dict layout (tensors of the working precision; the ones to differentiate require grad); x: NCHW image.
    Returns (logits [B, n], the buffers after this call).  Train mode normalises with the batch statistics (biased variance) and moves the
    running ones (unbiased variance, momentum 0.1); eval mode uses the running ones and leaves them."""
    h = _r(x, dtype)
    bufs = {}
    for i in conv_indices(sd):
        w = sd[f"before_linear.{i}.weight"]
        h = _r(F.conv2d(h, w if dtype is None else _RoundValue.apply(w, dtype), sd[f"before_linear.{i}.bias"], stride=2), dtype)
        bn = f"before_linear.{i + 1}."
        if bn + "running_mean" in sd:
            rm, rv, nbt = sd[bn + "running_mean"], sd[bn + "running_var"], sd[bn + "num_batches_tracked"]
            if training:
                n = h.numel() // h.shape[1]
                mean = h.mean(dim=(0, 2, 3))
                var = ((h - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
                bufs[bn + "running_mean"] = ((1 - momentum) * rm + momentum * mean).detach()
                bufs[bn + "running_var"] = ((1 - momentum) * rv + momentum * var * (n / max(n - 1, 1))).detach()
                bufs[bn + "num_batches_tracked"] = nbt + 1
            else:
                mean, var = rm, rv
                bufs.update({bn + "running_mean": rm, bn + "running_var": rv, bn + "num_batches_tracked": nbt})
            h = (h - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
            h = h * sd[bn + "weight"][None, :, None, None] + sd[bn + "bias"][None, :, None, None]
        h = _r(F.leaky_relu(h, 0.2), dtype)
    h = h.flatten(1)
    work = h.dtype if dtype is None else torch.float32      # the yardstick's tail runs in fp32, forward and backward, as the HIP network's does
    h = h.to(work)
    for j in (0, 1):
        h = F.linear(h, sd[f"after_linear.{j}.weight"].to(work), sd[f"after_linear.{j}.bias"].to(work))
    return h.to(x.dtype), bufs


def cls_loss(logits, target, mode=CE, lam=1.0, prev=None, threshold=1.0):
    """(loss, d loss / d logits, argmax, gate) as jg_cls_loss defines them: loss = lam * gate * mean_b l_b with gate = 1 without `prev`,
    else not (prev > threshold) (a NaN leaves it open); cross entropy as a max-subtracted log-sum-exp, the lowest index on ties in the argmax;
    a label outside [0, n) gives a NaN loss and a zero gradient row; a closed gate gives exactly 0 and zeros."""
    x = logits.detach().double()
    B, n = x.shape
    gate = 1.0 if prev is None else (0.0 if float(prev) > threshold else 1.0)
    d = torch.zeros_like(x)
    if mode == CE:
        m = x.max(dim=1).values
        arg = torch.tensor([int((x[b] == m[b]).nonzero()[0]) for b in range(B)], dtype=torch.int64)
        lse = torch.log(torch.exp(x - m[:, None]).sum(dim=1)) + m
        per = torch.empty(B, dtype=torch.float64)
        for b in range(B):
            t = int(target[b])
            if 0 <= t < n:
                per[b] = lse[b] - x[b, t]
                d[b] = torch.exp(x[b] - lse[b])
                d[b, t] -= 1.0
            else:
                per[b] = float("nan")
    else:
        if n != 1:
            raise ValueError("the regression modes take one value per sample")
        diff = x[:, 0] - target.double()
        per = diff * diff if mode == MSE else diff.abs()
        d[:, 0] = 2 * diff if mode == MSE else torch.sign(diff)
        arg = torch.zeros(B, dtype=torch.int64)
    if gate == 0.0:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(x), arg, False
    return lam * per.mean(), lam * d / B, arg, True
