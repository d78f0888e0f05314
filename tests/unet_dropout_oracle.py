"""The CPU oracle of the diffusion UNet (oracle/jg_oracle.py) with G_dropout, test helper.

The oracle's ResBlock is the module-level function `jg_oracle.resblock`; `recorded_masks(table, keep)` swaps it, for the duration of a `with`
block, for a restatement that applies `_q(h * mask / keep)` between `_q(F.silu(h))` and the second convolution (unet_generator_attn.py:207-215,
254-258 of the reference).  `table` maps (module path, invocation of that module since the `with` began) to the boolean mask [B, C, H, W] the
reference drew (tests/golden/unet_dropout/, tests/tools/make_fixture_unet_dropout.py), paths as the fixture names them
(`denoise_fn.model.middle_block.0.out_layers.2`).  A block whose path has no entry at all runs without dropout (the reference's input and
output blocks have a rate of 0); a block that has entries but not for this invocation is an error.  The context yields the set of consumed
keys."""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import jg_oracle as O


def unpack(bits, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(bits.numpy())[:n].astype(bool)).reshape(shape)


def table_of(step):
    """a step of the fixture -> {(path, invocation): mask [B, C, H, W] bool}"""
    return {(path, call): unpack(bits, shape) for path, call, shape, bits in step["dropout"]}


def uniforms(mask):
    """what a device test injects for a recorded mask: u = 0 where the element was kept, 1 where it was dropped"""
    return (~mask).float()


@contextlib.contextmanager
def recorded_masks(table, keep):
    calls, used = {}, set()
    live = {path for path, _ in table}

    def drop(path, h):
        if path not in live:
            return h
        call = calls.get(path, 0)
        calls[path] = call + 1
        m = table[(path, call)]
        assert tuple(m.shape) == tuple(h.shape), (path, call, tuple(m.shape), tuple(h.shape))
        used.add((path, call))
        return O._q(h * m.to(h.dtype) / keep)

    def resblock(P, pre, x, emb, cfg, d):
        G = cfg.group_norm_size
        h = O._q(F.silu(O.group_norm(x, G, P[pre + ".in_layers.0.norm.weight"], P[pre + ".in_layers.0.norm.bias"])))
        conv_w, conv_b = P[pre + ".in_layers.2.weight"], P[pre + ".in_layers.2.bias"]
        if d["up"] or d["down"]:
            upd = (lambda t: F.interpolate(t, scale_factor=2, mode="nearest")) if d["up"] else (lambda t: F.avg_pool2d(t, kernel_size=2, stride=2))
            if cfg.efficient and d["up"]:
                h = O._q(F.conv2d(h, conv_w, conv_b, padding=1))
                h, x = upd(h), upd(x)
            else:
                h, x = O._q(upd(h)), O._q(upd(x))
                h = O._q(F.conv2d(h, conv_w, conv_b, padding=1))
        else:
            h = O._q(F.conv2d(h, conv_w, conv_b, padding=1))
        emb_out = F.linear(F.silu(emb), P[pre + ".emb_layers.1.weight"], P[pre + ".emb_layers.1.bias"]).type(h.dtype)[:, :, None, None]
        scale, shift = torch.chunk(emb_out, 2, dim=1)
        h = O.group_norm(h, G, P[pre + ".out_layers.0.norm.weight"], P[pre + ".out_layers.0.norm.bias"]) * (1 + scale) + shift
        h = drop(pre + ".out_layers.2", O._q(F.silu(h)))
        h = F.conv2d(h, P[pre + ".out_layers.3.weight"], P[pre + ".out_layers.3.bias"], padding=1)
        skip = x if d["cin"] == d["cout"] else O._q(F.conv2d(x, P[pre + ".skip_connection.weight"], P[pre + ".skip_connection.bias"]))
        return O._q((1.0 / math.sqrt(2) if cfg.efficient else 1.0) * skip + h)

    real, O.resblock = O.resblock, resblock
    try:
        yield used
    finally:
        O.resblock = real
