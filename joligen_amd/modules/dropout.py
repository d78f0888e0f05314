"""nn.Dropout(0.5) of the CUT ResNet generator (resnet_generator.py:62-88 of the reference) and of the PatchGAN (discriminators.py:51-108) as a
placeholder at the reference's nn.Sequential index: it holds no parameter, keeps the `state_dict` keys where the reference has them, and is
never run as a module -- the walkers of resnet_generator.py / discriminators.py fold it into the normalise + activate pass in front of it
(ops.group_norm(keep=...) / ops.activation_dropout, csrc/dropout.hip).  In eval() it is the identity, as nn.Dropout is.

Every placeholder has a fixed `stream` (the Philox stream of its masks, unique within a DropoutState) and a `path` (its name for injected
uniforms); a DropoutState is shared by the networks of one model and holds what changes per step: the Philox key and how often each
placeholder has been invoked (`call`: the reference draws a fresh mask on every invocation of a Dropout module)."""
from __future__ import annotations

import torch.nn as nn


class DropoutState:
    def __init__(self):
        self.key = None         # two-word device tensor (ops.d_aug_key), drawn once per step
        self.rand = None        # parity runs: callable(module_path, call, shape_BCHW, device) -> fp32 uniforms
        self.calls = {}         # stream -> invocations since begin_step

    def begin_step(self, key=None):
        """a new step: every placeholder's next invocation is call 0; `key` replaces the Philox key (None: kept)"""
        self.calls.clear()
        if key is not None:
            self.key = key

    def ensure_key(self, device):
        """a state nobody has given a key (no step driver) draws one, on the current stream; injected uniforms need none"""
        if self.rand is None and self.key is None:
            from .. import ops

            self.key = ops.d_aug_key(device)

    def next(self, m, x=None, shape=None, device=None, call=None, key=None, keep=None):
        """the dropout arguments of ops.group_norm / ops.activation_dropout for one invocation of placeholder `m` on x [B, H, W, C] (or a mask
        of `shape` on `device`).  call / key None: the placeholder's next invocation and this state's key; given (the fused schedule of the
        diffusion UNet names the call and key of its node): the counter moves past `call`.  keep None: 1 - m.p."""
        if x is not None:
            shape, device = x.shape, x.device
        if call is None:
            call = self.calls.get(m.stream, 0)
        self.calls[m.stream] = call + 1
        u = None
        if self.rand is not None:
            B, H, W, C = shape
            u = self.rand(m.path, call, (B, C, H, W), device)
        elif key is None:
            key = self.key
            if key is None:
                raise RuntimeError(f"dropout {m.path or m.stream}: no Philox key (DropoutState.begin_step(ops.d_aug_key(device))) and no dropout_rand")
        return dict(keep=1.0 - m.p if keep is None else keep, u=u, key=key, stream=m.stream, call=call)


class FusedDropout(nn.Dropout):
    def __init__(self, p=0.5):
        super().__init__(p)
        self.stream, self.path, self.state = 0, "", None

    def forward(self, x):
        raise RuntimeError("FusedDropout is folded into the pass in front of it by its network's walker; it is not called")

    def args(self, x):
        return self.state.next(self, x)


class DropoutOwner:
    """mix-in of a network with placeholders: `dropout_state`, and `dropout_rand` as the attribute that injects uniforms"""

    @property
    def dropout_rand(self):
        return self.dropout_state.rand

    @dropout_rand.setter
    def dropout_rand(self, fn):
        self.dropout_state.rand = fn


def bind_dropout(net, state, prefix="", first_stream=0):
    """give every placeholder of `net` its path (prefix + module name), the next free stream and the shared state -> the next free stream"""
    n = first_stream
    for name, m in net.named_modules():
        if isinstance(m, DropoutOwner) and hasattr(m, "dropout_state"):      # the network and its blocks: one state, none left behind
            m.dropout_state = state
        if isinstance(m, FusedDropout):
            if n > 0xffff:
                raise ValueError("more than 65536 dropout streams")
            m.stream, m.path, m.state = n, prefix + name, state
            n += 1
    return n
