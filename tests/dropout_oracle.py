"""The CPU oracle trainer of the CUT step (oracle/jg_oracle.py::OracleCUTTrainer) with G_dropout / D_dropout, test helper.

The oracle's networks are module-level functions of jg_oracle; `OracleCUTDropoutTrainer.step` swaps two of them for the duration of a step:
  resnet_block         [pad, conv, IN, ReLU, Dropout(0.5), pad, conv, IN] + skip: the second convolution is `conv_block.6` (resnet_generator.py:62-88)
  nlayer_discriminator Dropout(0.5) behind every LeakyReLU, convolutions at model.0 / 3 / 7 / 11 / 15 (discriminators.py:51-108)
Dropout is x * (u < 0.5) / 0.5 with u GIVEN: `dropout` maps (module path, invocation of that module within the step) to the uniforms the
reference drew (tests/golden/dropout/cutstep_dropout.pt), paths as the fixture names them (`netG_A.encoder.model.10.conv_block.4`,
`netD_B_basic.model.2`).  Every module counts its own invocations, so the order of the oracle's passes only has to agree with the
reference's per module.  `used` holds the keys consumed by the last step."""
import torch
import torch.nn.functional as F

import jg_oracle as O

KEEP = 0.5


class OracleCUTDropoutTrainer(O.OracleCUTTrainer):
    def _drop(self, path, x):
        call = self._calls_of.get(path, 0)
        self._calls_of[path] = call + 1
        u = self._table[(path, call)]
        assert tuple(u.shape) == tuple(x.shape), (path, call, tuple(u.shape), tuple(x.shape))
        self.used.add((path, call))
        return O._q(x * (u < KEEP).to(x.dtype) / KEEP)

    def _resnet_block(self, P, pre, x):
        h = O._q(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), P[pre + "conv_block.1.weight"], P[pre + "conv_block.1.bias"]))
        h = self._drop("netG_A." + pre + "conv_block.4", O._q(F.relu(O._inorm(h))))
        h = O._q(F.conv2d(F.pad(h, (1, 1, 1, 1), mode="reflect"), P[pre + "conv_block.6.weight"], P[pre + "conv_block.6.bias"]))
        return O._q(x + O._inorm(h))

    def _discriminator(self, P, x, n_layers=3, pre="model."):
        conv = lambda h, i, stride: O._q(F.conv2d(h, P[f"{pre}{i}.weight"], P[f"{pre}{i}.bias"], stride=stride, padding=1))
        h = self._drop(f"netD_B_basic.{pre}2", O._q(F.leaky_relu(conv(O._q(x), 0, 2), 0.2)))
        idx = 3
        for n in range(1, n_layers + 1):
            h = O._q(F.leaky_relu(O._inorm(conv(h, idx, 2 if n < n_layers else 1)), 0.2))
            h = self._drop(f"netD_B_basic.{pre}{idx + 3}", h)
            idx += 4
        return conv(h, idx, 1)

    def step(self, real_A, real_B, ids_AB, ids_idt=None, dropout=None):
        self._table, self._calls_of, self.used = dict(dropout), {}, set()
        keep = O.resnet_block, O.nlayer_discriminator
        O.resnet_block, O.nlayer_discriminator = self._resnet_block, self._discriminator
        try:
            return self.iteration(real_A, real_B, ids_AB, ids_idt, iter_size=1)
        finally:
            O.resnet_block, O.nlayer_discriminator = keep


def trainer_for(g, rng):
    """tests/test_oracle_golden.py::cut_trainer_for for a fixture recorded with G_dropout and D_dropout"""
    c, hp = g["cfg"], g["hp"]
    sd = lambda keys, shapes, seed: O.synth_state_dict({k: torch.empty(g[shapes][k]) for k in g[keys]}, seed)
    return OracleCUTDropoutTrainer(sd("keysG", "shapesG", 0), sd("keysF", "shapesF", 3), sd("keysD", "shapesD", 1), c["n_blocks"],
                                   [int(i) for i in c["nce_layers"].split(",")], num_patches=c["num_patches"], T=hp["T"], monce=c["nce_loss"] == "monce",
                                   lambda_NCE=hp["lambda_NCE"], lambda_GAN=hp["lambda_GAN"], lr_G=hp["lr_G"], lr_D=hp["lr_D"], beta1=hp["beta1"],
                                   beta2=hp["beta2"], eps=hp["eps"], pool_size=c["pool"], pool_rng=rng, ema_beta=hp["ema_beta"], gen="resnet")
