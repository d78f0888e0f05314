"""Generate tests/golden/dropout/ from the UNMODIFIED reference on CPU (TEST INFRASTRUCTURE ONLY):
  * resblock.pt  : one ResnetBlock(16, "reflect", InstanceNorm2d, use_dropout=True, use_bias=True) on [2, 16, 9, 7];
  * patchgan.pt  : NLayerDiscriminator(3, ndf=16, n_layers=3, InstanceNorm2d, use_dropout=True) on [2, 3, 32, 32];
    both: input, state_dict keys / shapes (the weights are jg_oracle.synth_state_dict of them, seed 0 / 1), the uniforms of every Dropout
    invocation, output, the input gradient and parameter-gradient checksums for a seeded grad_output;
  * cutstep_dropout.pt : 3 x CUTModel.optimize_parameters() of the `patchnce` step configuration of oracle/make_golden_cutstep.py with
    G_dropout and D_dropout on, recorded by that recipe's own loop.  Beside what the recipe records, every step carries under "dropout" the
    list of (module path, invocation of that module within the step, uniforms) in invocation order.  The step's uniforms are stored in 16 bits,
    q = floor(u * 65536) - 32768 as int16: u < 0.5 exactly when q < 0, so the mask of keep = 0.5 is the reference's bit for bit
    (`dequant`: u = (q + 32768.5) / 65536).
Only torch.nn.functional.dropout is wrapped: it draws u = torch.rand(x.shape), records it and returns x * (u < keep) / keep -- nn.Dropout's
definition with the draw made visible.  The reference is imported at run time through oracle/ref_shim.py; nothing of its text is here.
   PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_fixture_dropout.py [output directory]"""
import functools
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
_argv, sys.argv = sys.argv, sys.argv[:1]          # make_golden_cutstep reads its own selection from sys.argv at import
import make_golden_cutstep as MG  # noqa: E402  (installs ref_shim)

sys.argv = _argv
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import jg_oracle as O  # noqa: E402
from make_golden import checks  # noqa: E402

BASE = dict(MG.STEP_CFGS["patchnce"], iters=3)


class DropoutRecorder:
    """torch.nn.functional.dropout with its draw recorded; `watch(net, prefix)` names the Dropout modules by forward pre-hooks"""

    def __init__(self, seed):
        self.g, self.log, self.path, self.real = torch.Generator().manual_seed(seed), [], None, F.dropout

    def dropout(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        u = MG.REAL_RAND(x.shape, generator=self.g)
        self.log.append((self.path, u.clone()))
        return x * (u < 1.0 - p).to(x.dtype) / (1.0 - p)

    def watch(self, net, prefix=""):
        for name, m in net.named_modules():
            if isinstance(m, nn.Dropout):
                m.register_forward_pre_hook(lambda mod, inp, path=prefix + name: setattr(self, "path", path))

    def __enter__(self):
        F.dropout = self.dropout
        return self

    def __exit__(self, *a):
        F.dropout = self.real


def numbered(log):
    """[(path, u)] in invocation order -> [(path, invocation of that module, u)]"""
    seen, out = {}, []
    for path, u in log:
        out.append((path, seen.get(path, 0), u))
        seen[path] = seen.get(path, 0) + 1
    return out


def quant(u):
    return (torch.floor(u.double() * 65536.0) - 32768.0).to(torch.int16)


def dequant(q):
    return ((q.to(torch.float64) + 32768.5) / 65536.0).float()


def module_fixture(out, name, net, x, seed):
    sd = O.synth_state_dict(net.state_dict(), seed=seed)
    net.load_state_dict(sd)
    net.train()
    x = x.clone().requires_grad_(True)
    with DropoutRecorder(41) as rec:
        rec.watch(net)
        y = net(x)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(43))
    y.backward(R)
    torch.save(dict(x=x.detach(), keys=list(sd.keys()), shapes={k: tuple(v.shape) for k, v in sd.items()}, seed=seed, u=numbered(rec.log),
                    out=y.detach(), R=R, dx=x.grad.clone(), grad_checks=checks({k: p.grad for k, p in net.named_parameters()})),
               os.path.join(out, f"{name}.pt"))
    print(name, tuple(y.shape), [(p, c, tuple(u.shape)) for p, c, u in numbered(rec.log)])


def module_fixtures(out):
    from models.modules.discriminators import NLayerDiscriminator
    from models.modules.resnet_architecture.resnet_generator import ResnetBlock

    inorm = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    g = torch.Generator().manual_seed(7)
    module_fixture(out, "resblock", ResnetBlock(16, "reflect", inorm, True, True), torch.randn(2, 16, 9, 7, generator=g), 0)
    module_fixture(out, "patchgan", NLayerDiscriminator(3, ndf=16, n_layers=3, norm_layer=inorm, use_dropout=True),
                   torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, 1)


def step_fixture(out):
    import models

    real_build_opt, real_create = MG.build_opt, models.create_model
    rec = DropoutRecorder(47)
    steps = []

    def build_opt(c):
        opt = real_build_opt(c)
        opt.G_dropout, opt.D_dropout = True, True
        return opt

    def create_model(opt, rank):
        model = real_create(opt, rank)
        rec.watch(model.netG_A, "netG_A.")
        rec.watch(model.netD_B_basic, "netD_B_basic.")
        assert any(isinstance(m, nn.Dropout) for m in model.netG_A.modules()) and any(isinstance(m, nn.Dropout) for m in model.netD_B_basic.modules())
        step = model.optimize_parameters

        def optimize_parameters():
            n = len(rec.log)
            step()
            steps.append([(p, c, quant(u)) for p, c, u in numbered(rec.log[n:])])

        model.optimize_parameters = optimize_parameters
        return model

    keep = MG.STEP_CFGS, MG.OUT, MG.ONLY
    MG.STEP_CFGS, MG.OUT, MG.ONLY, MG.build_opt = {"dropout": BASE}, out, [], build_opt
    models.create_model = create_model
    try:
        with rec:
            MG.step_fixtures()
    finally:
        (MG.STEP_CFGS, MG.OUT, MG.ONLY), MG.build_opt = keep, real_build_opt
        models.create_model = real_create
    path = os.path.join(out, "cutstep_dropout.pt")
    g = torch.load(path, weights_only=False)
    assert len(steps) == len(g["steps"]) == BASE["iters"]
    for s, d in zip(g["steps"], steps):
        for _, _, q in d:
            assert torch.equal(dequant(q) < 0.5, q < 0)
        s["dropout"] = d
    g["hp"].update(G_dropout=True, D_dropout=True)
    torch.save(g, path)
    print("cutstep_dropout:", [[(p, c, tuple(q.shape)) for p, c, q in d] for d in steps][0])


def main(out):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    os.chdir(tempfile.gettempdir())
    module_fixtures(out)
    step_fixture(out)
    print("bytes:", {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dropout"))
