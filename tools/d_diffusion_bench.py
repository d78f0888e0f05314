"""Timing of dataaug_D_diffusion (Diffusion-GAN noise on the projected discriminator's backbone features) on the GPU:

1. the fused launches (ops.d_diffusion forward + backward: jg_d_diffusion / jg_d_diffusion_bwd of csrc/d_diffusion.hip, t and noise drawn in the
   kernel) beside the same arithmetic composed from torch ops per level (randint, two gathers, randn, multiply-add, the backward's multiply) at the
   feature shapes of the `cut_effnet` benchmark leg, HIP events; and ops.d_diffusion_update beside the reference's form (host read of the loss);
2. one optimize_parameters() of the `cut_effnet`-shaped model (SegFormer-attn G, [projected_d (tf_efficientnet_lite0), basic] D) with the option
   off and on: the two models are built once and timed ALTERNATELY in rounds in one process, so that the spread of one configuration over the
   rounds stands beside the difference between them.

    python tools/d_diffusion_bench.py [--batch 16] [--size 256] [--p 0.37] [--warmup 20] [--iters 100] [--step-warmup 8] [--rounds 5]
        [--round-steps 10] [--no-step] [--out profiles/d_diffusion.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import joligen_amd  # noqa: E402,F401  (before the first HIP call: the package makes captured graphs safe to replay, joligen_amd/__init__.py)

WIDTHS, STRIDES = (24, 40, 112, 320), (4, 8, 16, 32)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def state_at(p, device):
    from joligen_amd import ops

    st = ops.DDiffusionState.fresh(device)
    st.p.fill_(p)
    ops.d_diffusion_update(st, torch.tensor(0.9, device=device), 0)      # loss == 0.9: p stays, the tables and t_epl are built from it
    return st


def kernel_rows(a, dtype_name):
    from joligen_amd import ops

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    B, S = a.batch, a.size
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    xs = [torch.randn(B, S // s, S // s, c, device=d, generator=g).to(dtype).requires_grad_(True) for c, s in zip(WIDTHS, STRIDES)]
    dys = [torch.randn_like(x) for x in xs]
    st = state_at(a.p, d)
    key = ops.d_aug_key(d)
    nbytes = sum(x.numel() * 2 for x in xs)
    t_epl = st.t_epl.long()

    def fused():
        outs, _ = ops.d_diffusion(xs, st, 0.5, key=key)
        torch.autograd.grad(outs, xs, dys)

    def fused_fwd():
        with torch.no_grad():
            ops.d_diffusion(xs, st, 0.5, key=key)

    def composed_level(x, dy):
        Bc = (x.shape[0], 1, 1, x.shape[3])
        t = t_epl[torch.randint(0, 64, (x.shape[0] * x.shape[3],), device=d)]
        at, bt = st.a[t].view(Bc), st.b[t].view(Bc)
        out = (at * x.detach().float() + bt * (torch.randn(x.shape, device=d) * 0.5)).to(dtype)
        return out, (at * dy.float()).to(dtype)

    def composed():
        for x, dy in zip(xs, dys):
            composed_level(x, dy)

    def composed_fwd():
        for x in xs:
            Bc = (x.shape[0], 1, 1, x.shape[3])
            t = t_epl[torch.randint(0, 64, (x.shape[0] * x.shape[3],), device=d)]
            (st.a[t].view(Bc) * x.detach().float() + st.b[t].view(Bc) * (torch.randn(x.shape, device=d) * 0.5)).to(dtype)

    with torch.no_grad():
        _, ts = ops.d_diffusion(xs, st, 0.5, key=key)
    tl = [t.long() for t in ts]

    def fused_bwd():                # the backward launch on its own, without the autograd engine around it
        ops._d_diffusion_bwd_launch(dys, ts, st.a)

    def composed_bwd():
        for dy, t in zip(dys, tl):
            (st.a[t].view(dy.shape[0], 1, 1, dy.shape[3]) * dy.float()).to(dtype)

    rows = []
    for label, f, c, launches in (("forward (4 levels)", fused_fwd, composed_fwd, 1), ("backward (4 levels), launched directly", fused_bwd, composed_bwd, 1),
                                  ("forward + backward (4 levels) through autograd", fused, composed, 2)):
        t_f, m_f = timed(f, a.warmup, a.iters)
        t_t, m_t = timed(c, a.warmup, a.iters)
        moved = nbytes * 2 * launches
        rows.append(f"| {dtype_name} | {label} | {launches} | {t_f * 1e3:.1f} us ({m_f * 1e3:.1f}) | {moved / 1e6:.1f} MB | {t_t * 1e3:.1f} us ({m_t * 1e3:.1f}) | "
                    f"{t_t / t_f:.1f} |")
    if dtype_name == "bf16":
        loss = torch.tensor(1.0, device=d)
        host = {"p": a.p}

        def fused_update():
            ops.d_diffusion_update(st, loss, B * 4, key=key)

        def host_update():          # the reference's form: the sign of the loss is read back on the host (a synchronisation), the tables rebuilt there
            import numpy as np

            host["p"] = float(np.clip(host["p"] + float(torch.sign(loss - 0.9)) * (B * 4) / 100000.0, 0.0, 1.0))
            T = int(np.clip(5 + round(host["p"] * 495), 5, 500))
            betas = torch.from_numpy(np.linspace(1e-4, 1e-2, T)).float()
            cp = torch.cat([torch.tensor([1.0]), (1.0 - betas).cumprod(0)])
            return torch.sqrt(cp).to(d), torch.sqrt(1 - cp).to(d)

        t_f, m_f = timed(fused_update, a.warmup, a.iters)
        t_t, m_t = timed(host_update, a.warmup, a.iters)
        rows.append(f"| fp32 | `ops.d_diffusion_update` (p, T, n, tables, t_epl) | 1 | {t_f * 1e3:.1f} us ({m_f * 1e3:.1f}) | | {t_t * 1e3:.1f} us ({m_t * 1e3:.1f}), with "
                    f"its host read and without the draw of t_epl | {t_t / t_f:.1f} |")
    return rows


def step_model(on, batch, size, p):
    """the `cut_effnet` leg of bench.py: SegFormer-attn G, [projected_d (tf_efficientnet_lite0), basic] D, MoNCE; `on`: dataaug_D_diffusion at
    strength `p` (the tables and t_epl built by the update kernel)"""
    from joligen_amd import ops
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(model_type="cut", G_netG="segformer_attn_conv", G_ngf=64, G_nblocks=9, D_netDs=["projected_d", "basic"], D_ndf=64, D_proj_interp=size,
              D_proj_network_type="efficientnet", data_crop_size=size, data_load_size=size, train_batch_size=batch, train_iter_size=1, train_optim="adam",
              train_G_ema=True, train_G_ema_beta=0.999, gpu_ids="0", jg_act_dtype="bf16", name="d_diffusion_bench", checkpoints_dir="/tmp/jg_bench_ckpt/")
    if on:
        ov["dataaug_D_diffusion"] = True
    opt = opt_from_json({}, ov)
    torch.manual_seed(0)
    model = create_model(opt, 0)
    g = torch.Generator().manual_seed(1)
    data = {k: (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda() for k in ("A", "B")}
    model.data_dependent_initialize(data)
    model.setup(opt)
    model.single_gpu()
    if on:
        dif = model.netD_B_projected_d.freeze_feature_network.diffusion
        dif.p.fill_(p)
        ops.d_diffusion_update(dif.state, torch.tensor(0.9, device="cuda:0"), 0)

    def step():
        model.set_input(data)
        model.optimize_parameters()

    return model, step


def step_rows(a):
    import time
    import warnings

    variants = ("off", "on")
    built = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for v in variants:
            built[v] = step_model(v == "on", a.batch, a.size, a.p)
            for _ in range(a.step_warmup):
                built[v][1]()
            torch.cuda.synchronize()
        ms = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v in variants:                      # alternated: every round times every configuration once
                step = built[v][1]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.round_steps):
                    step()
                torch.cuda.synchronize()
                ms[v].append((time.perf_counter() - t0) * 1e3 / a.round_steps)
    med = {v: statistics.median(ms[v]) for v in variants}
    dif = built["on"][0].netD_B_projected_d.freeze_feature_network.diffusion
    rows = [f"| {v} | {med[v]:.2f} | {min(ms[v]):.2f} - {max(ms[v]):.2f} | {med[v] - med['off']:+.2f} | {built[v][0].step_driver} |" for v in variants]
    rows.append("")
    rows.append(f"State of the option-on model after the run: p = {float(dif.p):.5f}, T = {int(dif.Tn[0])}, n = {int(dif.Tn[1])}.")
    built.clear()
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--p", type=float, default=0.37)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step-warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.warmup >= 10 and a.iters >= 50 and a.step_warmup >= 4 and a.rounds >= 3      # (the step graphs are captured on the third step)
    assert torch.cuda.is_available(), "d_diffusion_bench.py measures on the GPU; there is no CPU path"

    B, S = a.batch, a.size
    shapes = ", ".join(f"[{B}, {S // s}, {S // s}, {c}]" for c, s in zip(WIDTHS, STRIDES))
    lines = [f"# dataaug_D_diffusion: the fused feature-noising kernels and the CUT step, batch {B}, interp {S}",
             "",
             f"{torch.cuda.get_device_name(0)}.  HIP events around each call (the Python wrapper and, for forward + backward, the autograd engine included), "
             f"{a.warmup} warm-up + {a.iters} timed calls, median (minimum in brackets).  Feature maps {shapes}, state at p = {a.p}.  The fused launches "
             "draw t and the noise in the kernel (Philox4x32-10, Box-Muller); the composition is, per level, randint, gathers of t_epl and of both "
             "tables, randn, the multiply-add in fp32 and the backward's multiply.  Bytes: the maps read and written once per launch; they fit the "
             "256 MiB Infinity Cache, so this is not an HBM-only figure.",
             "",
             "| dtype | what | fused kernel launches | fused | bytes moved | torch composition | torch / fused |",
             "|---|---|---|---|---|---|---|"]
    for dtype_name in ("bf16", "fp16"):
        lines += kernel_rows(a, dtype_name)
    if not a.no_step:
        lines += ["", f"One `optimize_parameters()` of the `cut_effnet`-shaped model (SegFormer-attn G, [projected_d (tf_efficientnet_lite0), basic] D; set_input on a "
                  f"device-resident batch included), batch {B}, {S} x {S}, bf16; {a.step_warmup} warm-up steps per model, then {a.rounds} rounds that time "
                  f"{a.round_steps} steps of each configuration in turn (host clock around steps that end in a device synchronise).  `spread`: the fastest "
                  "and slowest round of that configuration; `difference`: median against the option-off median.",
                  "", "| dataaug_D_diffusion | ms per step (median of rounds) | spread over rounds | difference to off | step driver |", "|---|---|---|---|---|"]
        lines += step_rows(a)
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
