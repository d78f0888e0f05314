"""HIP-event timing of the paired / identity pixel loss of the CUT model: ops.pixel_loss (jg_pixel_loss: two launches, and
jg_pixel_loss_bwd: one launch, csrc/elementwise.hip) with both segments on, beside the same two terms as a plain torch composition
((x[..., :3].float() - y[..., :3].float()).abs().mean() per segment, and its autograd) on the same tensors, and one
optimize_parameters() of cut_model at the shape of `bench.py --model cut` with the two options off and on.  Same process, same box;
median of the timed calls.

    python tools/pixel_loss_bench.py [--batch 16] [--size 256] [--channels 3] [--dtype bf16] [--warmup 20] [--iters 100]
        [--step-warmup 8] [--step-iters 20] [--no-step] [--out FILE.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


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


def step_model(pixel, batch, size, dtype_name):
    """the model of `bench.py --model cut` (resnet 9 blocks, basic D, MoNCE), with or without the pixel-loss options"""
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(model_type="cut", G_netG="resnet", G_ngf=64, G_nblocks=9, D_netDs=["basic"], D_ndf=64, D_proj_interp=size, data_crop_size=size,
              data_load_size=size, train_batch_size=batch, train_iter_size=1, train_optim="adam", train_G_ema=True, train_G_ema_beta=0.999,
              gpu_ids="0", jg_act_dtype=dtype_name, name="pixel_loss_bench", checkpoints_dir="/tmp/jg_bench_ckpt/")
    if pixel:
        ov.update(alg_cut_supervised_loss=["L1"], alg_cut_MSE_idt=True)
    opt = opt_from_json({}, ov)
    torch.manual_seed(0)
    model = create_model(opt, 0)
    g = torch.Generator().manual_seed(1)
    data = {k: (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda() for k in ("A", "B")}
    model.data_dependent_initialize(data)
    model.setup(opt)
    model.single_gpu()

    def step():
        model.set_input(data)
        model.optimize_parameters()

    return model, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step-warmup", type=int, default=8)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.warmup >= 10 and a.iters >= 50 and a.step_warmup >= 4      # (the step graphs are captured on the third step)

    from joligen_amd import ops

    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    M, C, S = a.batch, a.channels, a.size
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    x = torch.randn(2 * M, S, S, 8, device=d, generator=g).to(dtype).requires_grad_(True)
    y = torch.randn(M, S, S, 8, device=d, generator=g).to(dtype)
    up = torch.ones(2, device=d)
    modes, lambdas = (ops.PIXEL_L1, ops.PIXEL_L1), (1.0, 1.0)

    def fused_fwd():
        return ops.pixel_loss(x, y, C, modes, lambdas)

    def fused_bwd():
        return ops._pixel_loss_bwd_launch(x.detach(), y, up, C, modes, lambdas)

    def torch_fwd():
        yv = y[..., :C].float()
        return torch.stack([(x[:M, ..., :C].float() - yv).abs().mean(), (x[M:, ..., :C].float() - yv).abs().mean()])

    loss_t = torch_fwd()

    def torch_bwd():
        return torch.autograd.grad(loss_t, x, up, retain_graph=True)

    t_f, m_f = timed(fused_fwd, a.warmup, a.iters)
    t_b, m_b = timed(fused_bwd, a.warmup, a.iters)
    t_tf, m_tf = timed(torch_fwd, a.warmup, a.iters)
    t_tb, m_tb = timed(torch_bwd, a.warmup, a.iters)
    px = M * S * S
    rd = (2 * px + px) * 16          # both segments of x and y once (y is read by both segments: the second read is counted in the rate below)
    lines = [
        f"# Pixel-loss kernel: x [{2 * M}, {S}, {S}, 8] in two segments against y [{M}, {S}, {S}, 8], {C} valid channels, {a.dtype}, both segments L1",
        "",
        f"HIP events around each call (the Python wrapper included: output and workspace allocations), {a.warmup} warm-up + {a.iters} timed "
        f"calls, median (minimum in brackets); {torch.cuda.get_device_name(0)}.",
        f"Bytes: x {2 * px * 16 / 1e6:.1f} MB, y {px * 16 / 1e6:.1f} MB (read once per segment); the gradient store is {2 * px * 16 / 1e6:.1f} MB.",
        "",
        "| path | launches | time per call | GB/s over (x + 2 y [+ dx]) |",
        "|---|---|---|---|",
        f"| `ops.pixel_loss` forward (`jg_pixel_loss`) | 2 | {t_f * 1e3:.1f} us ({m_f * 1e3:.1f}) | {(rd + px * 16) / t_f / 1e6:.0f} |",
        f"| backward (`jg_pixel_loss_bwd`) | 1 | {t_b * 1e3:.1f} us ({m_b * 1e3:.1f}) | {(rd + px * 16 + 2 * px * 16) / t_b / 1e6:.0f} |",
        f"| torch composition forward (slice, float, sub, abs, mean per segment) | many | {t_tf * 1e3:.1f} us ({m_tf * 1e3:.1f}) | |",
        f"| torch composition backward (autograd) | many | {t_tb * 1e3:.1f} us ({m_tb * 1e3:.1f}) | |",
        "",
        f"ratio torch / fused: forward {t_tf / t_f:.1f}, backward {t_tb / t_b:.1f}",
    ]
    if not a.no_step:
        res = {}
        for pixel in (False, True):
            model, step = step_model(pixel, M, S, a.dtype)
            res[pixel] = timed(step, a.step_warmup, a.step_iters) + (model.step_driver,)
            del model, step
            torch.cuda.empty_cache()
        lines += ["", f"One `optimize_parameters()` (set_input on a device-resident batch included) of the model of `bench.py --model cut` (resnet 9 blocks, "
                  f"basic D, MoNCE, {S} x {S}), batch {M}, {a.dtype}, {a.step_warmup} warm-up + {a.step_iters} timed steps, median (minimum):", "",
                  "| alg_cut_supervised_loss / alg_cut_MSE_idt | ms per step | step driver |", "|---|---|---|"]
        label = {False: "off (default)", True: '["L1"] / true'}
        lines += [f"| {label[pixel]} | {res[pixel][0]:.2f} ({res[pixel][1]:.2f}) | {res[pixel][2]} |" for pixel in (False, True)]
        lines += ["", f"ratio on / off: {res[True][0] / res[False][0]:.3f}"]
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
