"""HIP-event timing of the easy-consistency-tuning loss: ops.ect_loss (jg_ect_loss: two launches, csrc/elementwise.hip) beside
ops.cm_loss (jg_cm_loss: one launch with an atomic per block) on the same tensors, and one optimize_parameters() of cm_model in each
training mode (alg_ddpm_ft_mode "ect" / "cm") at the BASELINE configs[4] shape.  Same process, same box; median of the timed calls.

    python tools/ect_loss_bench.py [--batch 32] [--size 256] [--channels 3] [--dtype bf16] [--warmup 20] [--iters 100]
        [--step-batch 32] [--step-warmup 5] [--step-iters 20] [--no-step] [--out FILE.md]
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


def step_model(ft_mode, batch, size, dtype_name):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    opt = opt_from_json({}, dict(model_type="cm", G_ngf=64, G_unet_mha_channel_mults=[1, 2, 4, 8], G_unet_mha_res_blocks=[2, 2, 2, 2],
                                 G_unet_mha_attn_res=[16], G_unet_mha_vit_efficient=True, data_crop_size=size, train_batch_size=batch,
                                 gpu_ids="0", jg_act_dtype=dtype_name, train_optim="adamw", train_G_ema=True, train_iter_size=1,
                                 checkpoints_dir="/tmp/jg_amd_ckpt/", name="ect_bench", alg_ddpm_ft_mode=ft_mode))
    torch.manual_seed(0)
    model = create_model(opt, 0)
    model.setup(opt)
    model.single_gpu()
    g = torch.Generator().manual_seed(1)
    Bimg = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
    mask = torch.zeros(batch, 1, size, size, dtype=torch.int64)
    mask[:, :, size // 4: 3 * size // 4, size // 4: 3 * size // 4] = 1
    A = Bimg * (1 - mask) + torch.randn(Bimg.shape, generator=g) * mask
    data = {"A": A.cuda(), "B": Bimg.cuda(), "B_label_mask": mask.cuda()}

    def step():
        model.set_input(data)
        model.optimize_parameters()

    return model, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step-batch", type=int, default=32)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.warmup >= 10 and a.iters >= 50

    from joligen_amd import ops

    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    B, C, S = a.batch, a.channels, a.size
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    Fn = torch.randn(B, S, S, 8, device=d, generator=g).to(dtype).requires_grad_(True)
    Fc = torch.randn(B, S, S, 8, device=d, generator=g).to(dtype)
    noisy_n = torch.randn(B, C, S, S, device=d, generator=g)
    noisy_c = torch.randn(B, C, S, S, device=d, generator=g)
    v = [torch.rand(B, device=d, generator=g) + 0.1 for _ in range(5)]
    mask = (torch.rand(B, 1, S, S, device=d, generator=g) < 0.5).long()

    def ect():
        return ops.ect_loss(Fn, Fc, noisy_n, noisy_c, v[0], v[1], v[2], v[3], mask, v[4], 1.0, 1.0)

    def cm():
        return ops.cm_loss(Fn, Fc, noisy_n, noisy_c, v[0], v[1], v[2], v[3], mask, v[4], 1.0, 1.0)

    t_e, m_e = timed(ect, a.warmup, a.iters)
    t_c, m_c = timed(cm, a.warmup, a.iters)
    px = B * S * S
    read = px * (2 * 16 + 2 * 4 * C + 8)
    lines = [
        f"# Easy-consistency-tuning loss kernel: batch {B}, {C} x {S} x {S}, {a.dtype} UNet outputs (Cpad 8), int64 label mask",
        "",
        f"HIP events around each call (the Python wrapper included: output allocations, for `cm_loss` the zeroing of its accumulator), "
        f"{a.warmup} warm-up + {a.iters} timed calls, median (minimum in brackets); {torch.cuda.get_device_name(0)}.",
        f"Bytes per pass over the inputs: {read / 1e6:.1f} MB read; the gradient store is {px * 16 / 1e6:.1f} MB more.",
        "",
        "| path | launches | passes over the inputs | time per call | GB/s over (passes x read + store) |",
        "|---|---|---|---|---|",
        f"| `ops.ect_loss` (`jg_ect_loss`) | 2 | 2 | {t_e * 1e3:.1f} us ({m_e * 1e3:.1f}) | {(2 * read + px * 16) / t_e / 1e6:.0f} |",
        f"| `ops.cm_loss` (`jg_cm_loss`) | 1 (+ memset) | 1 | {t_c * 1e3:.1f} us ({m_c * 1e3:.1f}) | {(read + px * 16) / t_c / 1e6:.0f} |",
        "",
        f"ratio ect / cm: {t_e / t_c:.2f}",
    ]
    if not a.no_step:
        res = {}
        for mode in ("cm", "ect"):
            model, step = step_model(mode, a.step_batch, S, a.dtype)
            res[mode] = timed(step, a.step_warmup, a.step_iters)
            del model, step
            torch.cuda.empty_cache()
        lines += ["", f"One `optimize_parameters()` (set_input on a device-resident batch included) at the configs[4] shape (unet_mha ngf 64, mults "
                  f"[1,2,4,8], 2 res-blocks per level, mid-block attention, {S} x {S}), batch {a.step_batch}, {a.dtype}, {a.step_warmup} warm-up + "
                  f"{a.step_iters} timed steps, median (minimum):", "",
                  "| alg_ddpm_ft_mode | ms per step |", "|---|---|"]
        lines += [f"| `{mode}` | {res[mode][0]:.2f} ({res[mode][1]:.2f}) |" for mode in ("cm", "ect")]
        lines += ["", f"ratio ect / cm: {res['ect'][0] / res['cm'][0]:.3f} (the noise levels differ between the modes; the kernels run do not "
                  "depend on them)"]
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
