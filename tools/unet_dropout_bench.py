"""Timing of G_dropout in the diffusion UNet on the GPU:

1. the two kernels for a dropout behind a low-resolution GroupNorm + nearest 2x upsample (csrc/dropout.hip) beside their composed forms, on
   the tensors of the efficient UNet's up-blocks, the mask drawn in the kernel:
     forward   jg_gn_apply_drop_up2(c1)                                   |  jg_upsample2x_ld(c1), then jg_gn_apply_drop at the high resolution
     backward  jg_drop_pool2_bwd(dh), then the plain GroupNorm backward   |  jg_gn_bwd_reduce_drop + jg_gn_bwd_apply_drop at the high resolution
               (reduce + apply) at the low resolution                     |  on the upsampled c1, then jg_pool2x2_ld
   (the coefficient step between reduce and apply is the same launch on either side and is left out), HIP events around the launch helpers
   of joligen_amd/launch.py and modules/unet_exec.py, output allocation included on both sides;
2. one optimize_parameters() of palette_model at the shape of bench.py on ONE model whose rate and graph are switched between rounds:
   dropout 0 on the fused schedule (the launches of before); dropout 0.25 on the fused schedule (jg355::unet_fused_drop); dropout 0.25 on the
   module-by-module graph with the mask in the GroupNorm pass; dropout 0.25 on the module-by-module graph with a torch.rand mask per block
   (the `dropout_rand` hook: what a network with dropout ran before the fused schedule had the mask).  The configurations are timed
   alternately in rounds in one process, so that the spread over the rounds stands beside the differences.

    python tools/unet_dropout_bench.py [--batch 32] [--size 256] [--warmup 20] [--iters 100] [--step-warmup 6] [--rounds 5] [--round-steps 10]
        [--no-step] [--out profiles/unet_dropout.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import joligen_amd  # noqa: E402,F401  (before the first HIP call)

P_DROP = 0.25


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


def kernel_rows(a, shape):
    from joligen_amd import _lib, launch, ops
    from joligen_amd._lib import check
    from joligen_amd.modules import unet_exec as X

    B, H, W, C = shape
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    c1 = torch.randn(shape, device=d, generator=g).to(torch.bfloat16)
    dh = torch.randn((B, 2 * H, 2 * W, C), device=d, generator=g).to(torch.bfloat16)
    f32 = dict(device=d, dtype=torch.float32)
    ab = torch.stack((torch.rand((B, C), **f32) + 0.5, torch.randn((B, C), **f32) * 0.3), dim=-1).contiguous()
    pqr = torch.randn((B, C, 3), **f32) * 0.1
    red = torch.zeros((B, C, 2), **f32)
    act, keep = _lib.JG_ACT_SILU, 1.0 - P_DROP
    drop = (keep, None, ops.d_aug_key(d), 1, 0)
    L, dt = _lib.lib(), ops._dt(c1)
    c1_up = X.up2(c1, 1.0)

    def plain_bwd_low(dl):
        check(L.jg_gn_bwd_reduce_ld_acc(dt, c1.data_ptr(), C, dl.data_ptr(), C, ab.data_ptr(), red.data_ptr(), B, H * W, C, act, ops._st()), "reduce")
        out = torch.empty_like(c1)
        check(L.jg_gn_bwd_apply(dt, c1.data_ptr(), dl.data_ptr(), ab.data_ptr(), pqr.data_ptr(), out.data_ptr(), B, H * W, C, act, ops._st()), "apply")
        return out

    def composed_bwd():
        launch.gn_bwd_reduce_drop(c1_up, dh, ab, red, act, *drop)
        return X.pool2(launch.gn_bwd_apply_drop(c1_up, dh, ab, pqr, act, *drop), 1.0)

    pairs = {"forward": (lambda: launch.gn_apply_drop_up2(c1, ab, act, *drop), lambda: launch.gn_apply_drop(X.up2(c1, 1.0), ab, act, *drop)),
             "backward": (lambda: plain_bwd_low(launch.drop_pool2_bwd(dh, *drop)), composed_bwd)}
    n_lo, n_hi = c1.numel() * 2, dh.numel() * 2
    nbytes = {"forward": (n_lo + n_hi, n_lo + 3 * n_hi), "backward": (n_hi + n_lo + 5 * n_lo, 5 * n_hi + n_lo)}
    rows = []
    for name, (new, comp) in pairs.items():
        t_n, m_n = timed(new, a.warmup, a.iters)
        t_c, m_c = timed(comp, a.warmup, a.iters)
        rows.append(f"| {list(shape)} | {name} | {t_n * 1e3:.1f} us ({m_n * 1e3:.1f}), {nbytes[name][0] / 1e6:.1f} MB | "
                    f"{t_c * 1e3:.1f} us ({m_c * 1e3:.1f}), {nbytes[name][1] / 1e6:.1f} MB | {t_c / t_n:.2f} |")
    return rows


def step_rows(a):
    sys.path.insert(0, ROOT)
    import bench

    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    # the model of bench.py (build_model), with the rate
    opt = opt_from_json({}, dict(model_type="palette", G_netG="unet_mha", G_ngf=64, G_unet_mha_channel_mults=[1, 2, 4, 8], G_unet_mha_res_blocks=[2, 2, 2, 2],
                                 G_unet_mha_attn_res=[16], G_unet_mha_num_head_channels=32, G_unet_mha_vit_efficient=True, data_crop_size=a.size,
                                 data_load_size=a.size, train_batch_size=a.batch, train_iter_size=1, train_optim="adamw", train_G_ema=True,
                                 train_G_ema_beta=0.999, train_G_lr=2e-4, alg_diffusion_task="inpainting", alg_palette_loss="MSE", gpu_ids="0",
                                 jg_act_dtype="bf16", name="unet_dropout_bench", checkpoints_dir="/tmp/jg_bench_ckpt/", G_dropout=P_DROP))
    torch.manual_seed(0)
    model = create_model(opt, 0)
    model.setup(opt)
    model.single_gpu()
    unet = model.netG_A.denoise_fn.model
    live = [rb for rb in unet._res_blocks if rb.dropout]
    data = bench.synth_batch(a.batch, a.size, 1, torch.device("cuda:0"))

    def configure(rate, fused, legacy):
        unet.dropout = rate
        for rb in live:
            rb.dropout = rate
            rb.dropout_rand = (lambda shape, dev: torch.rand(shape, device=dev)) if legacy else None
        unet.jg_fused = fused

    variants = {"dropout 0, fused schedule": (0.0, True, False),
                f"dropout {P_DROP}, fused schedule (unet_fused_drop)": (P_DROP, True, False),
                f"dropout {P_DROP}, module graph, mask in the GroupNorm pass": (P_DROP, False, False),
                f"dropout {P_DROP}, module graph, torch.rand mask per block (before)": (P_DROP, False, True)}

    def step():
        model.set_input(data)
        model.optimize_parameters()

    for v in variants.values():
        configure(*v)
        for _ in range(a.step_warmup):
            step()
        torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, v in variants.items():
            configure(*v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.round_steps):
                step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.round_steps)
    configure(P_DROP, True, False)
    first = next(iter(variants))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return [f"| {k} | {med[k]:.2f} | {min(ms[k]):.2f} - {max(ms[k]):.2f} | {med[k] - med[first]:+.2f} |" for k in variants], len(live), len(unet._res_blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step-warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.warmup >= 10 and a.iters >= 50 and a.step_warmup >= 4 and a.rounds >= 3
    assert torch.cuda.is_available(), "unet_dropout_bench.py measures on the GPU; there is no CPU path"
    B, S = a.batch, a.size
    shapes = [(B, S // 2, S // 2, 64), (B, S // 4, S // 4, 128), (B, S // 8, S // 8, 256)]      # c1 of the three up-blocks (ngf 64, mults 1-2-4-8)
    lines = ["# G_dropout in the diffusion UNet: the up-block kernels and the palette step", "",
             "Command: `python tools/unet_dropout_bench.py " + " ".join(sys.argv[1:]) + "`", "",
             f"{torch.cuda.get_device_name(0)}, bf16, keep = {1 - P_DROP}, SiLU, the mask drawn in the kernels.  HIP events around the launch helpers (output "
             f"allocation included on both sides), {a.warmup} warm-up + {a.iters} timed calls, median (minimum in brackets).  `low-resolution form`: "
             "jg_gn_apply_drop_up2 forward; jg_drop_pool2_bwd + jg_gn_bwd_reduce_ld_acc + jg_gn_bwd_apply at the low resolution backward.  `composed`: "
             "jg_upsample2x_ld + jg_gn_apply_drop forward; jg_gn_bwd_reduce_drop + jg_gn_bwd_apply_drop on the upsampled tensor + jg_pool2x2_ld backward.  "
             "The tensor is the LOW-resolution conv1 output of an up-block; MB: the 16-bit bytes the form must move.", "",
             "| c1 | direction | low-resolution form | composed | composed / low-resolution |", "|---|---|---|---|---|"]
    for shape in shapes:
        lines += kernel_rows(a, shape)
    if not a.no_step:
        rows, n_live, n_all = step_rows(a)
        lines += ["", f"One `optimize_parameters()` of palette_model at the shape of bench.py (efficient UNet, ngf 64, mults 1-2-4-8, batch {B}, {S} x {S}, bf16, "
                  f"set_input on a device-resident batch included) on one model; the rate reaches {n_live} of its {n_all} ResBlocks (the middle block, as in "
                  f"the reference's UNet).  {a.step_warmup} warm-up steps per configuration, then {a.rounds} rounds that time {a.round_steps} steps of each "
                  "configuration in turn (host clock around steps that end in a device synchronise).", "",
                  "| configuration | ms per step (median of rounds) | spread over rounds | difference to dropout 0 |", "|---|---|---|---|"]
        lines += rows
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
