"""HIP-event timing of the cm_gan seam: ops.cm_gan_head (jg_cm_gan_head forward, jg_cm_gan_head_bwd backward: one launch each,
csrc/elementwise.hip) beside the composition of the ops that existed before it on the same tensors -- forward ops.cm_loss + ops.cm_combine +
ops.to_nhwc, backward ops.axpby of the saved gradient + a per-sample scale of dpred by c_out + the add of the two contributions -- and one
optimize_parameters() of cm_gan (the example's discriminators: projected_d + basic) beside cm at the BASELINE configs[4] shape.
Same process, same box; median of the timed calls.

    python tools/cm_gan_bench.py [--batch 32] [--size 256] [--channels 3] [--dtype bf16] [--warmup 20] [--iters 100]
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


def step_model(model_type, batch, size, dtype_name):
    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    opt = opt_from_json({}, dict(model_type=model_type, G_ngf=64, G_unet_mha_channel_mults=[1, 2, 4, 8], G_unet_mha_res_blocks=[2, 2, 2, 2],
                                 G_unet_mha_attn_res=[16], G_unet_mha_vit_efficient=True, data_crop_size=size, train_batch_size=batch,
                                 gpu_ids="0", jg_act_dtype=dtype_name, train_optim="adamw", train_G_ema=True, train_iter_size=1,
                                 checkpoints_dir="/tmp/jg_amd_ckpt/", name="cm_gan_bench"))
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
    dpred = (torch.randn(B, S, S, 8, device=d, generator=g) * 1e-2).to(dtype)
    gl = torch.tensor(0.5, device=d)
    co4 = v[1].view(B, 1, 1, 1).to(dtype)

    def fused_fwd():
        return ops.cm_gan_head(Fn, Fc, noisy_n, noisy_c, v[0], v[1], v[2], v[3], mask, v[4], 1.0, 1.0)

    def composed_fwd():
        loss = ops.cm_loss(Fn, Fc, noisy_n, noisy_c, v[0], v[1], v[2], v[3], mask, v[4], 1.0, 1.0)
        return loss, ops.to_nhwc(ops.cm_combine(noisy_n, Fn.detach(), v[0], v[1]), dtype, 8)

    loss, _ = fused_fwd()
    dFn = loss.grad_fn.saved_tensors[0]

    def fused_bwd():
        return ops._cm_gan_head_bwd_launch(dFn, dpred, gl, v[1], C)

    def composed_bwd():
        return ops.axpby(dFn, 1.0, alpha_dev=gl) + dpred * co4

    res = {k: timed(f, a.warmup, a.iters) for k, f in (("ff", fused_fwd), ("cf", composed_fwd), ("fb", fused_bwd), ("cb", composed_bwd))}
    px = B * S * S
    mb = lambda per_px: per_px * px / 1e6
    f_fwd, c_fwd = 2 * 16 + 2 * 4 * C + 8 + 2 * 16, (2 * 16 + 2 * 4 * C + 8 + 16) + (4 * C + 16 + 4 * C) + (4 * C + 16)
    f_bwd, c_bwd = 3 * 16, 2 * 16 + 2 * 16 + 3 * 16
    row = lambda name, launches, key, per_px: (f"| {name} | {launches} | {mb(per_px):.1f} MB ({per_px} B/pixel) | {res[key][0] * 1e3:.1f} us ({res[key][1] * 1e3:.1f}) | "
                                               f"{mb(per_px) / res[key][0]:.0f} |")
    rf, rb = res["ff"][0] / res["cf"][0], res["fb"][0] / res["cb"][0]
    lines = [
        f"# cm_gan seam kernels: batch {B}, {C} x {S} x {S}, {a.dtype} UNet outputs (Cpad 8), int64 label mask",
        "",
        f"HIP events around each call (the Python wrappers included: output allocations, the zeroing of the loss accumulator), {a.warmup} warm-up + "
        f"{a.iters} timed calls, median (minimum in brackets); {torch.cuda.get_device_name(0)}.  Bytes are the algorithmic traffic of each path "
        "(every operand read once, every result written once per launch).",
        "",
        "| path | launches | bytes moved | time per call | GB/s |",
        "|---|---|---|---|---|",
        row("forward fused: `ops.cm_gan_head` (`jg_cm_gan_head`)", "1 (+ memset)", "ff", f_fwd),
        row("forward composed: `ops.cm_loss` + `ops.cm_combine` + `ops.to_nhwc`", "3 (+ memset)", "cf", c_fwd),
        row("backward fused: `jg_cm_gan_head_bwd`", "1", "fb", f_bwd),
        row("backward composed: `ops.axpby` + per-sample scale + add", "3", "cb", c_bwd),
        "",
        f"ratio fused / composed: forward {rf:.2f} (bytes {f_fwd / c_fwd:.2f}), backward {rb:.2f} (bytes {f_bwd / c_bwd:.2f})",
        f"the fused path is {'NOT slower' if rf <= 1.0 and rb <= 1.0 else 'SLOWER'} than the composition (median, same process)",
    ]
    if not a.no_step:
        steps = {}
        for mt in ("cm", "cm_gan"):
            model, step = step_model(mt, a.step_batch, S, a.dtype)
            steps[mt] = timed(step, a.step_warmup, a.step_iters)
            del model, step
            torch.cuda.empty_cache()
        lines += ["", f"One `optimize_parameters()` (set_input on a device-resident batch included) at the configs[4] shape (unet_mha ngf 64, mults "
                  f"[1,2,4,8], 2 res-blocks per level, mid-block attention, {S} x {S}), batch {a.step_batch}, {a.dtype}, {a.step_warmup} warm-up + "
                  f"{a.step_iters} timed steps, median (minimum); cm_gan with D_netDs = [projected_d (random-initialised backbone), basic]:", "",
                  "| model_type | ms per step |", "|---|---|"]
        lines += [f"| `{mt}` | {steps[mt][0]:.2f} ({steps[mt][1]:.2f}) |" for mt in ("cm", "cm_gan")]
        lines += ["", f"ratio cm_gan / cm: {steps['cm_gan'][0] / steps['cm'][0]:.3f} (recorded, not bounded: cm_gan adds the generator-side forward and "
                  "backward of both discriminators and their own training step)"]
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
