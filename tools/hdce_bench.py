"""HIP-event timing of the SRC_hDCE loss: (1) the fused kernel (`jg_nce_hdce`, csrc/nce.hip) forward and backward against the same math composed
from ATen element-wise / reduction ops on the same Gram matrices (both sides get S = q k^T and G = k k^T from `ops.sgemm`), at the contrastive
problem set of the benchmarked CUT shape: 2 terms x 4 layers x batch 16 problems of P = 256 patches, 256 features, the NCE term weighted and the
identity term not; (2) the whole CUT step (resnet_9blocks G + basic D, 256 x 256, batch 16, bf16) with alg_cut_nce_loss = SRC_hDCE against the
same step with patchnce, same process, same box.  Median of the timed calls.

    python tools/hdce_bench.py [--batch 16] [--layers 4] [--patches 256] [--dim 256] [--warmup 20] [--iters 100] [--steps 30] [--no-step] [--out FILE.md]
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


def aten_forward(S, G, mask, eye, T, gamma):
    """weights, logits, A and the loss value from the two Gram matrices (what the fused forward computes)"""
    rinv = 1.0 / (torch.diagonal(G, dim1=1, dim2=2).sqrt() + 1e-7)
    Gh = G * rinv[:, :, None] * rinv[:, None, :]
    m = Gh.masked_fill(eye, float("-inf")).amax(dim=2, keepdim=True)
    w = torch.where(mask, torch.exp((Gh - m) / gamma), torch.ones_like(Gh))
    a = (S * w / T).masked_fill(eye, -10.0 / T)
    A = torch.logsumexp(a, dim=2)
    pos = torch.diagonal(S, dim1=1, dim2=2) / T
    return torch.nn.functional.softplus(A - pos), w, a, A


def aten_backward(w, a, A, grow, eye, T):
    dS = (grow[:, :, None] * torch.exp(a - A[:, :, None]) * w / T).masked_fill(eye, 0.0)
    return dS, -grow / T


def step_ms(nce_loss, batch, size, warmup, steps):
    import random

    from joligen_amd.models import create_model
    from joligen_amd.options import opt_from_json

    ov = dict(model_type="cut", G_netG="resnet", G_ngf=64, G_nblocks=9, D_netDs=["basic"], D_ndf=64, data_crop_size=size, data_load_size=size,
              train_batch_size=batch, train_iter_size=1, train_optim="adam", train_G_ema=True, train_G_ema_beta=0.999, gpu_ids="0", jg_act_dtype="bf16",
              alg_cut_nce_loss=nce_loss)
    torch.manual_seed(0)
    random.seed(0)
    model = create_model(opt_from_json({}, ov), 0)
    g = torch.Generator().manual_seed(1)
    data = {"A": (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda(), "B": (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda()}
    model.data_dependent_initialize(data)
    model.setup(model.opt)
    model.single_gpu()

    def step():
        model.set_input(data)
        model.optimize_parameters()

    t, tmin = timed(step, warmup, steps)
    out = (t, tmin, model.step_driver, float(model.loss_G_NCE), float(model.loss_G_NCE_Y))
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.warmup >= 10 and a.iters >= 50

    from joligen_amd import _lib, ops

    B, P, D, T, gamma = a.batch, a.patches, a.dim, 0.07, 1.0
    nimg, wperiod, wcount = 2 * a.layers * B, 2 * B, B
    g = torch.Generator().manual_seed(0)
    k = torch.nn.functional.normalize(torch.randn(nimg * P, D, generator=g)).cuda()
    q = torch.nn.functional.normalize(k + 0.5 * torch.randn(nimg * P, D, generator=g).cuda())
    grow = torch.rand(nimg * P, generator=g).cuda()
    S, G = torch.empty(nimg, P, P, device="cuda"), torch.empty(nimg, P, P, device="cuda")
    bstr = (P * D, P * D, P * P)

    def gemms():
        ops.sgemm(q, k, S, P, P, D, (D, 1), (D, 1), (P, 1), nimg, bstr)
        ops.sgemm(k, k, G, P, P, D, (D, 1), (D, 1), (P, 1), nimg, bstr)

    gemms()
    L = _lib.lib()
    stats, loss = torch.empty(3, nimg * P, device="cuda"), torch.empty(nimg * P, device="cuda")
    dS, gpos = torch.empty_like(S), torch.empty(nimg * P, device="cuda")

    def fused_fwd():
        _lib.check(L.jg_nce_hdce(S.data_ptr(), G.data_ptr(), stats.data_ptr(), loss.data_ptr(), None, None, None, None, nimg, P, T, gamma, wperiod, wcount,
                                 ops._st()), "jg_nce_hdce")

    def fused_bwd():
        _lib.check(L.jg_nce_hdce(S.data_ptr(), G.data_ptr(), stats.data_ptr(), None, dS.data_ptr(), gpos.data_ptr(), grow.data_ptr(), None, nimg, P, T, gamma,
                                 wperiod, wcount, ops._st()), "jg_nce_hdce")

    eye = torch.eye(P, dtype=torch.bool, device="cuda")[None]
    mask = torch.tensor([(b % wperiod) < wcount for b in range(nimg)], device="cuda").view(nimg, 1, 1)
    grow2 = grow.view(nimg, P)
    with torch.no_grad():
        fused_fwd()
        fused_bwd()
        l_a, w_a, a_a, A_a = aten_forward(S, G, mask, eye, T, gamma)
        dS_a, _ = aten_backward(w_a, a_a, A_a, grow2, eye, T)
        err_l = float((loss.view(nimg, P) - l_a).norm() / l_a.norm())
        err_d = float((dS - dS_a).norm() / dS_a.norm())
        t_ff, m_ff = timed(fused_fwd, a.warmup, a.iters)
        t_fb, m_fb = timed(fused_bwd, a.warmup, a.iters)
        t_af, m_af = timed(lambda: aten_forward(S, G, mask, eye, T, gamma), a.warmup, a.iters)
        t_ab, m_ab = timed(lambda: aten_backward(w_a, a_a, A_a, grow2, eye, T), a.warmup, a.iters)
        t_g, m_g = timed(gemms, a.warmup, a.iters)

    def whole():
        qd, kd = q.detach().requires_grad_(True), k.detach().requires_grad_(True)
        (ops.patch_hdce_loss(qd, kd, nimg, T, gamma, wperiod, wcount) * grow).sum().backward()

    t_w, m_w = timed(whole, a.warmup, a.iters)
    mat = nimg * P * P * 4
    frac = wcount / wperiod
    by_f, by_b = mat * (1 + frac), mat * (2 + frac)
    lines = [
        f"# SRC_hDCE loss: {nimg} problems (2 terms x {a.layers} layers x batch {B}), P = {P} patches, {D} features, T = {T}, gamma = {gamma}; "
        f"problems with (b % {wperiod}) < {wcount} weighted",
        "",
        f"HIP events around each call, {a.warmup} warm-up + {a.iters} timed calls, median (minimum in brackets); {torch.cuda.get_device_name(0)}.",
        f"Fused against ATen on this input: loss {err_l:.2e}, dS {err_d:.2e} (relative, in norm).",
        "",
        "| part | launches | time per call | GB/s over S (+ G of the weighted half) (+ dS) |",
        "|---|---|---|---|",
        f"| fused forward (`jg_nce_hdce`, dS = NULL) | 1 | {t_ff * 1e3:.1f} us ({m_ff * 1e3:.1f}) | {by_f / t_ff / 1e6:.0f} |",
        f"| fused backward (`jg_nce_hdce`, dS) | 1 | {t_fb * 1e3:.1f} us ({m_fb * 1e3:.1f}) | {by_b / t_fb / 1e6:.0f} |",
        f"| ATen forward from the same S, G (weights, logits, logsumexp, value) | ~20 | {t_af * 1e3:.1f} us ({m_af * 1e3:.1f}) | {by_f / t_af / 1e6:.0f} |",
        f"| ATen backward from saved w, a, A (dS, gpos) | ~8 | {t_ab * 1e3:.1f} us ({m_ab * 1e3:.1f}) | {by_b / t_ab / 1e6:.0f} |",
        f"| the two Gram GEMMs (`jg_sgemm`, both sides) | 2 | {t_g * 1e3:.1f} us ({m_g * 1e3:.1f}) | |",
        f"| `ops.patch_hdce_loss` forward + backward (3 + 4 launches incl. GEMMs, autograd) | 7 | {t_w * 1e3:.1f} us ({m_w * 1e3:.1f}) | |",
        "",
        f"ratio fused / ATen: forward {t_ff / t_af:.3f}, backward {t_fb / t_ab:.3f}, both {(t_ff + t_fb) / (t_af + t_ab):.3f}",
    ]
    if not a.no_step:
        rows = [(n, *step_ms(n, B, a.size, a.warmup, a.steps)) for n in ("patchnce", "SRC_hDCE", "patchnce")]
        lines += ["", f"## Whole CUT step: resnet_9blocks G + basic D + mlp_sample F, {a.size} x {a.size}, batch {B}, bf16, nce_layers 0,4,8,12,16",
                  "", f"{a.warmup} warm-up + {a.steps} timed `optimize_parameters()`, HIP events, median (minimum); the patchnce step is run before and after.",
                  "", "| alg_cut_nce_loss | step | step_driver | G_NCE / G_NCE_Y of the last step |", "|---|---|---|---|"]
        lines += [f"| {n} | {t:.2f} ms ({tm:.2f}) | {drv} | {l1:.3f} / {l2:.3f} |" for n, t, tm, drv, l1, l2 in rows]
        base = 0.5 * (rows[0][1] + rows[2][1])
        lines += ["", f"SRC_hDCE - patchnce: {rows[1][1] - base:+.3f} ms per step ({(rows[1][1] / base - 1) * 100:+.2f} %); the two patchnce runs differ by "
                      f"{abs(rows[0][1] - rows[2][1]):.3f} ms."]
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0 if t_ff + t_fb <= t_af + t_ab else 1


if __name__ == "__main__":
    sys.exit(main())
