"""HIP-event timing of the super-resolution conditioning pass: ops.lowres_roundtrip (one launch, csrc/resize_aa.hip) against the same
round trip as torch's own device `F.interpolate(..., antialias=True)` pair, same process, same box.  Median of the timed calls.

    python tools/superres_roundtrip_bench.py [--batch 32] [--size 256] [--scale 4] [--warmup 20] [--iters 100] [--out FILE.md]
        [--bench-line FILE.json]     (a bench.py result line of the same box, quoted for context)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    ap.add_argument("--bench-line", default="")
    a = ap.parse_args()
    assert a.warmup >= 10 and a.iters >= 50

    from joligen_amd import ops, resize_aa

    S, lo = a.size, resize_aa.low_size(a.size, a.scale)
    x = torch.rand(a.batch, a.channels, S, S, device="cuda") * 2 - 1
    y = torch.empty_like(x)

    def fused():
        ops.lowres_roundtrip(x, (lo, lo), out=y)

    def aten():
        return F.interpolate(F.interpolate(x, size=(lo, lo), mode="bilinear", antialias=True, align_corners=False), size=(S, S),
                             mode="bilinear", antialias=True, align_corners=False)

    err = float((ops.lowres_roundtrip(x, (lo, lo)) - aten()).abs().max())
    t_f, tmin_f = timed(fused, a.warmup, a.iters)
    t_a, tmin_a = timed(aten, a.warmup, a.iters)
    nbytes = 2 * x.numel() * 4
    band = resize_aa.band_rows(S, S, lo, lo)
    lines = [
        f"# Super-resolution conditioning pass: {a.batch} x {a.channels} x {S} x {S} fp32, scale {a.scale:g} (low resolution {lo} x {lo})",
        "",
        f"HIP events around each call, {a.warmup} warm-up + {a.iters} timed calls, median (minimum in brackets); {torch.cuda.get_device_name(0)}.",
        f"Band of the fused kernel: {band} output rows per workgroup.  max |fused - ATen| on this input: {err:.2e}.",
        "",
        "| path | launches | time per call | GB/s over the algorithmic 2 B C H W 4 bytes |",
        "|---|---|---|---|",
        f"| `ops.lowres_roundtrip` (`jg_lowres_roundtrip_f32`) | 1 | {t_f * 1e3:.1f} us ({tmin_f * 1e3:.1f}) | {nbytes / t_f / 1e6:.0f} |",
        f"| ATen `F.interpolate(antialias=True)` down + up | 2 | {t_a * 1e3:.1f} us ({tmin_a * 1e3:.1f}) | {nbytes / t_a / 1e6:.0f} |",
        "",
        f"ratio fused / ATen: {t_f / t_a:.3f}",
    ]
    if a.bench_line and os.path.exists(a.bench_line):
        with open(a.bench_line) as f:
            txt = [l for l in f.read().splitlines() if l.startswith("{")]
        if txt:
            r = json.loads(txt[-1])
            keep = {k: r[k] for k in ("metric", "value", "unit", "images_per_s", "step_ms", "batch", "size", "dtype") if k in r}
            lines += ["", "bench.py line of the same box, same visit (context): `" + json.dumps(keep or {k: r[k] for k in list(r)[:6]}) + "`"]
    out = "\n".join(lines) + "\n"
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0 if t_f <= t_a else 1


if __name__ == "__main__":
    sys.exit(main())
