#!/usr/bin/env python3
"""ConvTranspose2d(k=2, s=2) on srk_tconv.hip against PyTorch's on the same GPU; prints ONE JSON line.

  per shape  srk_tconv2x2_fwd / _dgrad / _wgrad (incl. its split-K reduce) against F.conv_transpose2d and its autograd input
             gradient / weight+bias gradient; FLOP and the HBM bytes each call must move, and the roofline bound
             max(FLOP / 155 TFLOP/s fp32 matrix, bytes / 6.3 TB/s copy bandwidth) with the fraction of it each kernel reaches
  step       one whole Stepper.gan_step of a fully_tconv_upsample generator (23 RRDBs, 64^2 -> 256^2, batch 32) with the
             upsampling stages on srk_tconv2x2 and, alternating in the same process, on nn.ConvTranspose2d (the same parameters)
Random inputs; HIP-event timing, median of --reps after --warmup."""
import argparse, importlib, json, os, sys
import torch
import torch.nn as nn
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sr = importlib.import_module("super-resolution_amd")
L = sr._lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--step-reps", type=int, default=6)
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
PEAK_FLOPS, PEAK_BW = 155e12, 6.3e12


def med_ms(fn, reps=None, warmup=None):
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    ts = []
    for _ in range(args.reps if reps is None else reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


SHAPES = {  # name: N, H, W, F
    "jets_40to80_f64_b64": (64, 40, 40, 64),
    "c2_64to128_f64_b32": (32, 64, 64, 64),
    "c2_128to256_f64_b32": (32, 128, 128, 64),
    "g16_40to80_f16_b64": (64, 40, 40, 16),
}

res = {"metric": "tconv2x2", "peaks": {"fp32_matrix_tflops": PEAK_FLOPS / 1e12, "copy_TBps": PEAK_BW / 1e12}, "shapes": {}}
for name, (N, H, W, Fc) in SHAPES.items():
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(N, Fc, H, W, device=dev, generator=g)
    w = torch.randn(Fc, Fc, 2, 2, device=dev, generator=g) / (2 * Fc) ** 0.5
    b = torch.randn(Fc, device=dev, generator=g)
    dy = torch.randn(N, Fc, 2 * H, 2 * W, device=dev, generator=g)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    flop = 2.0 * N * H * W * Fc * 4 * Fc
    nbytes = 4.0 * (x.numel() + dy.numel())          # every call reads or writes one x-sized and one y-sized tensor
    bound_us = max(flop / PEAK_FLOPS, nbytes / PEAK_BW) * 1e6
    r = {"N": N, "H": H, "W": W, "F": Fc, "gflop": round(flop / 1e9, 3), "mbytes": round(nbytes / 1e6, 2),
         "bound_us": round(bound_us, 2), "bound": "flop" if flop / PEAK_FLOPS > nbytes / PEAK_BW else "bytes"}
    r["srk_fwd_us"] = med_ms(lambda: L.tconv2x2_fwd_flat(x, w, b, y)) * 1e3
    r["srk_dgrad_us"] = med_ms(lambda: L.tconv2x2_dgrad_flat(dy, w, dx)) * 1e3
    r["srk_wgrad_us"] = med_ms(lambda: L.tconv2x2_wgrad_flat(x, dy, dw, db)) * 1e3
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    with torch.no_grad():
        r["torch_fwd_us"] = med_ms(lambda: F.conv_transpose2d(x, w, b, stride=2)) * 1e3
    yr = F.conv_transpose2d(xr, wr, br, stride=2)
    r["torch_dgrad_us"] = med_ms(lambda: torch.autograd.grad(yr, [xr], dy, retain_graph=True)) * 1e3
    r["torch_wgrad_us"] = med_ms(lambda: torch.autograd.grad(yr, [wr, br], dy, retain_graph=True)) * 1e3
    r["torch_bwd_us"] = med_ms(lambda: torch.autograd.grad(yr, [xr, wr, br], dy, retain_graph=True)) * 1e3
    # same results as PyTorch's (fp32 both; different summation orders)
    L.tconv2x2_fwd_flat(x, w, b, y)
    L.tconv2x2_dgrad_flat(dy, w, dx)
    L.tconv2x2_wgrad_flat(x, dy, dw, db)
    gx, gw, gb = torch.autograd.grad(yr, [xr, wr, br], dy)
    rel = lambda a, c: ((a - c).abs().max() / c.abs().max()).item()
    r["rel_diff_vs_torch"] = {"y": rel(y, yr.detach()), "dx": rel(dx, gx), "dw": rel(dw, gw), "db": rel(db, gb)}
    for k in ("fwd", "dgrad", "wgrad"):
        r[f"srk_{k}_us"] = round(r[f"srk_{k}_us"], 2)
        r[f"srk_{k}_frac_of_bound"] = round(bound_us / r[f"srk_{k}_us"], 3)
        r[f"torch_{k}_us"] = round(r[f"torch_{k}_us"], 2)
        r[f"speedup_{k}"] = round(r[f"torch_{k}_us"] / r[f"srk_{k}_us"], 2)
    r["torch_bwd_us"] = round(r["torch_bwd_us"], 2)
    res["shapes"][name] = r
    del x, w, b, dy, y, dx, dw, db, xr, wr, br, yr, gx, gw, gb
    torch.cuda.empty_cache()

if not args.skip_step:
    train = importlib.import_module("super-resolution_amd.train")
    torch.manual_seed(0)
    st = train.Stepper(workload="gan", res_blocks=23, filters=64, device=dev, hr=256, factor=4, fully_tconv_upsample=True)
    g = torch.Generator(device=dev).manual_seed(3)
    hr = 10 * torch.rand(32, 1, 256, 256, device=dev, generator=g) * (torch.rand(32, 1, 256, 256, device=dev, generator=g) < 0.1)
    lr = sr.SumPool2d(4)(hr)
    stages = [m for m in st.generator.upsampling if isinstance(m, nn.ConvTranspose2d)]
    assert len(stages) == 2

    def on(cls):
        for m in stages:
            m.__class__ = cls           # same parameters, same optimizer state: only the forward (and so the backward) changes

    step = lambda: st.gan_step(lr, hr)
    times = {"srk": [], "torch": []}
    for cls in (sr.ConvTranspose2x2, nn.ConvTranspose2d):
        on(cls)
        med_ms(step, reps=1, warmup=2)
    for _ in range(args.step_reps):     # alternate the two forms
        for key, cls in (("srk", sr.ConvTranspose2x2), ("torch", nn.ConvTranspose2d)):
            on(cls)
            times[key].append(med_ms(step, reps=1, warmup=0))
    on(sr.ConvTranspose2x2)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    res["gan_step_fully_tconv_r23_b32_64to256"] = {"srk_ms": round(med["srk"], 2), "torch_tconv_ms": round(med["torch"], 2),
                                                    "srk_all_ms": [round(t, 2) for t in times["srk"]],
                                                    "torch_all_ms": [round(t, 2) for t in times["torch"]]}
print(json.dumps(res))
