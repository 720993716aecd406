#!/usr/bin/env python3
"""Jet-observable evaluation (evaluation.distribution's device loop) on the MI355X; prints ONE JSON line.

  kernels  srk_eval_image_stats for the four kinds (SR, HR 80^2; LR, LR_gen 40^2) + srk_eval_pixel_counts (meanimg), batch 512,
           the reference's default eval_modes (E_1 ... E_30, meanimg): images/s and the GB/s of one read of every image
  jets     the eval loop per batch at the jets' default geometry (residual_blocks 10, 40^2 -> 80^2, batch 256): generator
           forward (eval, no_grad) + SumPool2d + the observable launches, and the observables' share of it
  c2       the same loop at configs[2]'s generator (23 RRDBs, 64^2 -> 256^2, batch 32): HR px/s in eval mode
Random-init generators, synthetic jet-like LR inputs; HIP-event timing, median of --reps after --warmup."""
import argparse, importlib, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sr = importlib.import_module("super-resolution_amd")
obs = sr.observables

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--skip-c2", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
MODES = [f"E_{i}" for i in range(1, 31)] + ["meanimg"]


def med_ms(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def jets(B, H, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return 10 * torch.rand(B, 1, H, H, device=dev, generator=g) * (torch.rand(B, 1, H, H, device=dev, generator=g) < 0.1)


res = {"metric": "eval_observables", "modes": "E_1..E_30+meanimg"}
specs = obs.parse_modes(MODES)
pool2 = sr.SumPool2d(2)

# ---- kernels alone
B = 512
hr = jets(B, 80, 1)
srimg = (hr + 0.05 * torch.rand_like(hr)).contiguous()
kinds = [srimg, hr, pool2(hr), pool2(srimg)]
col = obs.Collector(specs, 2)
def kernels():
    col.add(kinds)
    for r in col.recs:                      # keep the records from piling up across reps
        r.parts.clear(); r.sizes.clear()
ms = med_ms(kernels)
nbytes = sum(x.numel() * 4 for x in kinds)
res["kernels_ms"] = round(ms, 4)
res["kernels_images_per_s"] = round(4 * B / (ms * 1e-3))
res["kernels_GBps_one_read"] = round(nbytes / (ms * 1e-3) / 1e9, 1)


def loop(gen, lr, f):
    pool = sr.SumPool2d(f)
    c = obs.Collector(specs, f)
    hr_ = jets(lr.shape[0], lr.shape[2] * f, 7)
    def step_full():
        with torch.no_grad():
            y = gen(lr)
            c.add([y, hr_, lr, pool(y)])
            for r in c.recs:
                r.parts.clear(); r.sizes.clear()
    def step_gen():
        with torch.no_grad():
            y = gen(lr)
            pool(y)
    return med_ms(step_full), med_ms(step_gen)


# ---- jets geometry
gen = sr.GeneratorRRDB(1, filters=64, num_res_blocks=10, num_upsample=1).to(dev).eval()
lr = jets(256, 40, 3)
full, g_only = loop(gen, lr, 2)
res["jets_loop_ms"], res["jets_generator_pool_ms"] = round(full, 3), round(g_only, 3)
res["jets_observables_share"] = round((full - g_only) / full, 4)
res["jets_hr_px_per_s"] = round(256 * 80 * 80 / (full * 1e-3))
del gen

# ---- configs[2] generator
if not args.skip_c2:
    gen = sr.GeneratorRRDB(1, filters=64, num_res_blocks=23, num_upsample=2).to(dev).eval()
    lr = jets(32, 64, 5)
    full, g_only = loop(gen, lr, 4)
    res["c2_loop_ms"], res["c2_generator_pool_ms"] = round(full, 3), round(g_only, 3)
    res["c2_observables_share"] = round((full - g_only) / full, 4)
    res["c2_eval_hr_px_per_s"] = round(32 * 256 * 256 / (full * 1e-3))
print(json.dumps(res))
