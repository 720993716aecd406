#!/usr/bin/env python3
"""Time the fused Sinkhorn head (losses.wasser_loss, csrc/srk_sinkhorn.hip) forward + backward at the jet geometry (B = 8, 80^2)
with controlled positive counts N' ~ 150 / 1600 / 3200 / 6400, against an ATen restatement of the same math on the GPU (our own
code: explicit N' x M' cost matrix, logsumexp iterations, autograd through them).  The restatement runs exactly the K iterations
the HIP path ran on the same input (K-matched; it skips the err test, which would cost a host sync per iteration).  Records K, time
per call and peak memory; an out-of-memory restatement is reported as "OOM".

    python tools/bench_sinkhorn.py [--reps 5] [--out profiles/r06_bench_sinkhorn.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sr = importlib.import_module("super-resolution_amd")
DEV = torch.device("cuda")


def images(B, HW, npos, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(B, HW * HW)
    for b in range(B):
        k = max(1, int(npos * (0.8 + 0.2 * b / max(B - 1, 1))))
        sel = torch.randperm(HW * HW, generator=g)[:k]
        img[b, sel] = torch.rand(k, generator=g) * 2 + 0.01
    return img.reshape(B, 1, HW, HW).to(DEV)


def aten_wasser(gen, real, eps, iters):
    B = gen.shape[0]
    gs, _ = torch.sort(gen.view(B, -1), 1)
    rs, _ = torch.sort(real.view(B, -1), 1)
    n = int((gs > 0).sum(1).max()) or gs.shape[1]
    m = int((rs > 0).sum(1).max()) or rs.shape[1]
    x, y = gs[:, -n:], rs[:, -m:]
    C = (x[:, :, None] - y[:, None, :]) ** 2
    a, b = torch.log(torch.tensor(1.0 / n) + 1e-8).item(), torch.log(torch.tensor(1.0 / m) + 1e-8).item()
    u, v = torch.zeros_like(x), torch.zeros_like(y)
    for _ in range(iters):
        u = eps * (a - torch.logsumexp((-C + u[:, :, None] + v[:, None, :]) / eps, -1)) + u
        v = eps * (b - torch.logsumexp((-C + u[:, :, None] + v[:, None, :]) / eps, -2)) + v
    pi = torch.exp((-C + u[:, :, None] + v[:, None, :]) / eps)
    return (pi * C).sum()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for npos in (150, 1600, 3200, 6400):
        gen, real = images(8, 80, npos, 1), images(8, 80, npos, 2)

        def ours(with_bwd=True):
            g = gen.clone().requires_grad_(with_bwd)
            loss, K = sr.losses.wasser_loss(g, real, a.eps, return_iterations=True)
            if with_bwd:
                loss.backward()
            return K
        K = int(ours())
        n = int((gen.view(8, -1) > 0).sum(1).max())
        t_f, m_f = timed(lambda: ours(False), a.reps)
        t_fb, m_fb = timed(ours, a.reps)
        row = dict(npos=npos, n_kept=n, K=K, ours_fwd_ms=t_f, ours_fwd_bwd_ms=t_fb, ours_peak_mb=m_fb,
                   pair_updates_fwd=2 * K * 8 * n * n)
        try:
            def ref():
                g = gen.clone().requires_grad_(True)
                aten_wasser(g, real, a.eps, K).backward()
            t_r, m_r = timed(ref, max(1, a.reps // 2))
            row.update(aten_fwd_bwd_ms=t_r, aten_peak_mb=m_r)
        except torch.OutOfMemoryError:
            row.update(aten_fwd_bwd_ms="OOM", aten_peak_mb="OOM")
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f)


if __name__ == "__main__":
    main()
