#!/usr/bin/env python3
"""Generate tests/golden/G18_sinkhorn.npz from the reference's own Sinkhorn code (build container only): utils.SinkhornDistance and
utils.cut_smaller, composed as esrgan.py:539-542 composes them, run in float32 and in float64 on the CPU.  Stand-in modules as in
tools/make_golden_eval.py.  Only inputs and outputs are stored; the run is deterministic (rerunning rewrites the same arrays).

Per case ``<name>/...``: inputs, cost / gradients in float32 and float64, the iteration count K, the reference's err_k of every
iteration (float32 run, captured from its ``err.item()`` calls) and ``margin`` = min_k |err_k - 0.1| / 0.1.  The stopping test
compares a float with 0.1, so a case is only kept if that margin is at least MIN_MARGIN in both precisions and both stop at the
same K: the seed of a case is advanced until it is.

Cases:
  sd_*     SinkhornDistance(eps, max_iter, reduction)(x, y) with x (B, N, 1), y (B, M, 1) or unbatched (N, 1) / (M, 1):
           B = 1, B > 1, unbatched; N != M; reductions none / mean / sum; eps 0.1 and 1; stopped by max_iter and stopped early.
           Gradients: of cost.sum() w.r.t. x and y.
  wl_*     the fused head: SinkhornDistance(eps, 100, 'sum')(cut_smaller(sort(gen))[..., None], cut_smaller(sort(real))[..., None])[0]
           on jet-like images [B, 1, H, W]: ties among the kept values (quantised energies) and an all-zero generated batch
           (cut_smaller keeps the whole row).  Gradient w.r.t. gen.
"""
import os
import sys
sys.dont_write_bytecode = True
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("reference not present")

for name in ["torchvision", "torchvision.transforms", "torchvision.utils", "torchvision.datasets", "h5py", "energyflow",
             "energyflow.emd", "pyjet"]:
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)
sys.modules["energyflow"].emd = sys.modules["energyflow.emd"]
os.chdir(REF)
sys.path.insert(0, REF)
import matplotlib  # noqa: E402
matplotlib.use("Agg")
import utils as rutils  # noqa: E402  (the reference, read-only)

MIN_MARGIN = 1e-3
THRESH = 0.1


def run_ref(fn):
    """Run fn() and capture the reference's per-iteration err (its only .item() calls)."""
    rec = []
    orig = torch.Tensor.item

    def item(self):
        v = orig(self)
        rec.append(v)
        return v
    torch.Tensor.item = item
    try:
        out = fn()
    finally:
        torch.Tensor.item = orig
    return out, rec


def margin(errs):
    return min(abs(e - THRESH) / THRESH for e in errs)


def sd_case(x, y, eps, max_iter, reduction):
    res = {}
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        xt = torch.tensor(x, dtype=dt, requires_grad=True)
        yt = torch.tensor(y, dtype=dt, requires_grad=True)
        (cost, pi, C), errs = run_ref(lambda: rutils.SinkhornDistance(eps, max_iter, reduction)(xt, yt))
        cost.sum().backward()
        res["cost" + tag] = cost.detach().numpy().astype(np.float64)
        res["gx" + tag] = xt.grad.numpy().astype(np.float64)
        res["gy" + tag] = yt.grad.numpy().astype(np.float64)
        res["K" + tag] = len(errs)
        res["err" + tag] = np.array(errs, np.float64)
        res["pi_shape"] = np.array(pi.shape, np.int64)
        res["C_shape"] = np.array(C.shape, np.int64)
        res["cost_shape"] = np.array(cost.shape, np.int64)
    return res


def wl_case(gen, real, eps, max_iter=100):
    res = {}
    B = gen.shape[0]
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        g = torch.tensor(gen, dtype=dt, requires_grad=True)
        r = torch.tensor(real, dtype=dt)

        def f():
            gen_sort, _ = torch.sort(g.view(B, -1), 1)
            real_sort, _ = torch.sort(r.view(B, -1), 1)
            return rutils.SinkhornDistance(eps, max_iter, 'sum')(rutils.cut_smaller(gen_sort)[..., None],
                                                                rutils.cut_smaller(real_sort)[..., None])[0]
        loss, errs = run_ref(f)
        loss.backward()
        res["loss" + tag] = np.float64(loss.item())
        res["ggen" + tag] = g.grad.numpy().astype(np.float64)
        res["K" + tag] = len(errs)
        res["err" + tag] = np.array(errs, np.float64)
    return res


def accept(res):
    ok = res["K32"] == res["K64"] and margin(res["err32"]) >= MIN_MARGIN and margin(res["err64"]) >= MIN_MARGIN
    if ok:
        res["margin"] = np.float64(min(margin(res["err32"]), margin(res["err64"])))
    return ok


def points(rng, shape):
    """jet-like energies: mostly small, a few large"""
    return (rng.exponential(0.3, size=shape) * (1 + 4 * (rng.random(shape) < 0.1))).astype(np.float32)


def jet_images(rng, B, H, W, frac, quant=None):
    img = np.zeros((B, 1, H, W), np.float32)
    for b in range(B):
        m = rng.random((H, W)) < frac * (0.5 + rng.random())
        e = rng.exponential(0.4, size=(H, W)).astype(np.float32)
        if quant:
            e = np.ceil(e / quant) * quant
        img[b, 0][m] = e[m]
        img[b, 0][~m] = np.where(rng.random(((~m).sum(),)) < 0.3, -rng.random(((~m).sum(),)) * 0.01, 0.0).astype(np.float32)
    return img


SD_CASES = [   # name, batch shape (None: unbatched), N, M, eps, max_iter, reduction, want: "max_iter" | "early"
    ("sd_b1_sum_eps01", 1, 40, 40, 0.1, 100, "sum", None),
    ("sd_b4_mean_eps01", 4, 60, 45, 0.1, 100, "mean", None),
    ("sd_unbatched_none_eps1", None, 50, 35, 1.0, 100, "none", None),
    ("sd_b3_none_eps1", 3, 30, 70, 1.0, 100, "none", None),
    ("sd_b2_sum_maxiter", 2, 64, 48, 0.1, 6, "sum", "max_iter"),
    ("sd_b2_mean_early", 2, 24, 32, 1.0, 100, "mean", "early"),
]


def main():
    out = {}
    for name, B, N, M, eps, max_iter, red, want in SD_CASES:
        seed = 0
        while True:
            rng = np.random.default_rng(1800 + 97 * seed + sum(map(ord, name)))
            shx = (N, 1) if B is None else (B, N, 1)
            shy = (M, 1) if B is None else (B, M, 1)
            x, y = points(rng, shx), points(rng, shy)
            res = sd_case(x, y, eps, max_iter, red)
            stopped_early = res["K32"] < max_iter
            if accept(res) and (want is None or (want == "early") == stopped_early):
                break
            seed += 1
            assert seed < 200, name
        out[name] = dict(x=x, y=y, eps=np.float64(eps), max_iter=np.int64(max_iter), reduction=np.array(red), seed=np.int64(seed), **res)
        print(f"{name}: K={res['K32']} margin={res['margin']:.3g} cost32={res['cost32']} seed={seed}")
    WL_CASES = [("wl_jets", 4, 20, 20, 0.3, None, 0.1, False), ("wl_ties", 3, 16, 16, 0.4, 0.25, 0.1, False),
                ("wl_zero_gen", 2, 12, 12, 0.3, None, 1.0, True)]
    for name, B, H, W, frac, quant, eps, zero_gen in WL_CASES:
        seed = 0
        while True:
            rng = np.random.default_rng(1900 + 97 * seed + sum(map(ord, name)))
            real = jet_images(rng, B, H, W, frac, quant)
            gen = np.zeros_like(real) if zero_gen else jet_images(rng, B, H, W, frac, quant)
            res = wl_case(gen, real, eps)
            if accept(res):
                break
            seed += 1
            assert seed < 200, name
        out[name] = dict(gen=gen, real=real, eps=np.float64(eps), max_iter=np.int64(100), seed=np.int64(seed), **res)
        print(f"{name}: K={res['K32']} margin={res['margin']:.3g} loss32={res['loss32']} seed={seed}")
    flat = {f"{c}/{k}": np.asarray(v) for c, d in out.items() for k, v in d.items()}
    path = os.path.join(ROOT, "tests", "golden", "G18_sinkhorn.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
