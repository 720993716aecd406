#!/usr/bin/env python3
"""Generate tests/golden/G17_observables.npz from the reference's own evaluation code (build container only): seeded jet-like
batches run through evaluation/eval.py's ``MultModeHist`` / ``MultHist.append`` (with its ``SumRaster`` and ``MeanImage``),
the histogram / KL summary computed by ``MultHist.histogram`` and ``KLD_hist`` the way eval.py:598-718 composes them, and an
end-to-end case through the reference ``GeneratorRRDB`` loaded from G10_ref_generator.pth.  Stand-in modules as in
tools/make_golden_heads.py.  Only inputs and outputs are stored; the run is deterministic (rerunning rewrites the same arrays).

Sets (each a list of batches of the four kinds SR, HR, LR, LR_gen = SumPool(SR)):
  jets80, jets40   seeded jet-like batches (SR = HR with sparse positive perturbations), factor 2
  edge             16x16 edge cases: fewer non-zero pixels than the ranks asked for, exact ties among non-zero values, negative
                   pixels, an all-zero image (one batch); an image with a NaN (second batch); a batch of one (third)
  e2e              fixed LR jets 10x10 through the reference generator (factor 4); the LR seed is advanced until no SR / LR_gen value
                   sits within 1e-5 (relative) of a threshold or a histogram edge, and no rank up to 6 within 1e-5 of the next
"""
import io
import os
import sys
sys.dont_write_bytecode = True
import types
import contextlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("reference not present")
sys.path.insert(0, ROOT)
from oracle import esrgan_oracle as O  # noqa: E402

for name in ["torchvision", "torchvision.transforms", "torchvision.utils", "torchvision.datasets", "h5py", "energyflow",
             "energyflow.emd", "pyjet"]:
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
sys.modules["torchvision"].datasets = sys.modules["torchvision.datasets"]
sys.modules["torchvision.utils"].save_image = lambda *a, **k: None
sys.modules["torchvision.datasets"].STL10 = object
sys.modules["energyflow"].emd = sys.modules["energyflow.emd"]
os.chdir(REF)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "evaluation"))
import matplotlib  # noqa: E402
matplotlib.use("Agg")
import utils as rutils  # noqa: E402  (the reference, read-only)
import models as rmodels  # noqa: E402
with contextlib.redirect_stdout(io.StringIO()):
    import eval as reval  # noqa: E402

# eval.py:334 calls np.nan_to_num(nnz.mean(), 0): the 0 is the `copy` argument, which NumPy 2 refuses for a scalar (ValueError,
# swallowed by MultHist.append, so meannnz would stay empty).  The fixture records the mode as written for NumPy 1, where the
# flag is ignored for scalars.
_nan_to_num = np.nan_to_num
np.nan_to_num = lambda x, copy=True, *a, **k: _nan_to_num(x, True, *a, **k)

MODES = ['max', 'min', 'mean', 'nnz', 'meannnz', 'E', 'E_1', 'E_2', 'E_5', 'E_10', 'E_30', 'R_12', 'R_25', 'deltaR_12', 'deltaR_13',
         'FWM_1_5', 'FWM_2_10', 'FWM_1_30', 'jetmass', 'hitogram', 'meanimg']
E2E_MODES = ['max', 'mean', 'nnz', 'meannnz', 'E_1', 'E_5', 'R_12', 'deltaR_12', 'FWM_1_5', 'jetmass', 'hitogram', 'meanimg']
THR = 0.002
out = {}


def pool(x, f):
    return O.sum_pool(torch.from_numpy(x), f).numpy()


def kinds(sr, hr, f):
    return [sr, hr, pool(hr, f), pool(sr, f)]


def jets(n_batches, B, H, seed, f):
    batches = []
    for k in range(n_batches):
        _, hr = O.jet_images(B, 1, H, H, seed + k, f)
        g = torch.Generator().manual_seed(1000 + seed + k)
        sr = hr + 3.0 * torch.rand(hr.shape, generator=g) * (torch.rand(hr.shape, generator=g) < 0.05)
        batches.append(kinds(sr.numpy(), hr.numpy(), f))
    return batches


def run_reference(batches, f, modes, meanenergy=False):
    hhd = reval.MultModeHist(modes, factor=f)
    hsum = reval.MultHist(4, 'sum', f)
    hme = reval.MultHist(2, 'meanimg', f, meanenergy=True) if meanenergy else None
    with contextlib.redirect_stdout(io.StringIO()):
        for b in batches:
            T = [torch.from_numpy(np.ascontiguousarray(x)) for x in b]
            hhd.append(*T)
            hsum.append(*T)
            if hme is not None:
                hme.append(*T[:2])
    return hhd, hsum, hme


def kl_summary(hhd, modes, bins, nth):
    """eval.py:598-718 without the plots: total_kld, kld_dict and the histogram entries per kind."""
    total, kd, hists = [], {}, {}
    kldiv = torch.nn.KLDivLoss(reduction='sum')
    for m, mode in enumerate(modes):
        if mode in ('hitogram', 'meanimg'):
            sr, hr = hhd[m].raster.get_hist() if mode == 'hitogram' else hhd[m].meanimg.get_hist()
            sr, hr = .1 + torch.Tensor(sr)[None, None, ...], .1 + torch.Tensor(hr)[None, None, ...]
            total.append(float(kldiv((sr / sr.sum()).log(), hr / (sr.sum()))))
            kd[mode] = float(kldiv((sr / sr.sum()).log(), hr / (sr.sum())))
            continue
        bin_entries, ents = [], []
        for i in range(4):
            if hhd.nums[m] == i:
                continue
            try:
                try:
                    entries, binedges = hhd[m].histogram(hhd[m].list[i], bins)
                except IndexError:
                    continue
                if nth == 'hr':
                    if i < 2:
                        bin_entries.append(entries)
                elif nth == 'lr':
                    if i > 1:
                        bin_entries.append(entries)
                else:
                    bin_entries.append(entries)
            except ValueError:
                entries, binedges = hhd[m].histogram(hhd[m].list[i], bins, auto_range=False)
            ents.append((entries, binedges))
        hists[mode] = ents
        if nth in ('hr', 'lr'):
            if hhd.nums[m] >= 2 and len(bin_entries) == 2:
                KLDiv = rutils.KLD_hist(torch.Tensor(binedges))
                v = float(KLDiv(torch.Tensor(bin_entries[0]), torch.Tensor(bin_entries[1])).item())
                total.append(v)
                kd[mode] = v
        elif hhd.nums[m] >= 2 and len(bin_entries) == 4:
            KLDiv = rutils.KLD_hist(torch.Tensor(binedges))
            v = float(KLDiv(torch.Tensor(bin_entries[0]), torch.Tensor(bin_entries[1])).item())
            v += float(KLDiv(torch.Tensor(bin_entries[2]), torch.Tensor(bin_entries[3])).item())
            total.append(v)
            kd[mode] = v
    return total, kd, hists


def store_set(tag, batches, f, modes, kl=True, meanenergy=False):
    for j, b in enumerate(batches):
        for i, x in enumerate(b):
            out[f"{tag}.in.{j}.{i}"] = x.astype(np.float32)
    out[f"{tag}.n_batches"] = np.int64(len(batches))
    out[f"{tag}.factor"] = np.int64(f)
    hhd, hsum, hme = run_reference(batches, f, modes, meanenergy)
    for m, mode in enumerate(modes):
        if mode == 'hitogram':
            for i, x in enumerate(hhd[m].raster.get_hist()):
                out[f"{tag}.map.{mode}.{i}"] = np.asarray(x)
        elif mode == 'meanimg':
            for i, x in enumerate(hhd[m].meanimg.get_hist()):
                out[f"{tag}.map.{mode}.{i}"] = np.asarray(x)
        else:
            for i, l in enumerate(hhd[m].list):
                out[f"{tag}.list.{mode}.{i}"] = np.array(l)
    for i, l in enumerate(hsum.list):
        out[f"{tag}.list.sum.{i}"] = np.array(l)
    if hme is not None:
        for i, x in enumerate(hme.meanimg.get_hist()):
            out[f"{tag}.map.meanenergy.{i}"] = np.asarray(x)
    # per-image references of the jet mass: E_jet too (the tolerance is relative to E_jet^2)
    for j, b in enumerate(batches):
        for i, x in enumerate(b):
            if np.isnan(x).any():
                continue
            ejet = []
            for img in x[:, 0]:
                H = img.shape[0]
                e = 0.0
                for r, c in zip(*np.nonzero(img)):
                    e += rutils.PtEtaPhiM_to_EPxPyPz(img[r, c], r * 2 / H - 1 + 1 / H, c * 2 / H - 1 + 1 / H, 0)[0]
                ejet.append(e)
            out[f"{tag}.ejet.{j}.{i}"] = np.array(ejet)
    if kl:
        for nth in ('hr', 'lr', 'both'):
            total, kd, hists = kl_summary(hhd, modes, 30, nth)
            out[f"{tag}.total_kld.{nth}"] = np.array(total)
            for mode, v in kd.items():
                out[f"{tag}.kld.{nth}.{mode}"] = np.float64(v)
            if nth == 'hr':
                for mode, ents in hists.items():
                    for i, (e, be) in enumerate(ents):
                        out[f"{tag}.hist.{mode}.{i}"] = e
                        out[f"{tag}.edges.{mode}.{i}"] = be
    return hhd


# ---- jet-like sets
store_set("jets80", jets(3, 4, 80, 101, 2), 2, MODES, meanenergy=True)
store_set("jets40", jets(2, 6, 40, 201, 2), 2, MODES)

# ---- edge cases at 16x16
g = torch.Generator().manual_seed(7)
H = 16
few = np.zeros((H, H), np.float32); few[3, 4], few[9, 1], few[12, 12] = 5.0, 2.5, 0.75          # 3 non-zero < 5, 10, 30
tie = (5 * torch.rand(H, H, generator=g) * (torch.rand(H, H, generator=g) < 0.3)).numpy()
tie[2, 2] = tie[7, 11] = tie[14, 0] = 9.5                                                        # exact tie at ranks 1-3
tie[5, 5] = tie[6, 6] = 7.25                                                                     # and at ranks 4-5
neg = (4 * torch.rand(H, H, generator=g) - 1).numpy() * (torch.rand(H, H, generator=g).numpy() < 0.5)
zero = np.zeros((H, H), np.float32)
sr0 = np.stack([few, tie, neg, zero])[:, None].astype(np.float32)
_, hr0 = O.jet_images(4, 1, H, H, 301, 2)
_, a1 = O.jet_images(2, 1, H, H, 302, 2)
nan1 = a1.numpy().copy(); nan1[1, 0, 3, 3] = np.nan
_, one = O.jet_images(1, 1, H, H, 303, 2)
edge = [kinds(sr0, hr0.numpy(), 2), kinds(nan1, a1.numpy(), 2), kinds(one.numpy(), one.numpy() * 0.5, 2)]
store_set("edge", edge, 2, MODES, kl=False)

# ---- end to end through the reference generator (G10: 16 filters, 2 RRDBs, x4, res_scale 0.1)
gen = rmodels.GeneratorRRDB(1, filters=16, num_res_blocks=2, num_upsample=2, res_scale=0.1)
gen.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "G10_ref_generator.pth"), map_location="cpu"))
gen.thres = 0
gen.eval()
F, NB, BS, LRS = 4, 3, 4, 10


def safe(vals, edges, rel=1e-5):
    """no value within rel (of the larger of the edge and the values' scale) of an edge; values equal to the edge itself are the
    range end points, which move with them"""
    v = np.asarray(vals, np.float64).ravel()
    scale = np.abs(v).max() if v.size else 0.0
    for e in np.asarray(edges, np.float64).ravel():
        d = np.abs(v - e)
        if ((d > 0) & (d <= rel * max(abs(e), scale))).any():
            return False
    return True


for seed in range(500, 600):
    lr = [O.jet_images(BS, 1, LRS * F, LRS * F, seed * 10 + k, F) for k in range(NB)]
    batches = []
    with torch.no_grad():
        for lr_k, hr_k in lr:
            srk = gen(lr_k)
            batches.append([srk.numpy(), hr_k.numpy(), lr_k.numpy(), pool(srk.numpy(), F)])
    ok = True
    for b in batches:
        for x in (b[0], b[3]):
            if not safe(x, [THR, 0.7, 0.0]):
                ok = False
                if os.environ.get("G17_VERBOSE"):
                    print("seed", seed, "threshold")
            s = np.sort(x.reshape(len(x), -1), axis=1)[:, ::-1]
            gaps = np.abs(s[:, :6] - s[:, 1:7])            # the positions deltaR_12 and FWM_1_5 read
            if ((gaps > 0) & (gaps <= 1e-5 * np.abs(s[:, :6]))).any():
                ok = False
                if os.environ.get("G17_VERBOSE"):
                    print("seed", seed, "gap")
    if not ok:
        continue
    hhd, _, _ = run_reference(batches, F, E2E_MODES)
    for m, mode in enumerate(E2E_MODES):
        if mode in ('hitogram', 'meanimg'):
            continue
        for nth in ('hr',):
            _, _, hists = kl_summary(hhd, E2E_MODES, 30, nth)
        for i in (0, 3):
            if i < len(hhd[m].list) and np.asarray(hhd[m].list[i]).dtype.kind == 'f':
                p = hhd[m].power
                vals = np.array(hhd[m].list[i]) ** p
                edges = [be for _, be in hists.get(mode, [])]
                pl = np.array(hhd[m].list[i]) ** p
                if len(pl):
                    edges.append(np.histogram(pl, 100)[1])
                if not all(safe(vals, e) for e in edges):
                    ok = False
                    if os.environ.get("G17_VERBOSE"):
                        print("seed", seed, "unsafe", mode, i)
    if ok:
        break
else:
    sys.exit("no safe end-to-end seed found")
out["e2e.seed"] = np.int64(seed)
store_set("e2e", batches, F, E2E_MODES)

np.savez_compressed(os.path.join(ROOT, "tests", "golden", "G17_observables.npz"), **out)
print("wrote G17_observables.npz:", len(out), "arrays, e2e seed", seed)
