"""Eval-mode inference callers of the generator: the HR/LR L1 part of the reference's ``calculate_metrics``
(evaluation/eval.py:455-494; the energy-mover's-distance term needs ``energyflow`` and is outside this build) and the jet
observable distributions of its ``distribution`` (eval.py:497-817, without plots).

The whole loop stays on the GPU (the reference moves every batch to the CPU for the pooling and the L1): eval-mode
forward on the HIP kernels under ``no_grad``, ``SumPool2d`` on the HIP kernel, per-image means.
"""
import numpy as np
import torch

from . import models, observables as obs


def calculate_metrics(generator, dataset, device, batch_size=4, n_cpu=0, factor=2, reference_labels=True):
    """Returns ``{'hr_l1': {'mean','std'}, 'lr_l1': {...}}``.

    ``reference_labels=True`` reproduces the reference's key assignment, which zips ``['hr_l1','lr_l1',...]`` with
    ``[lr_similarity, hr_similarity, ...]`` (eval.py:491): the value stored under 'hr_l1' is the LR-space L1 and vice
    versa.  Pass False for self-consistent names."""
    generator.eval()
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=n_cpu)
    pool = models.SumPool2d(factor)
    lr_similarity, hr_similarity = [], []
    with torch.no_grad():
        for imgs in loader:
            imgs_lr = imgs["lr"].to(device).float()
            imgs_hr = imgs["hr"].to(device).float()
            gen_hr = generator(imgs_lr)
            gen_lr = pool(gen_hr)
            lr_similarity.append((gen_lr - imgs_lr).abs().mean((1, 2, 3)))
            hr_similarity.append((gen_hr - imgs_hr).abs().mean((1, 2, 3)))
    lr_similarity = torch.cat(lr_similarity).cpu().numpy()
    hr_similarity = torch.cat(hr_similarity).cpu().numpy()
    names = ["hr_l1", "lr_l1"] if reference_labels else ["lr_l1", "hr_l1"]
    return {n: {"mean": float(np.mean(v)), "std": float(np.std(v))} for n, v in zip(names, [lr_similarity, hr_similarity])}


def distribution(generator, dataset, device, modes, bins=30, batch_size=4, factor=2, threshold=0.002, nth_jet_eval_mode="hr",
                 meanenergy=False, reference_quirks=True, n_cpu=0):
    """The reference's ``distribution`` (eval.py:497-817) without its plots: the observables of every mode for the kinds SR
    (generator output), HR, LR and LR_gen = SumPool2d(SR), their histograms and KL divergences.

    The loop (eval.py:527-541) runs the generator in eval mode under ``no_grad`` and ``SumPool2d`` on the HIP kernels; every
    per-image observable comes from ``srk_eval_image_stats`` and the maps from ``srk_eval_pixel_counts``, into device buffers;
    the host sees them once, at the end (mode ``E`` keeps each batch's images on the device and selects its values there too).
    ``dataset``: what ``train()`` accepts -- items {"lr", "hr"}, or the raw-row jet datasets, decoded batch by batch on the GPU
    (``datasets.extract_batch`` via ``decode_batch``).  No CPU path: CPU tensors, or a CPU device, raise.

    ``reference_quirks=True`` keeps ``MultHist.append``'s batch handling (eval.py:314-379): one kind's tensor of one batch adds
    nothing to a mode's list when it holds a NaN, when the reference raises for it (``R_nm`` with a zero m-th value,
    ``deltaR_nm`` with a tied n-th or m-th value, caught and printed there), or when the batch holds one image for ``E_n`` /
    ``R`` / ``deltaR`` / ``FWM`` / ``jetmass`` (``np.squeeze`` drops the batch axis).  ``False``: only images with a NaN are
    dropped, image by image; ties then resolve to the lowest flat position.  Either way ``deltaR_nm`` keeps the reference's
    bin centres (``bins = arr.shape[1]`` = 1 there), and the ``hitogram`` / ``meanimg`` KL keeps its ``hr / sr.sum()``.

    Returns ``{"lists": {mode: [array per kind]}, "maps": {mode: [sr, hr]}, "hists": {mode: {"entries", "binedges"}},
    "kld": {mode: float}, "total_kld": [float]}``: ``total_kld`` is what the reference returns, ``kld`` its ``kld_dict``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("evaluation.distribution runs on the HIP kernels of libsrk.so: got a CPU device (no CPU fallback)")
    if any(not p.is_cuda for p in generator.parameters()):
        raise RuntimeError("evaluation.distribution: the generator's parameters are on the CPU (no CPU fallback)")
    specs = obs.parse_modes(modes)
    col = obs.Collector(specs, factor, threshold, meanenergy)
    generator.eval()
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=n_cpu)
    pool = models.SumPool2d(factor)
    with torch.no_grad():
        for imgs in loader:
            if "rows" in imgs:
                imgs = dataset.decode_batch(imgs["rows"].to(device))
            imgs_lr = imgs["lr"].to(device).float()
            imgs_hr = imgs["hr"].to(device).float()
            gen_hr = generator(imgs_lr)
            col.add([gen_hr, imgs_hr, imgs_lr, pool(gen_hr) if col.n_kinds > 3 else None])
    lists, out_maps = col.finish(reference_quirks)          # the one hand-over to the host
    total_kld, kld, hists = obs.summarize(specs, lists, out_maps, bins=bins, nth_jet_eval_mode=nth_jet_eval_mode)
    return {"lists": lists, "maps": out_maps, "hists": hists, "kld": kld, "total_kld": total_kld}
