"""Jet observables of the reference's ``distribution()`` (evaluation/eval.py:238-430, 497-817): mode parsing, per-mode
extraction from the per-image records of the HIP kernels (``srk_eval_image_stats`` / ``srk_eval_pixel_counts``, see
include/srk.h), and the histogram / KL summary, which runs on the host on the small per-image arrays.

Modes (``MultHist``'s docstring): ``max min mean sum nnz meannnz E E_n R_nm deltaR_nm FWM_l_j jetmass hitogram meanimg``, each
optionally with the additions ``corr_`` / ``_lr`` / ``ratio_`` (they only add plots in the reference and are stripped here).
``wmass``, ``nsubj_*``, ``w_pf`` and ``C_0_*`` need the clustering packages and raise ``NotImplementedError``.

The kinds are, in order, SR (generator output), HR, LR and LR_gen = SumPool(SR); a mode uses the first ``nums`` of them
(``MultModeHist.standard_nums``; modes containing ``_`` use 4).  The reference has no entry for ``sum`` there (its
``MultModeHist`` raises ``KeyError``); here ``sum`` uses all 4 kinds.  ``meannnz`` follows eval.py:334 as written for NumPy 1: under
NumPy 2 its ``np.nan_to_num(mean, 0)`` passes ``copy=False`` for a scalar and raises, which ``MultHist.append`` swallows.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L
from .losses import KLD_hist

STANDARD_NUMS = {'max': 3, 'min': 3, 'nnz': 4, 'mean': 2, 'meannnz': 4, 'wmass': 2, 'E': 2, 'hitogram': 2, 'meanimg': 2, 'jetmass': 4,
                 'sum': 4}
KINDS = ("SR", "HR", "LR", "LR_gen")
MAP_MODES = ("hitogram", "meanimg")
HITOGRAM_THRESHOLD = 0.7        # SumRaster's default (utils.py:276); MultHist does not pass its own threshold
_NEEDS = {'wmass': 'pyjet', 'nsubj': 'pyjet and energyflow', 'w_pf': 'pyjet and energyflow', 'C_0_': 'energyflow'}


@dataclass
class ModeSpec:
    mode: str                   # as given (the key of the results)
    base: str                   # additions removed
    kind: str                   # max min mean sum nnz meannnz E E_n R deltaR FWM jetmass hitogram meanimg
    nums: int
    power: float = 1.0
    display_ratio: float = 1.0
    args: tuple = field(default_factory=tuple)


def rm_additions(mode):
    """MultModeHist.rmAdditions (eval.py:425-426)."""
    return mode.replace('corr_', '').replace('_lr', '').replace('ratio_', '')


def parse_mode(mode):
    """One mode string -> ModeSpec with MultHist's semantics (eval.py:238-313, 413-424)."""
    base = rm_additions(mode)
    for key, pkg in _NEEDS.items():
        if (base == key) or (key.endswith('_') and key in base) or (key == 'nsubj' and 'nsubj' in base):
            raise NotImplementedError(f"eval mode {mode!r} needs {pkg}, which is outside this build")
    if '_' not in base and base not in STANDARD_NUMS:
        raise ValueError(f"unknown eval mode {mode!r}")
    nums = 4 if '_' in base else STANDARD_NUMS[base]
    power, ratio = 1.0, 1.0
    if base == 'E' or ('R' in base and 'deltaR' not in base) or base[:2] == 'E_':
        power, ratio = 0.5, 0.98
    elif base == 'meannnz':
        ratio = 0.95
    # the dispatch order of MultHist.append
    if base in ('max', 'min', 'mean', 'nnz', 'sum', 'meannnz', 'E', 'jetmass', 'hitogram', 'meanimg'):
        kind, args = base, ()
    elif 'E_' in base:
        kind, args = 'E_n', (int(base[2:]),)
    elif 'deltaR_' in base:
        kind, args = 'deltaR', (int(base[7]), int(base[8]))
    elif 'R_' in base:
        kind, args = 'R', (int(base[2]), int(base[3]))
    elif 'FWM' in base:
        kind, args = 'FWM', tuple(int(s) for s in base[4:].split('_'))
    else:
        raise ValueError(f"unknown eval mode {mode!r}")
    for a in args:
        if kind != 'FWM' and not 1 <= a <= L.EVAL_MAX_K:
            raise ValueError(f"eval mode {mode!r}: ranks run from 1 to {L.EVAL_MAX_K}")
    if kind == 'FWM' and not (0 <= args[0] <= L.EVAL_MAX_L and 1 <= args[1] <= L.EVAL_MAX_K):
        raise ValueError(f"eval mode {mode!r}: FWM_l_j needs 0 <= l <= {L.EVAL_MAX_L}, 1 <= j <= {L.EVAL_MAX_K}")
    return ModeSpec(mode, base, kind, nums, power, ratio, args)


def parse_modes(modes):
    return [parse_mode(m) for m in ([modes] if isinstance(modes, str) else list(modes))]


def top_k_needed(specs):
    """How many of the largest values per image the modes read (at least the 9 ranks whose tie counts delta_r needs)."""
    k = L.EVAL_TIES
    for s in specs:
        if s.kind in ('E_n', 'R', 'deltaR'):
            k = max(k, *s.args)
        elif s.kind == 'FWM':
            k = max(k, s.args[1])
    return k


def fwm_pairs(specs):
    pairs = []
    for s in specs:
        if s.kind == 'FWM' and s.args not in pairs:
            pairs.append(s.args)
    if len(pairs) > L.EVAL_MAX_FWM:
        raise ValueError(f"at most {L.EVAL_MAX_FWM} distinct FWM_l_j modes per evaluation")
    return pairs


# ----------------------------------------------------------------------------------------------------------------- device records

class KindRecords:
    """Per-image records of one kind over the whole dataset, kept on the device until ``host()``."""

    def __init__(self, K, pairs, thr, keep_values):
        self.K, self.pairs, self.thr, self.keep_values = K, pairs, thr, keep_values
        self.parts, self.values, self.sizes, self.shape = [], [], [], None

    def add(self, x):
        if self.shape is None:
            self.shape = tuple(x.shape[2:])
        if tuple(x.shape[2:]) != self.shape:
            raise RuntimeError(f"image size changed between batches: {self.shape} -> {tuple(x.shape[2:])}")
        B, dev = x.shape[0], x.device
        K = min(self.K, self.shape[0] * self.shape[1])
        rec = (torch.empty(B, L.EVAL_NSTAT, dtype=torch.float64, device=dev), torch.empty(B, K, dtype=torch.float32, device=dev),
               torch.empty(B, K, dtype=torch.int32, device=dev), torch.zeros(B, L.EVAL_TIES, dtype=torch.int32, device=dev),
               torch.empty(B, len(self.pairs), dtype=torch.float64, device=dev) if self.pairs else None)
        L.eval_image_stats(x, self.thr, K, self.pairs, *rec)
        self.parts.append(rec)
        self.sizes.append(B)
        if self.keep_values:
            self.values.append(x.reshape(-1))

    def host(self):
        """One transfer per array at the end: {'stats','topv','topi','ties','fwm','sizes','H','W','values'}."""
        cat = lambda j: torch.cat([p[j] for p in self.parts]).cpu().numpy()
        out = dict(stats=cat(0), topv=cat(1), topi=cat(2), ties=cat(3), fwm=cat(4) if self.pairs else None,
                   sizes=list(self.sizes), H=self.shape[0], W=self.shape[1], pairs=list(self.pairs))
        out['values'] = [v[v > self.thr].cpu().numpy() for v in self.values] if self.keep_values else None
        return out


class Collector:
    """The device side of one evaluation: per batch, ``add([SR, HR, LR, LR_gen])`` ([B, 1, H, W] fp32 CUDA tensors; kinds past
    the modes' largest ``nums`` may be None) launches the record kernel per kind and the map kernels for SR / HR; ``finish()``
    moves everything to the host once and returns ``(lists, maps)``: lists[mode] = [array per kind], maps[mode] = [sr, hr]
    (hitogram folded to factor x factor, meanimg as MeanImage.get_hist returns it)."""

    def __init__(self, specs, factor, threshold=0.002, meanenergy=False):
        self.specs, self.factor, self.threshold = specs, factor, threshold
        self.list_specs = [s for s in specs if s.mode not in MAP_MODES]
        self.n_kinds = max([s.nums for s in self.list_specs] + [0])
        K, pairs = top_k_needed(self.list_specs), fwm_pairs(self.list_specs)
        keep_values = any(s.kind == "E" for s in self.list_specs)
        self.recs = [KindRecords(K, pairs, threshold, keep_values) for _ in range(self.n_kinds)]
        names = [s.mode for s in specs]
        self.map_cfg = [(n, thr, e) for n, thr, e in (("hitogram", HITOGRAM_THRESHOLD, False),
                                                      ("meanimg", threshold, meanenergy or threshold <= 0)) if n in names]
        self.maps, self.n_images = {}, 0

    def add(self, kinds):
        for x in kinds[:2]:
            if x is None or not x.is_cuda:
                raise RuntimeError("observables run on the HIP kernels of libsrk.so: got a CPU tensor (no CPU fallback)")
        for rec, x in zip(self.recs, kinds):
            rec.add(x)
        self.n_images += kinds[0].shape[0]
        for name, thr, energy in self.map_cfg:
            if name not in self.maps:
                H, W = kinds[1].shape[2:]
                z = lambda: torch.zeros(H, W, dtype=torch.float64, device=kinds[0].device)
                self.maps[name] = [(z(), z() if energy else None) for _ in range(2)]
            for (count, emap), x in zip(self.maps[name], kinds[:2]):
                L.eval_pixel_counts(x, thr, count, emap)

    def finish(self, reference_quirks=True):
        host = [r.host() for r in self.recs]
        lists = {s.mode: [extract(h, s, reference_quirks) for h in host[:s.nums]] for s in self.list_specs}
        maps, f = {}, self.factor
        for name, per_kind in self.maps.items():
            got = []
            for count, emap in per_kind:
                if name == "hitogram":
                    H, W = count.shape
                    if H % f or W % f:
                        raise ValueError(f"hitogram: image {H}x{W} does not split into {f}x{f} cells")
                    got.append(count.view(H // f, f, W // f, f).sum((0, 2)).cpu().numpy())
                else:
                    got.append((emap / self.n_images if emap is not None else count).cpu().numpy())
            maps[name] = got
        return lists, maps


# ----------------------------------------------------------------------------------------------------------------- extraction

def extract(rec, spec, reference_quirks=True):
    """One mode's list for one kind from host records (KindRecords.host()), with MultHist.append's batch handling; returns a
    numpy array of the element type the reference's list holds (float32 values, int64 counts, float64 for deltaR / FWM / jetmass;
    where the reference appends a python int 0 among float32 values -- meannnz or E of an image / batch without a value above the
    threshold -- the array is float64, as np.array of that list is).

    reference_quirks=True: a batch contributes nothing when it holds a NaN anywhere, when the reference would raise for it
    (R_nm with a zero m-th value, deltaR_nm with a tied n-th or m-th value), or when it holds one image for E_n / R / deltaR /
    FWM / jetmass (np.squeeze drops the batch axis there).  False: only images with a NaN are dropped, one by one."""
    st, topv, topi, ties = rec['stats'], rec['topv'], rec['topi'], rec['ties']
    H, W = rec['H'], rec['W']
    k = spec.kind
    parts, int_zero, begin = [], False, 0
    for bi, B in enumerate(rec['sizes']):
        sl = slice(begin, begin + B)
        begin += B
        nan = st[sl, L.EVAL_NAN] != 0
        keep = ~nan
        if reference_quirks:
            if nan.any():
                continue
            if B == 1 and k in ('E_n', 'R', 'deltaR', 'FWM', 'jetmass'):
                continue
            if k == 'R' and (topv[sl, spec.args[1] - 1] == 0).any():
                continue
            if k == 'deltaR' and ((ties[sl, spec.args[0] - 1] > 1) | (ties[sl, spec.args[1] - 1] > 1)).any():
                continue
        s = st[sl][keep]
        if k == 'max':
            v = s[:, L.EVAL_MAX].astype(np.float32)
        elif k == 'min':
            v = s[:, L.EVAL_MIN].astype(np.float32)
        elif k == 'mean':
            v = (s[:, L.EVAL_SUM] / (H * W)).astype(np.float32)
        elif k == 'sum':
            v = s[:, L.EVAL_SUM].astype(np.float32)
        elif k == 'nnz':
            v = s[:, L.EVAL_NNZ].astype(np.int64)
        elif k == 'meannnz':
            n = s[:, L.EVAL_NNZ]
            v = np.where(n > 0, s[:, L.EVAL_NNZ_SUM] / np.maximum(n, 1), 0.0).astype(np.float32)
            int_zero |= bool((n == 0).any())
        elif k == 'E':
            v = rec['values'][bi]                     # every value > thr of the batch, image by image
            if not reference_quirks and nan.any():
                per = np.split(v, np.cumsum(st[sl, L.EVAL_NNZ].astype(np.int64))[:-1])
                v = np.concatenate([p for p, ok in zip(per, keep) if ok] + [np.zeros(0, np.float32)])
            if len(v) == 0:
                v, int_zero = np.zeros(1, np.float32), True
        elif k == 'E_n':
            v = topv[sl][keep, spec.args[0] - 1]
        elif k == 'R':
            n, m = spec.args
            v = topv[sl][keep, n - 1] / topv[sl][keep, m - 1]
        elif k == 'deltaR':
            # eval.py:192-215 takes bins = arr.shape[1] of the [B, 1, H, W] batch, i.e. 1: bin b sits at 2 * b
            n, m = spec.args
            i_n, i_m = topi[sl][keep, n - 1].astype(np.int64), topi[sl][keep, m - 1].astype(np.int64)
            centre = lambda b: b * 2 * 1.0 / 1 - 1.0 + 1.0 / 1
            deta = centre(i_n // W) - centre(i_m // W)
            dphi = centre(i_n % W) - centre(i_m % W)
            v = np.sqrt(deta ** 2 + dphi ** 2)
        elif k == 'FWM':
            v = rec['fwm'][sl][keep, rec['pairs'].index(spec.args)]
        elif k == 'jetmass':
            E, px, py, pz = (s[:, j] for j in (L.EVAL_E, L.EVAL_PX, L.EVAL_PY, L.EVAL_PZ))
            v = np.sqrt(np.abs(E ** 2 - px ** 2 - py ** 2 - pz ** 2))
        else:
            raise ValueError(spec.mode)
        parts.append(v)
    dtype = {'nnz': np.int64, 'deltaR': np.float64, 'FWM': np.float64, 'jetmass': np.float64}.get(k, np.float32)
    if int_zero and dtype == np.float32:
        dtype = np.float64
    return np.concatenate([p.astype(dtype) for p in parts]) if parts else np.zeros(0, dtype)


# ----------------------------------------------------------------------------------------------------------------- host summary

def get_range(lists):
    """MultHist.get_range: (min, max) over every kind's list."""
    return min(l.min() for l in lists), max(l.max() for l in lists)


def display_max(lists, power, threshold):
    """MultHist.max (eval.py:386-400): the upper edge of the 100-bin cumulative cut at ``threshold`` (< 1), else the largest
    value, both in powered units."""
    MAX = 0
    if threshold < 1:
        for l in lists:
            pl = np.array(l) ** power
            c, b = np.histogram(pl, 100)
            e_max = b[(np.cumsum(c) > len(pl) * threshold).argmax()]
            if e_max > MAX:
                MAX = e_max
    else:
        MAX = max(l.max() for l in lists) ** power
    return MAX


def histogram(lists, i, spec, bins, auto_range=True):
    """MultHist.histogram of kind i (eval.py:402-410)."""
    l = lists[i]
    if auto_range:
        if spec.power != 1:
            return np.histogram(np.array(l) ** spec.power, bins, range=(get_range(lists)[0] ** spec.power,
                                                                        display_max(lists, spec.power, spec.display_ratio)))
        return np.histogram(l, bins, range=get_range(lists))
    return np.histogram(l, bins)


def map_kld(sr, hr):
    """eval.py:633-642 for hitogram / meanimg: both maps + 0.1, KLDivLoss(sum)((sr / sum sr).log(), hr / sum sr) -- the reference
    normalises hr by the sum of sr, kept as it is."""
    sr, hr = .1 + torch.Tensor(sr)[None, None, ...], .1 + torch.Tensor(hr)[None, None, ...]
    return float(torch.nn.KLDivLoss(reduction='sum')((sr / sr.sum()).log(), hr / (sr.sum())))


def summarize(specs, lists, maps, bins=30, nth_jet_eval_mode='hr'):
    """The histogram / KL part of distribution() (eval.py:598-718) on host lists: returns (total_kld, kld_dict, hists) where
    hists[mode] = {'entries': [per kind], 'binedges': [per kind]} (kinds whose histogram fell back to auto_range=False included,
    as the reference plots them; only auto-ranged ones enter the KL)."""
    total_kld, kld, hists = [], {}, {}
    for spec in specs:
        if spec.mode in MAP_MODES:
            v = map_kld(*maps[spec.mode])
            total_kld.append(v)
            kld[spec.mode] = v
            continue
        L_ = lists[spec.mode]
        bin_entries, binedges = [], None
        hists[spec.mode] = {'entries': [], 'binedges': []}
        for i in range(4):
            if spec.nums == i:
                continue
            if i >= len(L_):                          # the reference's IndexError
                continue
            try:
                entries, binedges = histogram(L_, i, spec, bins)
                if nth_jet_eval_mode == 'hr':
                    if i < 2:
                        bin_entries.append(entries)
                elif nth_jet_eval_mode == 'lr':
                    if i > 1:
                        bin_entries.append(entries)
                else:
                    bin_entries.append(entries)
            except ValueError:
                entries, binedges = histogram(L_, i, spec, bins, auto_range=False)
            hists[spec.mode]['entries'].append(entries)
            hists[spec.mode]['binedges'].append(binedges)
        if nth_jet_eval_mode in ('hr', 'lr'):
            if spec.nums >= 2 and len(bin_entries) == 2:
                KLDiv = KLD_hist(torch.Tensor(binedges))
                kl = float(KLDiv(torch.Tensor(bin_entries[0]), torch.Tensor(bin_entries[1])).item())
                total_kld.append(kl)
                kld[spec.mode] = kl
        elif spec.nums >= 2 and len(bin_entries) == 4:
            KLDiv = KLD_hist(torch.Tensor(binedges))
            kl = float(KLDiv(torch.Tensor(bin_entries[0]), torch.Tensor(bin_entries[1])).item())
            kl += float(KLDiv(torch.Tensor(bin_entries[2]), torch.Tensor(bin_entries[3])).item())
            total_kld.append(kl)
            kld[spec.mode] = kl
    return total_kld, kld, hists
