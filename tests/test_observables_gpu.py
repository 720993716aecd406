"""Jet observables on the HIP kernels (srk_eval_image_stats / srk_eval_pixel_counts) and evaluation.distribution(), against the
reference's own MultHist / SumRaster / MeanImage / KL code (tests/golden/G17_observables.npz, tools/make_golden_eval.py) and
against fp64 ATen / torch.topk computed here."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
srk = load_pkg()
obs, L = srk.observables, srk._lib
MODES = ['max', 'min', 'mean', 'nnz', 'meannnz', 'E', 'E_1', 'E_2', 'E_5', 'E_10', 'E_30', 'R_12', 'R_25', 'deltaR_12', 'deltaR_13',
         'FWM_1_5', 'FWM_2_10', 'FWM_1_30', 'jetmass', 'hitogram', 'meanimg', 'sum']
E2E_MODES = ['max', 'mean', 'nnz', 'meannnz', 'E_1', 'E_5', 'R_12', 'deltaR_12', 'FWM_1_5', 'jetmass', 'hitogram', 'meanimg']
RTOL = {'sum': 1e-6, 'mean': 1e-6, 'meannnz': 1e-6, 'FWM': 1e-5}


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(os.path.join(golden_dir, "G17_observables.npz"))


def _batches(g17, tag, gpu_pool=True):
    f = int(g17[f"{tag}.factor"])
    pool = srk.SumPool2d(f)
    out = []
    for j in range(int(g17[f"{tag}.n_batches"])):
        k = [torch.from_numpy(g17[f"{tag}.in.{j}.{i}"]).cuda() for i in range(4)]
        if gpu_pool:
            k[3] = pool(k[0])                          # LR_gen built on the GPU
        out.append(k)
    return out


def _check_lists(g17, tag, lists, modes, rtol_cont=None):
    for m in modes:
        if m in obs.MAP_MODES:
            continue
        spec = obs.parse_mode(m)
        for i, got in enumerate(lists[m]):
            ref = g17[f"{tag}.list.{m}.{i}"]
            assert got.shape == ref.shape, (m, i, got.shape, ref.shape)
            if spec.kind == 'jetmass':
                ej = np.concatenate([g17[f"{tag}.ejet.{j}.{i}"] for j in range(int(g17[f"{tag}.n_batches"]))
                                     if f"{tag}.ejet.{j}.{i}" in g17.files and len(g17[f"{tag}.ejet.{j}.{i}"]) > 1])
                tol = 1e-10 * ej ** 2 if rtol_cont is None else rtol_cont * np.maximum(ref.astype(np.float64) ** 2, ej ** 2 * 1e-6)
                assert (np.abs(got ** 2 - ref ** 2) <= tol + 1e-30).all(), (m, i)
                continue
            rtol = RTOL.get(spec.kind, 0.0) if rtol_cont is None else (rtol_cont if ref.dtype.kind == 'f' else 0.0)
            if rtol == 0.0:
                np.testing.assert_array_equal(got, ref, err_msg=f"{tag} {m} kind {i}")
            else:
                np.testing.assert_allclose(got, ref, rtol=rtol, atol=0, equal_nan=True, err_msg=f"{tag} {m} kind {i}")


@pytest.mark.parametrize("tag", ["jets80", "jets40", "edge"])
def test_lists_and_maps_against_reference(g17, tag):
    col = obs.Collector(obs.parse_modes(MODES), int(g17[f"{tag}.factor"]))
    for b in _batches(g17, tag):
        col.add(b)
    lists, maps = col.finish()
    _check_lists(g17, tag, lists, MODES)
    for m in obs.MAP_MODES:
        for i in range(2):
            np.testing.assert_array_equal(maps[m][i], g17[f"{tag}.map.{m}.{i}"], err_msg=m)


def test_meanenergy_map(g17):
    col = obs.Collector(obs.parse_modes(['meanimg']), 2, meanenergy=True)
    for b in _batches(g17, "jets80"):
        col.add(b)
    _, maps = col.finish()
    for i in range(2):
        np.testing.assert_allclose(maps['meanimg'][i], g17[f"jets80.map.meanenergy.{i}"], rtol=1e-6)


def _fwm_ref(img, idx, l, j):
    """eval.py:78-95 in fp64 ATen on the given top-j positions"""
    H, W = img.shape
    idx = idx[:j].long()
    r, c = (idx // W).double(), (idx % W).double()
    eta, phi = r * 2 / H - 1, c * 2 / H - 1
    th = 2 * torch.atan(torch.exp(-eta))
    pt = img.reshape(-1)[idx].abs().sqrt().double()
    cd, cs = torch.cos(th[:, None] - th[None]), torch.cos(th[:, None] + th[None])
    cosang = 0.5 * (cd - cs) * torch.cos(phi[:, None] - phi[None]) + 0.5 * (cd + cs)
    P = [torch.ones_like(cosang), cosang]
    for n in range(1, l):
        P.append(((2 * n + 1) * cosang * P[n] - n * P[n - 1]) / (n + 1))
    return float((pt[:, None] * pt[None] / pt.sum() ** 2 * P[l]).sum())


def _run(x, K, pairs, thr=0.002, poison=False):
    B = x.shape[0]
    rec = (torch.empty(B, L.EVAL_NSTAT, dtype=torch.float64, device="cuda"), torch.empty(B, K, dtype=torch.float32, device="cuda"),
           torch.empty(B, K, dtype=torch.int32, device="cuda"), torch.zeros(B, L.EVAL_TIES, dtype=torch.int32, device="cuda"),
           torch.empty(B, len(pairs), dtype=torch.float64, device="cuda"))
    if poison:
        L.poison_lds()
    L.eval_image_stats(x, thr, K, pairs, *rec)
    return [t.cpu() for t in rec]


@pytest.mark.parametrize("H,B", [(40, 8), (80, 8), (256, 4), (512, 2)])
def test_sizes_against_aten(H, B):
    g = torch.Generator(device="cuda").manual_seed(H)
    x = 10 * torch.rand(B, 1, H, H, device="cuda", generator=g) * (torch.rand(B, 1, H, H, device="cuda", generator=g) < 0.05)
    x[0, 0, 1, 1] = x[0, 0, 2, 3] = x[0, 0, H - 1, H - 1] = 20.0          # a three-way tie at the top
    x[1, 0, 5, 7] = -3.0
    K, pairs = 64, [(1, 5), (2, 30), (3, 64)]
    st, topv, topi, ties, fwm = _run(x, K, pairs)
    xc = x.cpu()[:, 0]
    flat = xc.reshape(B, -1)
    for b in range(B):
        v, _ = torch.topk(flat[b], K)
        assert torch.equal(topv[b], v), b
        assert torch.equal(flat[b][topi[b].long()], topv[b])
        same = topv[b][1:] == topv[b][:-1]
        assert (topi[b][1:][same] > topi[b][:-1][same]).all()               # ties: lowest position first
        for r in range(9):
            assert ties[b, r] == int((flat[b] == topv[b, r]).sum())
        d = flat[b].double()
        assert st[b, L.EVAL_MAX] == d.max() and st[b, L.EVAL_MIN] == d.min()
        assert math.isclose(st[b, L.EVAL_SUM], d.sum().item(), rel_tol=1e-12)
        nz = d[flat[b] > 0.002]
        assert st[b, L.EVAL_NNZ] == len(nz) and math.isclose(st[b, L.EVAL_NNZ_SUM], nz.sum().item(), rel_tol=1e-12)
        rr = torch.arange(H, dtype=torch.float64)
        ctr = rr * 2 / H - 1 + 1 / H
        img = xc[b].double()
        E = (img * torch.cosh(ctr)[:, None]).sum()
        pz = (img * torch.sinh(ctr)[:, None]).sum()
        px = (img * torch.cos(ctr)[None]).sum()
        py = (img * torch.sin(ctr)[None]).sum()
        for k, ref in ((L.EVAL_E, E), (L.EVAL_PX, px), (L.EVAL_PY, py), (L.EVAL_PZ, pz)):
            assert abs(st[b, k] - ref.item()) <= 1e-12 * E.item(), k
        for p, (l, j) in enumerate(pairs):
            assert math.isclose(fwm[b, p].item(), _fwm_ref(xc[b], topi[b], l, j), rel_tol=1e-6, abs_tol=1e-12), (l, j)
    assert st[:, L.EVAL_NAN].eq(0).all()


def test_deterministic_and_under_poisoned_lds():
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(16, 1, 80, 80, device="cuda", generator=g).round(decimals=2) * (torch.rand(16, 1, 80, 80, device="cuda", generator=g) < 0.3)
    a = _run(x, 64, [(1, 30), (4, 64)])
    b = _run(x, 64, [(1, 30), (4, 64)])
    c = _run(x, 64, [(1, 30), (4, 64)], poison=True)
    for ta, tb, tc in zip(a, b, c):
        assert torch.equal(ta.view(torch.uint8) if ta.dtype.is_floating_point else ta, tb.view(torch.uint8) if tb.dtype.is_floating_point else tb)
        assert torch.equal(ta.view(torch.uint8) if ta.dtype.is_floating_point else ta, tc.view(torch.uint8) if tc.dtype.is_floating_point else tc)
    count = [torch.zeros(80, 80, dtype=torch.float64, device="cuda") for _ in range(3)]
    en = [torch.zeros(80, 80, dtype=torch.float64, device="cuda") for _ in range(3)]
    for i in range(3):
        if i == 2:
            L.poison_lds()
        L.eval_pixel_counts(x, 0.3, count[i], en[i])
    assert torch.equal(count[0], count[1]) and torch.equal(count[0], count[2])
    assert torch.equal(en[0].view(torch.uint8), en[1].view(torch.uint8)) and torch.equal(en[0].view(torch.uint8), en[2].view(torch.uint8))
    assert torch.equal(count[0], (x[:, 0] > 0.3).sum(0).double())


class _Pairs(torch.utils.data.Dataset):
    def __init__(self, lr, hr):
        self.lr, self.hr = lr, hr

    def __len__(self):
        return len(self.lr)

    def __getitem__(self, i):
        return {"lr": self.lr[i], "hr": self.hr[i]}


def _e2e(g17):
    n = int(g17["e2e.n_batches"])
    lr = torch.cat([torch.from_numpy(g17[f"e2e.in.{j}.2"]) for j in range(n)])
    hr = torch.cat([torch.from_numpy(g17[f"e2e.in.{j}.1"]) for j in range(n)])
    gen = srk.GeneratorRRDB(1, filters=16, num_res_blocks=2, num_upsample=2, res_scale=0.1).cuda()
    gen.load_state_dict(torch.load(os.path.join(os.path.dirname(__file__), "golden", "G10_ref_generator.pth"), map_location="cuda"))
    return gen, _Pairs(lr, hr), len(g17["e2e.in.0.0"])


@pytest.mark.parametrize("nth", ["hr", "lr", "both"])
def test_distribution_end_to_end(g17, nth):
    gen, ds, bs = _e2e(g17)
    res = srk.evaluation.distribution(gen, ds, "cuda", E2E_MODES, bins=30, batch_size=bs, factor=4, nth_jet_eval_mode=nth)
    _check_lists(g17, "e2e", res["lists"], E2E_MODES, rtol_cont=1e-4)
    for m in obs.MAP_MODES:
        for i in range(2):
            np.testing.assert_array_equal(res["maps"][m][i], g17[f"e2e.map.{m}.{i}"], err_msg=m)
    np.testing.assert_allclose(res["total_kld"], g17[f"e2e.total_kld.{nth}"], rtol=1e-4, atol=1e-7)
    ref = {k.split('.')[-1]: float(g17[k]) for k in g17.files if k.startswith(f"e2e.kld.{nth}.")}
    assert set(res["kld"]) == set(ref)
    for k, v in ref.items():
        assert math.isclose(res["kld"][k], v, rel_tol=1e-4, abs_tol=1e-7), k
    if nth == "hr":
        for m, h in res["hists"].items():
            for i, e in enumerate(h["entries"]):
                np.testing.assert_array_equal(e, g17[f"e2e.hist.{m}.{i}"], err_msg=m)


def test_distribution_refuses_cpu(g17):
    gen, ds, bs = _e2e(g17)
    with pytest.raises(RuntimeError, match="CPU"):
        srk.evaluation.distribution(gen, ds, "cpu", ['max'], batch_size=bs, factor=4)
    with pytest.raises(RuntimeError, match="CPU"):
        srk.evaluation.distribution(gen.cpu(), ds, "cuda", ['max'], batch_size=bs, factor=4)
    with pytest.raises(RuntimeError, match="CUDA"):
        L.eval_image_stats(torch.zeros(1, 1, 8, 8), 0.002, 9, [], None, None, None, None, None)
