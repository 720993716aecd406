"""The Sinkhorn Wasserstein head on the MI355X (srk_sinkhorn.hip): parity with the reference's own numbers (G18), the fused
sort -> cut -> Sinkhorn path, gradients through the unrolled iterations, determinism, memory, no host sync, and the training step."""
import importlib
import os

import numpy as np
import pytest
import torch

from test_sinkhorn_host import _cases, _golden, sinkhorn64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _tol(r32, r64, floor_rel=1e-4):
    """max(floor, 1.5 x |ref32 - ref64|), the floor a fraction of the largest value"""
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    return max(floor_rel * max(np.abs(r64).max(), 1e-6), 1.5 * np.abs(r32 - r64).max())


def _close(have, r32, r64, what, floor_rel=1e-4):
    have = np.asarray(have, np.float64)
    assert have.shape == np.asarray(r64).shape, (what, have.shape, np.asarray(r64).shape)
    d, t = np.abs(have - r64).max(), _tol(r32, r64, floor_rel)
    assert d <= t, f"{what}: max |ours - ref64| = {d:.3g} > tol {t:.3g}"


def test_sinkhorn_distance_matches_g18(srk):
    g = _golden()
    for c in _cases(g, "sd_"):
        x = torch.tensor(g[c + "/x"], device=DEV, requires_grad=True)
        y = torch.tensor(g[c + "/y"], device=DEV, requires_grad=True)
        sd = srk.losses.SinkhornDistance(float(g[c + "/eps"]), int(g[c + "/max_iter"]), str(g[c + "/reduction"]))
        cost, pi, C = sd(x, y)
        cost.sum().backward()
        K = int(sd.last_iterations)
        assert K == int(g[c + "/K32"]) == int(g[c + "/K64"]), c
        np.testing.assert_allclose(sd.last_err[:K].cpu().numpy(), g[c + "/err32"], rtol=1e-3, err_msg=c)
        assert tuple(cost.shape) == tuple(g[c + "/cost_shape"]), c
        assert tuple(pi.shape) == tuple(g[c + "/pi_shape"]) and tuple(C.shape) == tuple(g[c + "/C_shape"]), c
        assert not pi.requires_grad and not C.requires_grad
        _close(cost.detach().cpu(), g[c + "/cost32"], g[c + "/cost64"], c + " cost")
        _close(x.grad.cpu(), g[c + "/gx32"], g[c + "/gx64"], c + " gx")
        _close(y.grad.cpu(), g[c + "/gy32"], g[c + "/gy64"], c + " gy")
        # C is the squared distance; the plan's columns hold exp(b) = 1/M + 1e-8 each (v was updated last) and sum_ij pi C is the cost
        xb = x.detach().reshape(-1, x.shape[-2])
        yb = y.detach().reshape(-1, y.shape[-2])
        B, N, M = xb.shape[0], xb.shape[1], yb.shape[1]
        torch.testing.assert_close(C.reshape(B, N, M), (xb[:, :, None] - yb[:, None, :]) ** 2)
        P3 = pi.reshape(B, N, M)
        torch.testing.assert_close(P3.sum(1), torch.full((B, M), 1.0 / M + 1e-8, device=DEV), rtol=1e-4, atol=0)
        per = (P3 * C.reshape(B, N, M)).sum((1, 2))
        red = str(g[c + "/reduction"])
        want = per.mean() if red == "mean" else per.sum() if red == "sum" else per.reshape(cost.shape)
        torch.testing.assert_close(cost.detach(), want, rtol=1e-4, atol=0)


def test_wasser_loss_matches_g18(srk):
    g = _golden()
    for c in _cases(g, "wl_"):
        gen = torch.tensor(g[c + "/gen"], device=DEV, requires_grad=True)
        real = torch.tensor(g[c + "/real"], device=DEV)
        loss, K = srk.losses.wasser_loss(gen, real, float(g[c + "/eps"]), int(g[c + "/max_iter"]), return_iterations=True)
        loss.backward()
        assert int(K) == int(g[c + "/K32"]), c
        _close(loss.item(), g[c + "/loss32"], g[c + "/loss64"], c + " loss")
        B = gen.shape[0]
        have = gen.grad.reshape(B, -1).cpu().numpy().astype(np.float64)
        r32, r64 = g[c + "/ggen32"].reshape(B, -1), g[c + "/ggen64"].reshape(B, -1)
        vals = g[c + "/gen"].reshape(B, -1)
        tol = _tol(r32, r64)
        for b in range(B):
            uniq, counts = np.unique(vals[b], return_counts=True)
            for val, cnt in zip(uniq, counts):
                sel = vals[b] == val
                if cnt == 1:          # untied pixel: its own gradient
                    assert abs(have[b][sel][0] - r64[b][sel][0]) <= tol, (c, b, val)
                else:                 # tied pixels: the sort may hand the group's gradient to different members
                    assert abs(have[b][sel].sum() - r64[b][sel].sum()) <= tol * cnt, (c, b, val)
        if c == "wl_zero_gen":        # nothing positive: cut_smaller keeps the whole row
            assert np.abs(have).max() > 0


def test_wasser_loss_nan_input_gives_nan(srk):
    gen = torch.rand(2, 1, 8, 8, device=DEV)
    gen[1, 0, 3, 3] = float("nan")
    loss, K = srk.losses.wasser_loss(gen, torch.rand(2, 1, 8, 8, device=DEV), 0.1, 30, return_iterations=True)
    assert torch.isnan(loss).item() and int(K) == 30


def test_fixed_iteration_gradient_matches_float64_autograd(srk):
    torch.manual_seed(5)
    B, N, M = 2, 500, 430
    x = (torch.rand(B, N, dtype=torch.float64) * 2.0)
    y = (torch.rand(B, M, dtype=torch.float64) * 2.0)
    x64, y64 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    cost64, K64, _ = sinkhorn64(x64, y64, 0.1, 20)
    assert K64 == 20
    cost64.sum().backward()
    xg = x.float().to(DEV)[..., None].requires_grad_(True)
    yg = y.float().to(DEV)[..., None].requires_grad_(True)
    sd = srk.losses.SinkhornDistance(0.1, 20, "none")
    cost, _, _ = sd(xg, yg)
    cost.sum().backward()
    assert int(sd.last_iterations) == 20
    for have, want, what in ((cost.detach(), cost64.detach(), "cost"), (xg.grad[..., 0], x64.grad, "gx"), (yg.grad[..., 0], y64.grad, "gy")):
        have = have.double().cpu()
        err = (have - want).abs().max().item() / want.abs().max().item()
        assert err < 1e-4, (what, err)


def _run(srk, gen, real):
    g = gen.clone().requires_grad_(True)
    loss = srk.losses.wasser_loss(g, real, 0.1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), g.grad.clone()


def _jets(B, H, W, frac, seed):
    gen = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 1, H, W, generator=gen)
    mask = torch.rand(B, 1, H, W, generator=gen) < frac
    return (img * mask).to(DEV)


def test_deterministic_and_lds_poison_proof(srk, monkeypatch):
    """Bit-identical repeats, also with NaN patterns written into every CU's LDS in front of every launch (SRK_POISON_LDS=1 is read
    by each srk_sort_cut / srk_sinkhorn_* call)."""
    gen, real = _jets(8, 40, 40, 0.3, 1), _jets(8, 40, 40, 0.25, 2)
    l0, g0 = _run(srk, gen, real)
    l1, g1 = _run(srk, gen, real)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    monkeypatch.setenv("SRK_POISON_LDS", "1")
    l2, g2 = _run(srk, gen, real)
    monkeypatch.delenv("SRK_POISON_LDS")
    assert torch.equal(l0, l2) and torch.equal(g0, g2)


def test_no_host_sync(srk):
    gen, real = _jets(4, 32, 32, 0.3, 3), _jets(4, 32, 32, 0.3, 4)
    g = gen.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):          # the mode catches a deliberate host sync on this build
            gen.sum().item()
        loss = srk.losses.wasser_loss(g, real, 0.1)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(loss).item() and torch.isfinite(g.grad).all().item()


def test_memory_stays_linear_in_the_kept_points(srk):
    gen = torch.rand(8, 1, 80, 80, device=DEV) + 0.01       # every pixel positive: N' = M' = 6400
    real = torch.rand(8, 1, 80, 80, device=DEV) + 0.01
    g = gen.clone().requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = srk.losses.wasser_loss(g, real, 0.1)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.isfinite(loss).item()
    assert peak < 64 * 2 ** 20, peak / 2 ** 20


def _stepper(srk, lambda_wasser=0.5, **kw):
    train = importlib.import_module("super-resolution_amd.train")
    torch.manual_seed(0)
    return train.Stepper(workload="gan", res_blocks=1, filters=16, device=DEV, hr=32, factor=2, res_scale=0.1, lambda_wasser=lambda_wasser,
                         sinkhorn_eps=0.1, **kw)


def test_head_adds_lambda_times_its_gradient_to_the_generator(srk):
    """loss_G gains sum_k lambdas[k] * lambda_wasser * wasser_loss(generated[k], ground_truth[k]) (esrgan.py:549-551): the
    generator's gradient with the head on minus the one with it off is the gradient of that term alone."""
    from oracle import esrgan_oracle as O
    lr, hr = O.jet_images(3, 1, 32, 32, 12, 2)
    lr, hr = lr.to(DEV), hr.to(DEV)
    lw = 5.0

    def grads(st, loss):
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in st.generator.named_parameters() if p.grad is not None}
    g = {}
    for on in (False, True):
        st = _stepper(srk, lambda_wasser=lw if on else 0.0)
        loss_G, _, _, parts = st.g_phase_loss(lr, hr)
        assert ("wasser" in parts[0]) == on and ("wasser" in parts[1]) == on
        g[on] = grads(st, loss_G)
    st = _stepper(srk, lambda_wasser=0.0)
    gen = [st.generator(lr), st.generator.srs]
    gt = [hr, hr ** st.scaling_power]
    head = sum(st.lambdas[k] * lw * srk.losses.wasser_loss(gen[k], gt[k], 0.1) for k in range(2))
    gh = grads(st, head)
    assert set(g[True]) == set(g[False]) == set(gh)
    big = max(t.abs().max().item() for t in g[True].values())
    hmax = max(t.abs().max().item() for t in gh.values())
    assert hmax > 1e-2 * big, (hmax, big)          # the head's share is far above the rounding of the rest
    for n in gh:
        err = (g[True][n] - g[False][n] - gh[n]).abs().max().item()
        assert err <= 1e-3 * hmax + 1e-5 * big, (n, err, hmax, big)


def test_single_point_images_are_separate_problems(srk):
    """Deliberate deviation: N = 1 or M = 1 with B > 1 solves each image on its own (the reference's mu.squeeze() would broadcast
    the images into each other)."""
    torch.manual_seed(3)
    for N, M in ((1, 6), (5, 1), (1, 1)):
        x = torch.rand(3, N, dtype=torch.float64) * 2
        y = torch.rand(3, M, dtype=torch.float64) * 2
        x64, y64 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        cost64, K64, _ = sinkhorn64(x64, y64, 0.5, 50)
        cost64.sum().backward()
        xg = x.float().to(DEV)[..., None].requires_grad_(True)
        yg = y.float().to(DEV)[..., None].requires_grad_(True)
        sd = srk.losses.SinkhornDistance(0.5, 50, "none")
        cost, pi, _ = sd(xg, yg)
        cost.sum().backward()
        assert int(sd.last_iterations) == K64 and tuple(cost.shape) == (3,) and tuple(pi.shape) == (3, N, M), (N, M)
        for have, want in ((cost.detach(), cost64.detach()), (xg.grad[..., 0], x64.grad), (yg.grad[..., 0], y64.grad)):
            torch.testing.assert_close(have.double().cpu(), want, rtol=1e-4, atol=1e-6)


def test_stepper_reports_the_wasser_head(srk):
    from oracle import esrgan_oracle as O
    st = _stepper(srk)
    lr, hr = O.jet_images(3, 1, 32, 32, 12, 2)
    lr, hr = lr.to(DEV), hr.to(DEV)
    with torch.no_grad():
        gen = [st.generator(lr), st.generator.srs]
    gt = [hr, hr ** st.scaling_power]
    want = [srk.losses.wasser_loss(gen[k], gt[k], 0.1) for k in range(2)]
    out = st.gan_step(lr, hr)
    s = st.loss_scalars(out)
    for k, name in enumerate(("wasser_loss", "wasser_loss_pow")):
        w = want[k].item()
        assert w > 0 and abs(s[name] - w) <= 1e-5 * max(1.0, abs(w)), (name, s[name], w)
    assert s["wasser_dist"] == 0.0 and s["wasser_dist_pow"] == 0.0
    # the head off (default): reported as 0.0, as before
    st0 = importlib.import_module("super-resolution_amd.train").Stepper(workload="gan", res_blocks=1, filters=16, device=DEV, hr=32,
                                                                         factor=2, res_scale=0.1)
    assert st0.loss_scalars(st0.gan_step(lr, hr))["wasser_loss"] == 0.0


def test_two_d_streams_equal_one(srk, monkeypatch):
    from oracle import esrgan_oracle as O
    lr, hr = O.jet_images(3, 1, 32, 32, 7, 2)
    lr, hr = lr.to(DEV), hr.to(DEV)
    res = []
    for mode in ("1", "0"):
        monkeypatch.setenv("SRK_D_STREAMS", mode)
        st = _stepper(srk)
        assert (st._d_streams is not None) == (mode == "1")
        loss_G, _, _, parts = st.g_phase_loss(lr, hr)
        loss_G.backward()
        torch.cuda.synchronize()
        res.append(([parts[k]["wasser"].clone() for k in range(2)], st.generator.conv1.weight.grad.clone()))
    for k in range(2):
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-8)
