"""Host-side checks of the Sinkhorn Wasserstein head (srk_sinkhorn.hip): the C ABI, a float64 restatement of the math pinned to the
reference's own numbers (G18), and the refusals that happen before anything is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("srk_sort_cut", "srk_sinkhorn_fwd", "srk_sinkhorn_bwd", "srk_sinkhorn_plan", "srk_scatter_rows")
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int*": C.c_void_p, "int*": C.c_void_p, "void*": C.c_void_p,
          "int": C.c_int, "float": C.c_float}


def _prototypes():
    hdr = open(os.path.join(ROOT, "include", "srk.h")).read()
    out = {}
    for name in ENTRIES:
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        out[name] = [_CTYPE[re.sub(r"\s*\w+$", "", p).replace(" *", "*")] for p in params]
    return out


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "G18_sinkhorn.npz"))


def _cases(g, prefix):
    return sorted({k.split("/")[0] for k in g.files if k.startswith(prefix)})


def sinkhorn64(x, y, eps, max_iter):
    """Our float64 restatement of the log-domain iterations, per image: x [B, N], y [B, M] -> (cost [B], K, errs).  The marginal
    logs are taken in float32, as the reference builds its marginals in float32."""
    N, M = x.shape[1], y.shape[1]
    a = torch.log(torch.tensor(1.0 / N, dtype=torch.float32) + 1e-8).double()
    b = torch.log(torch.tensor(1.0 / M, dtype=torch.float32) + 1e-8).double()
    Cm = (x[:, :, None] - y[:, None, :]) ** 2
    u = torch.zeros_like(x)
    v = torch.zeros_like(y)
    errs = []
    for _ in range(max_iter):
        u1 = u
        u = eps * (a - torch.logsumexp((-Cm + u[:, :, None] + v[:, None, :]) / eps, -1)) + u
        v = eps * (b - torch.logsumexp((-Cm + u[:, :, None] + v[:, None, :]) / eps, -2)) + v
        err = (u - u1).abs().sum(-1).mean()
        errs.append(float(err.detach()))
        if errs[-1] < 0.1:
            break
    pi = torch.exp((-Cm + u[:, :, None] + v[:, None, :]) / eps)
    return (pi * Cm).sum((-2, -1)), len(errs), errs


def test_abi_exports_the_sinkhorn_entries_with_the_header_prototypes(srk):
    lib = srk._lib.lib()
    assert set(ENTRIES) <= set(srk._lib.EXPORTS)
    for name, types in _prototypes().items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == types, name
    hdr = open(os.path.join(ROOT, "include", "srk.h")).read()
    assert re.search(r"SRK_SORT_CUT_MAX\s*=\s*65536", hdr) and srk._lib.SORT_CUT_MAX == 65536
    # null pointers, empty problems, bad eps / max_iter and oversized images are refused before anything is launched
    assert lib.srk_sort_cut(None, 1, 1, 0.0, None, None, None, None) == -1
    assert lib.srk_sort_cut(16, 1, 65537, 0.0, 16, 16, 16, None) == -1
    assert lib.srk_sinkhorn_fwd(*([16] * 3), 1, 4, 4, 0.0, 10, *([16] * 9)) == -1
    assert lib.srk_sinkhorn_fwd(*([16] * 3), 1, 4, 4, 0.1, 0, *([16] * 9)) == -1
    assert lib.srk_sinkhorn_fwd(*([None] * 3), 1, 4, 4, 0.1, 10, *([None] * 9)) == -1
    assert lib.srk_sinkhorn_bwd(*([16] * 3), 0, 4, 4, 0.1, 10, *([16] * 8)) == -1
    assert lib.srk_sinkhorn_plan(16, 16, 16, 16, 1, 0, 4, 0.1, 16, 16, None) == -1
    assert lib.srk_scatter_rows(None, 16, 16, 1, 4, 16, None) == -1


def test_restatement_reproduces_the_reference_float64_numbers():
    g = _golden()
    for c in _cases(g, "sd_"):
        x = torch.tensor(g[c + "/x"], dtype=torch.float64, requires_grad=True)
        y = torch.tensor(g[c + "/y"], dtype=torch.float64, requires_grad=True)
        eps, max_iter, red = float(g[c + "/eps"]), int(g[c + "/max_iter"]), str(g[c + "/reduction"])
        xb, yb = (x.reshape(1, -1), y.reshape(1, -1)) if x.dim() == 2 else (x[..., 0], y[..., 0])
        cost, K, errs = sinkhorn64(xb, yb, eps, max_iter)
        assert K == int(g[c + "/K64"]), c
        np.testing.assert_allclose(errs, g[c + "/err64"], rtol=1e-9, atol=1e-12, err_msg=c)
        have = {"none": cost if x.dim() == 3 else cost[0], "mean": cost.mean(), "sum": cost.sum()}[red]
        have.sum().backward()
        want = g[c + "/cost64"]
        np.testing.assert_allclose(have.detach().numpy(), want, rtol=1e-9, atol=1e-12, err_msg=c)
        np.testing.assert_allclose(x.grad.numpy(), g[c + "/gx64"], rtol=1e-7, atol=1e-10, err_msg=c)
        np.testing.assert_allclose(y.grad.numpy(), g[c + "/gy64"], rtol=1e-7, atol=1e-10, err_msg=c)


def test_restatement_reproduces_the_reference_wasser_head():
    g = _golden()
    for c in _cases(g, "wl_"):
        gen = torch.tensor(g[c + "/gen"], dtype=torch.float64, requires_grad=True)
        real = torch.tensor(g[c + "/real"], dtype=torch.float64)
        B = gen.shape[0]
        gs, gi = torch.sort(gen.reshape(B, -1), dim=1, stable=True)
        rs, _ = torch.sort(real.reshape(B, -1), dim=1, stable=True)
        n = int((gs > 0).sum(1).max()) or gs.shape[1]
        m = int((rs > 0).sum(1).max()) or rs.shape[1]
        cost, K, _ = sinkhorn64(gs[:, -n:], rs[:, -m:], float(g[c + "/eps"]), int(g[c + "/max_iter"]))
        cost.sum().backward()
        assert K == int(g[c + "/K64"]), c
        np.testing.assert_allclose(cost.sum().item(), float(g[c + "/loss64"]), rtol=1e-9, err_msg=c)
        # tied pixels may swap gradients between themselves (a different sort order): compare sums over groups of equal values
        have, want, vals = gen.grad.reshape(B, -1).numpy(), g[c + "/ggen64"].reshape(B, -1), g[c + "/gen"].reshape(B, -1)
        for b in range(B):
            for val in np.unique(vals[b]):
                sel = vals[b] == val
                np.testing.assert_allclose(have[b][sel].sum(), want[b][sel].sum(), rtol=1e-7, atol=1e-10, err_msg=c)


def test_cpu_input_is_refused_before_any_launch(srk):
    x = torch.rand(2, 8, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        srk.losses.SinkhornDistance(0.1, 10)(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        srk.losses.wasser_loss(torch.rand(2, 1, 4, 4), torch.rand(2, 1, 4, 4), 0.1)


def test_unsupported_arguments_are_refused(srk):
    with pytest.raises(NotImplementedError):
        srk.losses.SinkhornDistance(0.1, 10)(torch.rand(2, 8, 2), torch.rand(2, 8, 2))
    for bad in ("avg", None, "Sum"):
        with pytest.raises(ValueError):
            srk.losses.SinkhornDistance(0.1, 10, bad)
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            srk.losses.SinkhornDistance(eps, 10)
        with pytest.raises(ValueError):
            srk.losses.wasser_loss(torch.rand(2, 1, 4, 4), torch.rand(2, 1, 4, 4), eps)
    with pytest.raises(ValueError):
        srk.losses.SinkhornDistance(0.1, 0)


def test_cut_smaller_matches_the_reference_semantics(srk):
    t = torch.tensor([[-1.0, 0.0, 0.5, 2.0], [0.0, 0.0, 0.0, 3.0]])
    assert torch.equal(srk.losses.cut_smaller(t), t[:, -2:])
    z = torch.zeros(2, 5)
    assert torch.equal(srk.losses.cut_smaller(z), z)          # t[:, -0:] keeps the whole row


def test_stepper_takes_the_wasser_head_arguments(srk):
    import importlib
    import inspect
    sig = inspect.signature(importlib.import_module("super-resolution_amd.train").Stepper.__init__)
    assert sig.parameters["lambda_wasser"].default == 0.0 and sig.parameters["sinkhorn_eps"].default == 0.1
