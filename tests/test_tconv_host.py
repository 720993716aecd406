"""Host-side checks of the ConvTranspose2d(k=2, s=2) path (srk_tconv.hip): the C ABI, the module and the refusal of CPU input."""
import ctypes as C
import os
import pickle
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TCONV = ("srk_tconv2x2_fwd", "srk_tconv2x2_dgrad", "srk_tconv2x2_wgrad")
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "float": C.c_float,
          "size_t": C.c_size_t}


def _prototypes():
    hdr = open(os.path.join(ROOT, "include", "srk.h")).read()
    out = {}
    for name in TCONV:
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        out[name] = [_CTYPE[re.sub(r"\s*\w+$", "", p).replace(" *", "*")] for p in params]
    return out


def test_abi_exports_the_tconv_entries_with_the_header_prototypes(srk):
    lib = srk._lib.lib()
    assert set(TCONV) <= set(srk._lib.EXPORTS)
    for name, types in _prototypes().items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == types, name
    hdr = open(os.path.join(ROOT, "include", "srk.h")).read()
    assert re.search(r"SRK_OP_TCONV2X2_WGRAD\s*=\s*3", hdr) and srk._lib.OP_TCONV2X2_WGRAD == 3
    # the existing op codes keep their values and the new one sizes the split-K partial sums
    assert srk._lib.OP_CONV_FWD == 0 and srk._lib.OP_CONV_DGRAD == 1 and srk._lib.OP_CONV_WGRAD == 2
    n = srk._lib.workspace_bytes(srk._lib.OP_TCONV2X2_WGRAD, 64, 40, 40, 64, 64)
    assert n >= (64 * 256 + 256) * 4 and n % 4 == 0
    assert srk._lib.workspace_bytes(srk._lib.OP_TCONV2X2_WGRAD, 1, 1, 1, 1, 1) == (4 + 4) * 4
    # the ABI refuses null pointers and empty problems before it launches anything
    assert lib.srk_tconv2x2_fwd(None, None, None, None, 1, 1, 1, 1, 1, 1.0, None) == -1
    assert lib.srk_tconv2x2_dgrad(None, None, None, 1, 1, 1, 1, 1, None) == -1
    assert lib.srk_tconv2x2_wgrad(None, None, None, None, 1, 1, 1, 1, 1, 1.0, 0, None, 0, None) == -1
    assert lib.srk_tconv2x2_fwd(16, 16, None, 16, 0, 1, 1, 1, 1, 1.0, None) == -1
    assert lib.srk_tconv2x2_fwd(16, 16, None, 20, 1, 1, 1, 1, 1, 1.0, None) == -3        # y must be 8-byte aligned
    assert lib.srk_tconv2x2_wgrad(16, 16, 16, None, 1, 1, 1, 1, 1, 1.0, 0, 16, 4, None) == -4   # workspace too small


@pytest.mark.parametrize("kw", [dict(kernel_size=3), dict(stride=1), dict(padding=1), dict(output_padding=1), dict(dilation=2),
                                dict(groups=2)])
def test_module_rejects_other_geometries(srk, kw):
    with pytest.raises(NotImplementedError):
        srk.ConvTranspose2x2(16, 16, **kw)


def test_module_matches_nn_conv_transpose2d(srk):
    m = srk.ConvTranspose2x2(16, 16, kernel_size=2, stride=2, padding=0)
    ref = nn.ConvTranspose2d(16, 16, 2, 2)
    assert isinstance(m, nn.ConvTranspose2d) and srk.models.ConvTranspose2x2 is srk.ConvTranspose2x2
    assert [(k, tuple(v.shape)) for k, v in m.named_parameters()] == [(k, tuple(v.shape)) for k, v in ref.named_parameters()]
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    m.load_state_dict(ref.state_dict())
    assert torch.equal(m.weight, ref.weight) and torch.equal(m.bias, ref.bias)
    assert srk.ConvTranspose2x2(3, 5, 2, 2, bias=False).bias is None
    m2 = pickle.loads(pickle.dumps(m))
    assert type(m2) is srk.ConvTranspose2x2 and torch.equal(m2.weight, m.weight) and torch.equal(m2.bias, m.bias)


@pytest.mark.parametrize("kw,n_tconv", [(dict(use_transposed_conv=True), 1), (dict(fully_tconv_upsample=True), 2)])
def test_generator_tconv_stages_are_the_hip_module(srk, kw, n_tconv):
    g = srk.GeneratorRRDB(1, 16, 1, num_upsample=2, res_scale=0.1, **kw)
    tc = [m for m in g.upsampling if isinstance(m, nn.ConvTranspose2d)]
    assert len(tc) == n_tconv and all(type(m) is srk.ConvTranspose2x2 for m in tc)
    assert g.modulewise
    g2 = pickle.loads(pickle.dumps(g))
    assert all(type(m) is srk.ConvTranspose2x2 for m in g2.upsampling if isinstance(m, nn.ConvTranspose2d))


def test_cpu_input_is_refused_before_any_launch(srk):
    L = srk._lib
    m = srk.ConvTranspose2x2(4, 3)
    x = torch.randn(2, 4, 5, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x)
    with pytest.raises(RuntimeError, match="GPU"):
        srk.ops.tconv2x2(x, m.weight, m.bias)
    y = torch.empty(2, 3, 10, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        L.tconv2x2_fwd_flat(x, m.weight.detach(), m.bias.detach(), y)
    with pytest.raises(RuntimeError, match="GPU"):
        L.tconv2x2_dgrad_flat(y, m.weight.detach(), x)
    with pytest.raises(RuntimeError, match="GPU"):
        L.tconv2x2_wgrad_flat(x, y, torch.empty(4, 3, 2, 2), torch.empty(3))
    g = srk.GeneratorRRDB(1, 16, 1, num_upsample=2, fully_tconv_upsample=True)
    with pytest.raises(RuntimeError, match="GPU"):
        g(torch.randn(1, 1, 8, 8))
