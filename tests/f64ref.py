"""Float64 CPU reference of the fused 3x3 convolution and its weight gradient (include/srk.h: srk_conv_args, srk_wgrad_args),
with a per-element error bound.  Test infrastructure only; it loads no native code.

Every function takes the tensors the way a launch sees them: NHWC memory views (already sliced to the view's channels), weights in
the order the packed fragments carry them.  For each output element i the reference returns ``ref_i`` in float64 and ``A_i``, the
same operation applied to absolute values (sum |x||w| + |bias|, |r1||beta1|, ...).  A kernel result passes when

    |got_i - ref_i| <= tau * 2^-24 * A_i + FLOOR

with one tau per arithmetic family (TAU below).  A_i only scales the bound, so it is computed in float32.
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
FLOOR = 2.0 ** -120          # only matters where A_i == 0 (all-zero operands)

# Bound factor per arithmetic family: about 4x the worst err_i / (2^-24 A_i) observed over every case of
# tests/test_launch_set_f64_gpu.py (configs[2] and configs[1] launch sets), MI355X (gfx950), 2026-10-15; the observed worst sits next
# to each.  A weight gradient's A_i sums |dy||x| over every pixel while its error grows like the square root of that count, hence
# ratios far below 1 and families of their own.
# Finding: the fp32 Winograd families are NOT separable from split-bf16 per element.  The F(2x4,3x3) chain kernels reach 18.6 at
# K = 576..2880 where the split-bf16 kernel (conv3x3_bf16x3_kernel) measured 24.4 on the same dense-block launches, and the wino24
# weight gradient (1.60) sits above the split-bf16 one (1.54).  The transforms cost the Winograd kernels about the precision that
# dropping the lo*lo product costs split-bf16; plain bf16 operands (thousands) stay far outside every fp32 tau.
TAU = {
    "f32_direct": 27.0,          # direct fp32 MFMA conv (conv3x3_f32_kernel, conv3x3_f32_lw_kernel): observed 6.58
    "f32_wino": 130.0,           # F(2x4,3x3) forward / data gradient, separate and chain kernels: observed 32.4 (K = 144, a
                                 # discriminator layer; 18.6 at K >= 576)
    "f32_small": 21.0,           # small-channel VALU convs (conv3x3_cin_small / _cout_small): observed 5.07
    "f32_direct_wgrad": 0.75,    # direct fp32 MFMA weight gradient (wgrad_f32_kernel + reduce): observed 0.177
    "f32_wino_wgrad": 6.5,       # wino24 weight gradient + reduce: observed 1.60
    "f32_small_wgrad": 0.16,     # single-channel weight gradient (wgrad_c1_kernel + reduce): observed 0.039
    "bf16x3": 100.0,             # split-bf16 (opt-in, no fp32 case uses it): observed 24.4 conv (K 576..2880), 1.54 weight gradient
}


def family(kernel_name: str) -> str:
    """arithmetic family (key of TAU) of a kernel, by the name srk_conv3x3_kernel_name / _wgrad_kernel_name report"""
    n = kernel_name
    if "bf16x3" in n:
        return "bf16x3"
    if n.startswith("wgrad_c1"):
        return "f32_small_wgrad"
    if n.startswith("wgrad_f32_wino"):
        return "f32_wino_wgrad"
    if n.startswith("wgrad_f32_kernel"):
        return "f32_direct_wgrad"
    if "small" in n:
        return "f32_small"
    if "wino" in n:
        return "f32_wino"
    if n.startswith(("conv3x3_f32_kernel", "conv3x3_f32_lw_kernel")):
        return "f32_direct"
    raise KeyError(f"no arithmetic family for kernel {kernel_name!r}")


# ----------------------------------------------------------------------------------------------------------- layout helpers
def lrelu(x, slope):
    return x if slope == 1.0 else torch.where(x > 0, x, x * slope)


def unshuffle_nhwc(m):
    """SRK_IN_UNSHUFFLE: memory [N, 2H, 2W, C] -> logical [N, H, W, 4C], logical channel k*C + c = mem (2h+i, 2w+j, c), k = 2i+j"""
    n, h2, w2, c = m.shape
    return m.reshape(n, h2 // 2, 2, w2 // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * c)


def ps_store_nhwc(t):
    """ps_out: logical [N, OH, OW, M] with packed o = (2i+j)*M/4 + c -> stored [N, 2OH, 2OW, M/4]"""
    n, h, w, m = t.shape
    return t.reshape(n, h, w, 2, 2, m // 4).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, m // 4)


def ps_rows(w):
    """OIHW weight (or [Cout] bias) of a conv followed by nn.PixelShuffle(2) -> rows in packed-o order (x' = 4*(x % (C/4)) + x/(C/4))"""
    c4 = w.shape[0]
    idx = torch.tensor([4 * (o % (c4 // 4)) + o // (c4 // 4) for o in range(c4)])
    return w[idx]


def dgrad_weight(w_oihw, c_begin=0, c_len=None, scale=1.0, ps=False):
    """effective OIHW weight of the data-gradient conv (srk_pack_entry transpose == 1): output c = input channel c_begin + c of the
    forward conv, input k = its output k (packed-o order if ps), taps flipped; times scale"""
    w = ps_rows(w_oihw) if ps else w_oihw
    c_len = c_len or w.shape[1] - c_begin
    return scale * w[:, c_begin:c_begin + c_len].transpose(0, 1).flip(2, 3)


def _to64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _abs32(t):
    return None if t is None else t.detach().to("cpu", torch.float32).abs()


# ----------------------------------------------------------------------------------------------------------- the forward conv
def conv(x, w, bias=None, *, stride=1, in_mode=0, ps_out=False, alpha=1.0, r1=None, beta1=0.0, r2=None, beta2=0.0, slope=1.0,
         mask=None, mask_slope=1.0, in_slope=1.0):
    """srk_conv3x3 on CPU.  x: NHWC memory [N, Hm, Wm, Cx] (in_mode 1: Hm = 2H, Cx = Cin/4); w: [Cout][Cin][3][3] in packed-o order;
    bias [Cout] in packed-o order; r1 / r2 / mask: NHWC at the stored (after ps_out) layout.  Returns (ref float64, A float32), both
    at the stored layout [N, OHs, OWs, Cs]."""
    if in_mode not in (0, 1):
        raise NotImplementedError("in_mode 2 (zero upsample) has no case in the fp32 steps")

    def run(xx, ww, bb, rr1, rr2, is_abs):
        if in_mode == 1:
            xx = unshuffle_nhwc(xx)
        xx = xx.abs() if is_abs else lrelu(xx, in_slope)
        if is_abs and in_slope != 1.0:
            xx = xx * max(1.0, abs(in_slope))
        t = F.conv2d(xx.permute(0, 3, 1, 2), ww, bb, stride=stride, padding=1).permute(0, 2, 3, 1)
        t = t * (abs(alpha) if is_abs else alpha)
        if ps_out:
            t = ps_store_nhwc(t)
        for r, b in ((rr1, beta1), (rr2, beta2)):
            if r is not None:
                t = t + (abs(b) if is_abs else b) * r
        return t

    ref = run(_to64(x), _to64(w), _to64(bias), _to64(r1), _to64(r2), False)
    A = run(_abs32(x), _abs32(w), _abs32(bias), _abs32(r1), _abs32(r2), True)
    ref = lrelu(ref, slope)
    A = A * max(1.0, abs(slope))          # (a sign flip near 0 moves the result by at most the pre-activation error)
    if mask is not None:
        pos = mask.detach().cpu() > 0
        ref = torch.where(pos, ref, ref * mask_slope)
        A = torch.where(pos, A, A * abs(mask_slope))
    return ref, A


# ----------------------------------------------------------------------------------------------------------- the weight gradient
def wgrad(x, dy, *, Cout, stride=1, dy_mode=0, in_slope=1.0, scale=1.0, accumulate=False, dw0=None, db0=None, want_db=True):
    """srk_conv3x3_wgrad on CPU.  x: NHWC [N, H, W, Cin]; dy: NHWC memory [N, OH, OW, Cout] (dy_mode 1: [N, 2OH, 2OW, Cout/4],
    logical channel = packed o, the result un-permuted to OIHW rows on store).  dw0 / db0: contents before the launch (accumulate).
    Returns (dw ref f64 [Cout][Cin][3][3], dw A f32, db ref f64 [Cout] or None, db A or None)."""
    def run(xx, dd, is_abs):
        if dy_mode == 1:
            dd = unshuffle_nhwc(dd)
        xx = xx.abs() * max(1.0, abs(in_slope)) if is_abs else lrelu(xx, in_slope)
        dd = dd.abs() if is_abs else dd
        dwt = torch.nn.grad.conv2d_weight(xx.permute(0, 3, 1, 2), (Cout, xx.shape[3], 3, 3), dd.permute(0, 3, 1, 2),
                                          stride=stride, padding=1)
        dbt = dd.sum(dim=(0, 1, 2))
        if dy_mode == 1:                  # packed o = k*C + c  ->  OIHW row 4c + k
            c = Cout // 4
            inv = torch.empty(Cout, dtype=torch.long)
            for o in range(Cout):
                inv[4 * (o % c) + o // c] = o
            dwt, dbt = dwt[inv], dbt[inv]
        s = abs(scale) if is_abs else scale
        return s * dwt, s * dbt

    dw, db = run(_to64(x), _to64(dy), False)
    Aw, Ab = run(_abs32(x), _abs32(dy), True)
    if accumulate:
        dw, Aw = dw + _to64(dw0), Aw + _abs32(dw0)
        if want_db:
            db, Ab = db + _to64(db0), Ab + _abs32(db0)
    return (dw, Aw, db, Ab) if want_db else (dw, Aw, None, None)


# ----------------------------------------------------------------------------------------------------------- the check
def ratios(got, ref, A, floor=FLOOR):
    """err_i / (2^-24 A_i + floor) per element (float64); NaN / inf in got count as inf"""
    got = got.detach().to("cpu", torch.float64)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    return err / (EPS * A.to(torch.float64) + floor)


def worst(got, ref, A):
    return ratios(got, ref, A).max().item() if ref.numel() else 0.0


def check(got, ref, A, tau, what=""):
    """assert every element satisfies the bound; returns the worst ratio err_i / (2^-24 A_i)"""
    r = ratios(got, ref, A)
    bad = r > tau
    w = r.max().item() if r.numel() else 0.0
    if bad.any():
        idx = [tuple(i) for i in bad.nonzero()[:4].tolist()]
        first = idx[0]
        g = got.detach().cpu()[first].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {r.numel()} elements outside tau={tau} * 2^-24 * A (worst ratio {w:.4g}); "
                             f"first {idx}: got {g!r} ref {ref[first].item()!r} A {A[first].item():.4g}")
    return w
