"""Self-test of the float64 reference and its per-element bound (tests/f64ref.py), CPU only (no libsrk.so):
  - the reference agrees with oracle.esrgan_oracle / autograd and with oracle/conv_ref.c for every option srk_conv_args and
    srk_wgrad_args carry;
  - the bound admits a correct float32 result at K = 9 ... 2880;
  - the bound rejects subtly wrong results (a dropped tap, swapped channels, a missing bias row, a mis-scaled beta, a bf16 operand,
    a weight-gradient pixel split counted twice) at the shapes of tests/test_launch_set_f64_gpu.py with the tau of its families."""
import pytest
import torch

import f64ref as R
from oracle import c_ref
from oracle import esrgan_oracle as O

G = torch.Generator().manual_seed(1234)


def rnd(*shape, scale=1.0):
    return scale * torch.randn(*shape, generator=G)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def weights(co, ci):
    return rnd(co, ci, 3, 3, scale=1.0 / (3.0 * ci ** 0.5))


TAU_F32 = R.TAU["f32_direct"]       # an fp32 result computed another way (the oracle, torch's CPU conv)
ONE_ROUNDING = 1.0 + 1e-6           # a float64 result rounded once to float32


FP32_FAMILIES = ["f32_direct", "f32_wino", "f32_small"]
WGRAD_FAMILIES = ["f32_direct_wgrad", "f32_wino_wgrad", "f32_small_wgrad"]


def passes(got, ref, A, tau):
    try:
        R.check(got, ref, A, tau)
        return True
    except AssertionError:
        return False


# ----------------------------------------------------------------------------------------------------- reference vs the oracles
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("slope", [1.0, 0.2])
def test_conv_matches_c_reference(stride, slope):
    """conv_ref.c accumulates in double and rounds once: within one rounding of the float64 reference"""
    x, w, b = rnd(2, 5, 9, 11), weights(7, 5), rnd(7, scale=0.1)
    y = torch.from_numpy(c_ref.conv3x3(x.numpy(), w.numpy(), b.numpy(), stride=stride, slope=slope))
    ref, A = R.conv(nhwc(x), w, b, stride=stride, slope=slope)
    assert R.worst(nhwc(y), ref, A) <= 1.0 + 1e-6


def test_ps_store_matches_c_pixel_shuffle():
    t = rnd(2, 12, 5, 6)
    ps = torch.from_numpy(c_ref.pixel_shuffle2(t.numpy()))
    packed = nhwc(t)[..., R.ps_rows(torch.arange(12))]          # OIHW channel order -> packed-o order
    assert torch.equal(R.ps_store_nhwc(packed), nhwc(ps))


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_epilogue_matches_oracle(stride):
    """bias, alpha, r1*beta1 + r2*beta2, LeakyReLU slope, the LeakyReLU' mask and in_slope against esrgan_oracle's ops"""
    x, w, b = rnd(2, 8, 10, 12), weights(6, 8), rnd(6, scale=0.1)
    t = O.conv3x3(O.lrelu(x, 0.2), w, b, stride)
    r1, r2, m = rnd(*t.shape), rnd(*t.shape), rnd(*t.shape)
    want = O.lrelu(0.2 * t + 0.7 * r1 - 1.5 * r2, 0.01) * torch.where(m > 0, 1.0, 0.2)
    ref, A = R.conv(nhwc(x), w, b, stride=stride, alpha=0.2, r1=nhwc(r1), beta1=0.7, r2=nhwc(r2), beta2=-1.5, slope=0.01,
                    mask=nhwc(m), mask_slope=0.2, in_slope=0.2)
    R.check(nhwc(want), ref, A, TAU_F32)
    assert R.worst(nhwc(want), ref, A) < 4.0


def test_unshuffle_input_and_ps_out_match_oracle():
    """in_mode unshuffle reads the inverse of nn.PixelShuffle(2); ps_out stores through it (packed-o weights and bias)"""
    cps = 4
    logical = rnd(2, 4 * cps, 6, 7)                     # logical channel k*Cps + c
    oihw_order = logical.reshape(2, 4, cps, 6, 7).transpose(1, 2).reshape(2, 4 * cps, 6, 7)   # channel 4c + k
    mem = O.pixel_shuffle(oihw_order)
    w, b = weights(12, 4 * cps), rnd(12, scale=0.1)
    ref, A = R.conv(nhwc(mem), w, b, in_mode=1)
    R.check(nhwc(O.conv3x3(logical, w, b)), ref, A, TAU_F32)
    # ps_out: a conv + PixelShuffle(2) with the packed weights
    x = rnd(2, 5, 6, 7)
    w, b = weights(12, 5), rnd(12, scale=0.1)
    want = O.pixel_shuffle(O.conv3x3(x, w, b))
    ref, A = R.conv(nhwc(x), R.ps_rows(w), R.ps_rows(b), ps_out=True)
    R.check(nhwc(want), ref, A, TAU_F32)


@pytest.mark.parametrize("ps", [False, True])
def test_data_gradient_matches_autograd(ps):
    """transposed, tap-flipped weights with a c_begin slice and scale = the input gradient of the conv (ps: of conv + PixelShuffle)"""
    x = rnd(2, 10, 7, 9, scale=1.0).double().requires_grad_(True)
    w = weights(8, 10).double()
    y = O.conv3x3(x, w, None)
    if ps:
        y = O.pixel_shuffle(y)
    dy = rnd(*y.shape).double()
    (dx,) = torch.autograd.grad(y, x, dy)
    c_begin, c_len, scale = 3, 5, 0.25
    wd = R.dgrad_weight(w, c_begin, c_len, scale, ps=ps)
    ref, A = R.conv(nhwc(dy.float()), wd, None, in_mode=1 if ps else 0)
    R.check(nhwc(scale * dx[:, c_begin:c_begin + c_len]).float(), ref, A, ONE_ROUNDING)


@pytest.mark.parametrize("stride,dy_mode,in_slope,accumulate", [(1, 0, 1.0, False), (2, 0, 0.2, True), (1, 1, 1.0, True)])
def test_weight_gradient_matches_autograd(stride, dy_mode, in_slope, accumulate):
    x = rnd(3, 6, 9, 8)
    w = weights(8, 6).double().requires_grad_(True)
    b = torch.zeros(8, dtype=torch.float64, requires_grad=True)
    y = O.conv3x3(O.lrelu(x.double(), in_slope), w, b, stride)
    if dy_mode == 1:
        y = O.pixel_shuffle(y)
    dy = rnd(*y.shape)
    dw, db = torch.autograd.grad(y, (w, b), dy.double())
    dw0, db0 = rnd(8, 6, 3, 3), rnd(8)
    scale = 0.5
    rw, Aw, rb, Ab = R.wgrad(nhwc(x), nhwc(dy), Cout=8, stride=stride, dy_mode=dy_mode, in_slope=in_slope, scale=scale,
                             accumulate=accumulate, dw0=dw0, db0=db0)
    acc = 1.0 if accumulate else 0.0
    R.check((scale * dw + acc * dw0.double()).float(), rw, Aw, ONE_ROUNDING)
    R.check((scale * db + acc * db0.double()).float(), rb, Ab, ONE_ROUNDING)


# ----------------------------------------------------------------------------------------------------- the bound admits fp32
@pytest.mark.parametrize("cin", [1, 4, 16, 64, 192, 320])
def test_bound_admits_float32(cin):
    """torch's float32 CPU conv passes every fp32 conv family's tau, K = 9 * cin = 9 ... 2880; its weight gradient (4 images of
    32 x 32) the tau of the production weight-gradient batch (wino24).  (The direct and single-channel weight-gradient families are
    tighter than a plain serial fp32 sum over few pixels reaches: a weight gradient's ratio shrinks with the pixel count, and theirs
    were calibrated at the step's N = 32 / 16 and 64..256-pixel images.)"""
    x, w, b = rnd(1, cin, 32, 32), weights(64, cin), rnd(64, scale=0.1)
    got = nhwc(torch.nn.functional.conv2d(x, w, b, padding=1))
    ref, A = R.conv(nhwc(x), w, b)
    R.check(got, ref, A, min(R.TAU[f] for f in FP32_FAMILIES))
    dy = rnd(4, 64, 32, 32)
    xs = rnd(4, cin, 32, 32)
    dw = torch.nn.grad.conv2d_weight(xs, (64, cin, 3, 3), dy, padding=1)
    rw, Aw, _, _ = R.wgrad(nhwc(xs), nhwc(dy), Cout=64, want_db=False)
    R.check(dw, rw, Aw, R.TAU["f32_wino_wgrad"])


# ----------------------------------------------------------------------------------------------------- the bound rejects faults
@pytest.fixture(scope="module")
def block_conv():
    """conv 5 of a dense block at the trunk geometry (one image of 64 x 64, 320 -> 64, K = 2880), with the residual epilogue"""
    x, w, b = rnd(1, 320, 64, 64), weights(64, 320), rnd(64, scale=0.1)
    r1 = rnd(1, 64, 64, 64)
    ref, A = R.conv(nhwc(x), w, b, alpha=0.2, r1=nhwc(r1), beta1=1.0)
    got = nhwc(0.2 * torch.nn.functional.conv2d(x, w, b, padding=1) + r1)
    return dict(x=x, w=w, b=b, r1=r1, ref=ref, A=A, got=got)


@pytest.mark.parametrize("fam", FP32_FAMILIES)
def test_bound_rejects_conv_faults(block_conv, fam):
    bc, tau = block_conv, R.TAU[fam]
    x, w, got, ref, A = bc["x"], bc["w"], bc["got"], bc["ref"], bc["A"]
    assert passes(got, ref, A, tau)
    # one tap (r, s) = (2, 1) dropped at one border pixel (h = 0, w = 17): all output channels of that pixel
    bad = got.clone()
    bad[0, 0, 17] -= 0.2 * torch.einsum("oc,c->o", w[:, :, 2, 1], x[0, :, 1, 17])
    assert not passes(bad, ref, A, tau), "dropped tap admitted"
    # output channels 1 and 2 swapped (inside the group of 4 channels 0..3)
    bad = got.clone()
    bad[..., [1, 2]] = bad[..., [2, 1]]
    assert not passes(bad, ref, A, tau), "swapped channels admitted"
    # bias missing on the last tile row of the image
    bad = got.clone()
    bad[0, -2:] -= 0.2 * bc["b"]
    assert not passes(bad, ref, A, tau), "missing bias row admitted"
    # beta1 applied as beta1 * (1 + 2^-10)
    bad = got + 2.0 ** -10 * nhwc(bc["r1"])
    assert not passes(bad, ref, A, tau), "beta1 * (1 + 2^-10) admitted"
    # one operand rounded to bf16 (SRK_PRECISION=bf16)
    bad = nhwc(0.2 * torch.nn.functional.conv2d(x.bfloat16().float(), w, bc["b"], padding=1) + bc["r1"])
    assert not passes(bad, ref, A, tau), "bf16 operand admitted"


def test_bound_rejects_wgrad_split_faults():
    """the five-problem batch's largest problem (320 -> 64) over N = 2 images of 64 x 64: one pixel split's partial block counted
    twice and another's dropped.  With the loosest weight-gradient tau (wino24's); the other families' are tighter."""
    tau = max(R.TAU[f] for f in WGRAD_FAMILIES)
    x, dy = rnd(2, 320, 64, 64), rnd(2, 64, 64, 64)
    rw, Aw, rb, Ab = R.wgrad(nhwc(x), nhwc(dy), Cout=64, scale=0.2)
    got = 0.2 * torch.nn.grad.conv2d_weight(x, (64, 320, 3, 3), dy, padding=1)
    assert passes(got, rw, Aw, tau)

    def partial(img, rows):                  # the contribution of one pixel split (16 rows of one image)
        d = torch.zeros_like(dy[img:img + 1])
        d[..., rows, :] = dy[img:img + 1, :, rows, :]
        return 0.2 * torch.nn.grad.conv2d_weight(x[img:img + 1], (64, 320, 3, 3), d, padding=1)
    bad = got + partial(0, slice(16, 32)) - partial(1, slice(48, 64))
    assert not passes(bad, rw, Aw, tau), "split counted twice / dropped admitted"
    # the bias gradient of the same fault
    gb = 0.2 * dy.sum(dim=(0, 2, 3))
    assert passes(gb, rb, Ab, tau)
    bad_b = gb + 0.2 * dy[0, :, 16:32].sum(dim=(1, 2)) - 0.2 * dy[1, :, 48:64].sum(dim=(1, 2))
    assert not passes(bad_b, rb, Ab, tau)


def _split_bf16(t):
    hi = t.bfloat16().float()
    return hi, (t - hi).bfloat16().float()


def split_bf16_ratio(cin):
    """worst err / (2^-24 A) of the split-bf16 (bf16x3) product, emulated: hi*hi + hi*lo + lo*hi, fp32 accumulate, at K = 9 cin"""
    x, w = rnd(1, cin, 32, 32), weights(64, cin)
    xh, xl = _split_bf16(x)
    wh, wl = _split_bf16(w)
    conv = lambda a, b: torch.nn.functional.conv2d(a, b, padding=1)        # noqa: E731
    got = nhwc(conv(xh, wh) + conv(xh, wl) + conv(xl, wh))
    ref, A = R.conv(nhwc(x), w)
    return R.worst(got, ref, A)


def test_fp32_taus_below_bf16_rejection():
    """every fp32 family's tau rejects a plain-bf16 operand by a wide margin at every K of the launch set; the split-bf16 ratios
    are printed (a fp32 tau within 4x of them cannot tell exact fp32 from split-bf16 -- see TAU's comment)"""
    for cin in (16, 64, 320):
        x, w = rnd(1, cin, 32, 32), weights(64, cin)
        ref, A = R.conv(nhwc(x), w)
        bf = R.worst(nhwc(torch.nn.functional.conv2d(x.bfloat16().float(), w, padding=1)), ref, A)
        assert max(R.TAU[f] for f in FP32_FAMILIES + WGRAD_FAMILIES) * 4 < bf, (cin, bf)
        print(f"K={9 * cin}: bf16 operand {bf:.1f}, split-bf16 {split_bf16_ratio(cin):.1f}")
