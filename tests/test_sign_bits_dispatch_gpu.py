"""Sign bits across dispatch changes.  In the 16-bit modes a dense block's forward sequence writes the sign bits of its LeakyReLU outputs
and its data-gradient sequence reads them instead of the mask slices (engine.py _drb_forward / _drb_backward).  The bit layout belongs to
the kernel form that runs (one-conv 8- / 16-row tiles, the M16 chain kernel), so the engine uses the bits only when both sequences report
the same layout tag, which it caches per geometry and dispatch generation.  These tests change the dispatch BETWEEN a block's forward and
its backward -- the chain forms' rest after a recovered time-out running out inside the library, debug switches thrown by the caller --
and hold the generator to a twin that reads the mask tensors: every parameter gradient bit for bit, and at every launch the bits a
data-gradient sequence reads were written under the layout it reads them in.

The rest is entered with srk_debug_chain_set(0, k) only: it launches nothing and injects no fault.  At batch 8 x 128 x 128 a dense block
is 256 sixteen-row tiles: the one-conv form is the 16-row kernel (mt = 4) and both sequences are chain-eligible, so one RRDB makes six
sequence calls that count the rest down (three forward, three backward) per iteration."""
import ctypes as C
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import esrgan_oracle as O  # noqa: E402  (initial weights only)

pytestmark = pytest.mark.gpu
FMT = {"fp16": 7, "bf16s": 8}
SCALE = 1024.0          # loss scale (an exact power of two, as train.Stepper's GradScaler uses for fp16)


@pytest.fixture(scope="module")
def srk():
    return importlib.import_module("super-resolution_amd")


@pytest.fixture(scope="module")
def L(srk):
    return srk._lib


@pytest.fixture(autouse=True)
def _restore(L):
    yield
    lib = L.lib()
    lib.srk_debug_chain_set(0, 0)
    lib.srk_debug_set_h16_chain(1)
    lib.srk_debug_set_h16_chain_m16(1)
    lib.srk_debug_set_h16_mt(0)


_SD = {}


def _pair(srk, mode, R):
    """the generator under test (sign bits on) and its twin (same weights, mask tensors), both in 16-bit storage `mode`"""
    if R not in _SD:
        _SD[R] = O.default_init_generator(7, channels=3, filters=64, num_res_blocks=R, num_upsample=1)
    gens = []
    for bits in (True, False):
        g = srk.GeneratorRRDB(3, filters=64, num_res_blocks=R, num_upsample=1).cuda()
        g.load_state_dict(_SD[R])
        g._engine.precision = mode
        g._engine.sign_bits = bits
        gens.append(g)
    return gens


def _data():
    g = torch.Generator().manual_seed(17)
    x = torch.rand(8, 3, 128, 128, generator=g)
    t = torch.rand(8, 3, 256, 256, generator=g)
    return x.cuda(), t.cuda()


def _seq_kernel(L, calls):
    arr = (L.ConvArgs * len(calls))()
    for a, (x, wp, bias, y, kw) in zip(arr, calls):
        L._fill_conv_args(a, x, wp, bias, y, **kw)
    buf = C.create_string_buffer(96)
    L.check(L.lib().srk_conv3x3_seq_kernel_name(arr, len(calls), buf, 96), "srk_conv3x3_seq_kernel_name")
    return buf.value.decode()


class Recorder:
    """Wraps _lib.conv3x3_seq.  Before every call it asks the library afresh which layout tag the sequence's launches will use
    (conv_seq_signs: srk_chain_resting(false) -- the question does not count the rest down) and which kernel they go to.  A sequence
    that writes sign bits records its fresh tag under the storage of its buffer; one that reads sign bits must find its fresh tag equal
    to the recorded one.  That catches a layout mismatch even where the wrong masks happen to change no gradient.  Also counts the
    engine's own conv_seq_signs queries per geometry and dispatch generation."""

    def __init__(self, L, monkeypatch):
        self.L = L
        self._seq, self._signs = L.conv3x3_seq, L.conv_seq_signs
        self.tags = {}              # storage of a sign-bit buffer -> fresh tag of the forward sequence that wrote it
        self.bad = []               # (what, ...) of every violated invariant
        self.fwd, self.bwd = [], []  # per dense-block sequence of the current iteration: (kernel name, fresh tag[, reads bits])
        self.queries = {}           # (N, H, W, generation) -> conv_seq_signs calls made by the engine
        monkeypatch.setattr(L, "conv3x3_seq", self.seq)
        monkeypatch.setattr(L, "conv_seq_signs", self.signs)

    def new_iteration(self):
        self.fwd, self.bwd = [], []

    def signs(self, calls):
        kw = calls[0][4]
        gen = self.L.dispatch_generation() if hasattr(self.L, "dispatch_generation") else None
        key = (kw["N"], kw["H"], kw["W"], gen)
        self.queries[key] = self.queries.get(key, 0) + 1
        return self._signs(calls)

    def seq(self, calls):
        kws = [c[4] for c in calls]
        dense = len(calls) == 5 and all(k.get("Cout") == 64 for k in kws)
        if dense:
            _, tag = self._signs(calls)
            name = _seq_kernel(self.L, calls)
            writes = [k["signs_out"] for k in kws if k.get("signs_out") is not None]
            reads = [k["mask_signs"] for k in kws if k.get("mask_signs") is not None]
            for s in writes:
                self.tags[s.untyped_storage().data_ptr()] = tag
            for s in reads:
                want = self.tags.get(s.untyped_storage().data_ptr())
                if want != tag:
                    wrote = "no recorded writer" if want is None else f"tag {want:#x}"
                    self.bad.append(("layout", f"bits written under {wrote} read by a sequence whose launches use {tag:#x} ({name or 'one conv'})"))
            if any("mask_slope" in k for k in kws):
                self.bwd.append((name, tag, bool(reads)))
            else:
                self.fwd.append((name, tag))
        return self._seq(calls)


def _grads(gen):
    out = {k: p.grad.detach().clone() for k, p in gen.named_parameters() if p.grad is not None}
    assert len(out) == sum(1 for p in gen.parameters() if p.requires_grad)       # (power and multiplier carry none)
    return out


def _iteration(gen, x, t, between=None):
    gen.zero_grad(set_to_none=True)
    y = gen(x)
    if between is not None:
        between()
    ((y - t).abs().mean() * SCALE).backward()
    return _grads(gen)


def _run(L, gen, x, t, iters, k, rec=None, between=None):
    """`iters` iterations from a rest of k sequence calls; per iteration: (gradients, off_calls after it, off_calls before it, recorder
    fwd / bwd lists).  `between`: {iteration: fn} called after that iteration's forward, before its backward."""
    L.check(L.lib().srk_debug_chain_set(0, k), "srk_debug_chain_set")
    out = []
    for i in range(iters):
        before = L.chain_stats()["off_calls"]
        if rec is not None:
            rec.new_iteration()
        g = _iteration(gen, x, t, (between or {}).get(i))
        torch.cuda.synchronize()
        out.append((g, L.chain_stats()["off_calls"], before, list(rec.fwd) if rec else None, list(rec.bwd) if rec else None))
    return out


def _diff(a, b):
    """names of the gradients that are not bit-identical"""
    return sorted(n for n in a if not torch.equal(a[n], b[n]))


def _tags(mode):
    f = FMT[mode]
    return {"one16": 16 | (f << 8), "m16": 16 | 0x40 | (f << 8)}


def _check_pair(L, srk, mode, R, k, iters, monkeypatch, between=None, setup=None):
    """runs the twin, then the generator under test, through the same schedule (`setup` before each); returns the generator's
    per-iteration records"""
    gen, twin = _pair(srk, mode, R)
    x, t = _data()
    if setup:
        setup()
    ref = _run(L, twin, x, t, iters, k, between=between)
    if setup:
        setup()
    rec = Recorder(L, monkeypatch)
    got = _run(L, gen, x, t, iters, k, rec, between=between)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a[1] == b[1], (i, a[1], b[1])            # both went through the same countdown
        d = _diff(a[0], b[0])
        assert not d, f"iteration {i}: {len(d)} gradients differ from the mask-tensor twin, e.g. {d[:4]}"
    assert not rec.bad, rec.bad[:4]
    return got, rec


def _bits_used_again(got, R):
    """every iteration that ran entirely outside the rest reads sign bits in every data-gradient sequence"""
    for i, (_, after, before, fwd, bwd) in enumerate(got):
        if before == 0:
            assert len(bwd) == 3 * R, (i, len(bwd))
            assert all(r for _, _, r in bwd), f"iteration {i}: data-gradient sequences without sign bits: {bwd}"


# ---------------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("mode", ["fp16", "bf16s"])
def test_mask_tensor_twin_is_deterministic(srk, L, mode):
    """the yardstick of the tests below: the twin (mask tensors) run after run with no rest, bit for bit; and the generator reading
    sign bits, with no rest, equals it"""
    gen, twin = _pair(srk, mode, 1)
    x, t = _data()
    ref = _run(L, twin, x, t, 3, 0)
    for i in (1, 2):
        d = _diff(ref[i][0], ref[0][0])
        assert not d, (i, d[:4])
    got = _run(L, gen, x, t, 2, 0)
    for i in (0, 1):
        d = _diff(got[i][0], ref[0][0])
        assert not d, (i, d[:4])


# -------------------------------------------------------------------------------------------------------------- countdown sweep
@pytest.mark.parametrize("mode", ["fp16", "bf16s"])
@pytest.mark.parametrize("k", list(range(14)))
def test_rest_ending_anywhere_in_an_iteration(srk, L, mode, k, monkeypatch):
    """R = 1 (six counting sequence calls per iteration), rest of k = 0..13 calls, three iterations: the rest runs out in every position
    of the first three iterations -- between a block's forward and its backward included.  Gradients bit-identical to the twin,
    every read of sign bits in the layout they were written in, bits back in use once an iteration runs entirely outside the rest."""
    got, rec = _check_pair(L, srk, mode, 1, k, 3, monkeypatch)
    tags = _tags(mode)
    for i, (_, after, before, fwd, bwd) in enumerate(got):
        assert after == max(0, k - 6 * (i + 1)), (i, after)      # the count the positions above rely on
        assert len(fwd) == 3 and len(bwd) == 3
    # not vacuous: resting sequences go conv by conv in the 16-row form; the others are ONE M16 chain launch
    seqs = [s for _, _, _, fwd, bwd in got for s in fwd + bwd]
    for j, s in enumerate(seqs):
        if j < k:
            assert s[0] == "" and s[1] == tags["one16"], (j, s)
        else:
            assert s[0].startswith("conv3x3_h16_chain_kernel<") and s[1] == tags["m16"], (j, s)
    _bits_used_again(got, 1)


@pytest.mark.parametrize("mode", ["fp16", "bf16s"])
@pytest.mark.parametrize("k", [4, 5, 7, 11])
def test_rest_ending_mid_iteration_with_the_32x32_chain_layout(srk, L, mode, k, monkeypatch):
    """control: with the 32x32x16 chain kernel (h16_chain_m16 = 0) the chain writes the 16-row one-conv layout, so a stale decision
    reads the right bits anyway -- this passes with or without a fresh decision after the rest"""
    got, rec = _check_pair(L, srk, mode, 1, k, 3, monkeypatch, setup=lambda: L.lib().srk_debug_set_h16_chain_m16(0))
    assert all(s[1] == _tags(mode)["one16"] for _, _, _, fwd, bwd in got for s in fwd + bwd)
    _bits_used_again(got, 1)


@pytest.mark.parametrize("mode", ["fp16", "bf16s"])
def test_first_strike_rest(srk, L, mode, monkeypatch):
    """R = 2 (twelve counting calls per iteration) after a first strike: srk_chain_recover rests the chain forms for 64 calls, which run
    out at the fourth forward sequence of the sixth iteration"""
    got, rec = _check_pair(L, srk, mode, 2, 64, 7, monkeypatch)
    assert [a for _, a, _, _, _ in got] == [52, 40, 28, 16, 4, 0, 0]
    assert [s[0] != "" for s in got[5][3]] == [False] * 4 + [True] * 2
    _bits_used_again(got, 2)
    assert got[6][2] == 0


# ------------------------------------------------------------------------------------------- switches thrown between forward and backward
FLIPS = [("srk_debug_set_h16_chain", 1, 0), ("srk_debug_set_h16_chain", 0, 1), ("srk_debug_set_h16_chain_m16", 1, 0),
         ("srk_debug_set_h16_mt", 0, 1), ("srk_debug_set_h16_mt", 0, 2), ("srk_debug_set_h16_mt", 1, 2), ("srk_debug_set_h16_mt", 2, 1)]


@pytest.mark.parametrize("mode", ["fp16", "bf16s"])
@pytest.mark.parametrize("setter,a,b", FLIPS)
def test_switch_thrown_between_forward_and_backward(srk, L, mode, setter, a, b, monkeypatch):
    """a kernel-form switch thrown after the first iteration's forward, before its backward: gradients bit-identical to the twin (which
    sees the same flip), no read of bits in a layout they were not written in, and the bits in use again in the next iteration"""
    fn = getattr(L.lib(), setter)
    got, rec = _check_pair(L, srk, mode, 1, 0, 2, monkeypatch, between={0: lambda: fn(b)}, setup=lambda: fn(a))
    _bits_used_again(got[1:], 1)


# ------------------------------------------------------------------------------------------------------------- the dispatch generation
def test_dispatch_generation_is_steady_over_iterations(srk, L, monkeypatch):
    """nothing moves the generation in steady state, so the engine asks the library for a tag at most twice (forward, backward) per
    geometry and generation"""
    gen, _ = _pair(srk, "fp16", 1)
    x, t = _data()
    rec = Recorder(L, monkeypatch)
    _iteration(gen, x, t)
    g0 = L.dispatch_generation()
    for _ in range(3):
        _iteration(gen, x, t)
    torch.cuda.synchronize()
    assert L.dispatch_generation() == g0
    assert rec.queries and max(rec.queries.values()) <= 2, rec.queries


def test_dispatch_generation_moves_on_every_switch(L):
    lib = L.lib()
    steps = [("srk_debug_set_h16_mt", 4), ("srk_debug_set_h16_mt", 0), ("srk_debug_set_h16_chain", 0), ("srk_debug_set_h16_chain", 1),
             ("srk_debug_set_h16_chain_m16", 0), ("srk_debug_set_h16_chain_m16", 1), ("srk_debug_set_w42_chain", 0),
             ("srk_debug_set_w42_chain", 1), ("srk_debug_set_wino42_nmt", 1), ("srk_debug_set_wino42_nmt", 0),
             ("srk_debug_set_conv_small", 2), ("srk_debug_set_conv_small", 1), ("srk_debug_set_wgrad_w22_form", 1),
             ("srk_debug_set_wgrad_w22_form", -1)]
    for name, v in steps:
        g = L.dispatch_generation()
        getattr(lib, name)(v)
        assert L.dispatch_generation() == g + 1, name
    g = L.dispatch_generation()
    L.check(lib.srk_debug_chain_set(0, 0), "srk_debug_chain_set")
    assert L.dispatch_generation() == g + 1
    g = L.dispatch_generation()
    assert L.chain_recover() == 0               # (no fault pending: nothing else changes)
    assert L.dispatch_generation() == g + 1


def test_dispatch_generation_moves_once_when_the_rest_runs_out(L):
    """srk_debug_chain_set(0, 3), then four calls of one dense block's forward sequence: the first three go conv by conv and count the rest
    down; the generation moves on the third -- which still rests -- so that a question asked before the fourth already sees it"""
    import srk_testutil as U
    from test_h16_gpu import _dense_block_calls
    D, out, calls, keep = _dense_block_calls(U, 7, 8, 128, 128, False, 800)
    L.check(L.lib().srk_debug_chain_set(0, 3), "srk_debug_chain_set")
    g0 = L.dispatch_generation()
    seen = []
    for _ in range(4):
        name = _seq_kernel(L, calls)
        L.conv3x3_seq(calls)
        seen.append((name != "", L.chain_stats()["off_calls"], L.dispatch_generation() - g0))
    torch.cuda.synchronize()
    assert seen == [(False, 2, 0), (False, 1, 0), (False, 0, 1), (True, 0, 1)], seen
