"""Every convolution / weight-gradient launch of the exact-fp32 training steps, at the geometry the steps launch it with, checked
element by element against float64 (tests/f64ref.py).

The case table CASES below is what one configs[2] step (train.Stepper "gan", batch 32, 64x64 -> 256x256, both discriminators) and one
configs[1] step ("g_only", batch 16) hand to the library: every distinct call of conv3x3 / conv3x3_seq / conv3x3_wgrad /
conv3x3_wgrad_seq / conv3x3_wgrad_batched, recorded by `record_step` (wrappers around those functions) and deduplicated.  Buffers are
named by index within a call, so the views of one dense buffer ([N,H,W,5F] and its gradient mirror) keep their ldc / coff and their
sharing.  Each case
  - rebuilds the call on fresh buffers: the channels a launch may read hold random data, every other channel NaN; a sequence's
    not-yet-written slices are NaN too (each conv must read its predecessors' output, not stale memory);
  - asserts the kernel name recorded with the case (srk_conv3x3_kernel_name / _seq_kernel_name / _wgrad_kernel_name), so the case
    keeps testing the kernel it was recorded for;
  - poisons the LDS of every CU in front of the launch (NaN patterns: a kernel that consumes LDS it never wrote fails);
  - asserts that nothing outside the written slices changed and that no NaN reached a result;
  - checks every output element of a subset of the images (forward / data gradient: each image depends on its own input only) or of
    the whole result (weight gradients sum over every image) against float64 with |got - ref| <= tau * 2^-24 * A + floor.
For a sequence each conv is checked against float64 applied to what it actually read (its predecessors' slices as the GPU wrote
them), so the bound stays per conv.
test_launch_set_is_covered records both steps again and fails when a step launches a kernel no case covers.
"""
import ctypes as C
import importlib
import json
import math

import pytest
import torch

import f64ref

pytestmark = pytest.mark.gpu

L = importlib.import_module("super-resolution_amd")._lib
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------- recording
class _Bufs:
    """buffer ids of one recorded call, in order of first appearance (so equal calls on other buffers compare equal)"""

    def __init__(self):
        self.ptrs, self.shapes, self.spans = {}, [], []

    def id(self, t):
        p = t.data_ptr()
        if p not in self.ptrs:
            span = (p, p + t.numel() * t.element_size())
            for q0, q1 in self.spans:
                assert span[1] <= q0 or q1 <= span[0], "recorded views overlap without being the same buffer"
            self.ptrs[p] = len(self.shapes)
            self.shapes.append(list(t.shape))
            self.spans.append(span)
        else:
            assert self.shapes[self.ptrs[p]] == list(t.shape)
        return self.ptrs[p]


def _conv_sig(bufs, x, wp, bias, y, kw):
    a = L.ConvArgs()
    L._fill_conv_args(a, x, wp, bias, y, **kw)
    assert a.flags == 0 and a.wp_format in (0, 1, 3, 5, 6), "fp32 launches without sign bits expected"
    s = {k: getattr(a, k) for k in ("N", "H", "W", "OH", "OW", "Cin", "Cout", "stride", "in_mode", "ps_out", "wp_format")}
    s.update({k: getattr(a, k) for k in ("alpha", "beta1", "beta2", "slope", "mask_slope", "in_slope")})
    s["bias"] = bias is not None
    for nm, v in (("x", x), ("y", y), ("r1", kw.get("r1")), ("r2", kw.get("r2")), ("mask", kw.get("mask"))):
        if v is not None:
            s[nm] = [bufs.id(v.t), v.coff]
    return s, a


def _wgrad_sig(bufs, x, dy, dw, db, kw):
    assert dw.is_contiguous() and list(dw.shape) == [kw["Cout"], kw["Cin"], 3, 3]
    s = {k: kw.get(k, d) for k, d in (("N", None), ("H", None), ("W", None), ("OH", None), ("OW", None), ("Cin", None),
                                       ("Cout", None), ("stride", 1), ("dy_mode", 0), ("in_slope", 1.0), ("scale", 1.0),
                                       ("accumulate", False), ("precision", 0))}
    s["scale"], s["in_slope"] = float(C.c_float(s["scale"]).value), float(C.c_float(s["in_slope"]).value)
    s["accumulate"] = int(bool(s["accumulate"]))
    s["db"] = db is not None
    s["x"], s["dy"] = [bufs.id(x.t), x.coff], [bufs.id(dy.t), dy.coff]
    return s


class Recorder:
    """Wraps the library's launch functions for the duration of a `with` block; every top-level call is recorded as a case."""
    NAMES = ("conv3x3", "conv3x3_seq", "conv3x3_wgrad", "conv3x3_wgrad_seq", "conv3x3_wgrad_batched")

    def __init__(self, tag):
        self.tag, self.cases, self.depth, self.orig = tag, [], 0, {}

    def _wrap(self, name):
        orig = self.orig[name]

        def f(*a, **kw):
            if self.depth == 0:
                self.cases.append(self._record(name, *a, **kw))
            self.depth += 1
            try:
                return orig(*a, **kw)
            finally:
                self.depth -= 1
        return f

    def _record(self, name, *a, **kw):
        bufs = _Bufs()
        if name == "conv3x3":
            x, wp, bias, y = a
            s, args = _conv_sig(bufs, x, wp, bias, y, kw)
            case = dict(op="seq", convs=[s], kernel=[L._conv_kernel_name(args)])
        elif name == "conv3x3_seq":
            (calls,) = a
            sigs = [_conv_sig(bufs, *c) for c in calls]
            arr = (L.ConvArgs * len(sigs))(*[s[1] for s in sigs])
            buf = C.create_string_buffer(96)
            L.check(L.lib().srk_conv3x3_seq_kernel_name(arr, len(sigs), buf, 96), "srk_conv3x3_seq_kernel_name")
            case = dict(op="seq", convs=[s[0] for s in sigs],
                        kernel=[buf.value.decode()] if buf.value else [L._conv_kernel_name(s[1]) for s in sigs])
        elif name in ("conv3x3_wgrad", "conv3x3_wgrad_seq"):
            calls = [a + (kw,)] if name == "conv3x3_wgrad" else a[0]
            probs = [_wgrad_sig(bufs, *c) for c in calls]
            case = dict(op="wgrad_seq", probs=probs, kernel=[_wgrad_kernel_name_of([p], bufs.shapes) for p in probs])
        else:
            (problems,) = a
            geo = dict(kw)
            probs = [_wgrad_sig(bufs, p["x"], p["dy"], p["dw"], p.get("db"), dict(geo, Cin=p["Cin"], Cout=p["Cout"],
                     scale=p.get("scale", 1.0), accumulate=p.get("accumulate", False), in_slope=p.get("in_slope", 1.0)))
                     for p in problems]
            case = dict(op="wgrad_batched", probs=probs, kernel=[_wgrad_kernel_name_of(probs, bufs.shapes)])
        case["bufs"] = bufs.shapes
        case["step"] = self.tag
        return case

    def __enter__(self):
        for n in self.NAMES:
            self.orig[n] = getattr(L, n)
            setattr(L, n, self._wrap(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(L, n, f)


def _wgrad_arr(probs, shapes):
    """WgradArgs array of recorded problems for the kernel-name query (which launches nothing: the pointers are aligned
    placeholders; ldc / coff are the recorded ones)"""
    arr = (L.WgradArgs * len(probs))()
    for a, p in zip(arr, probs):
        for k in ("N", "H", "W", "OH", "OW", "Cin", "Cout", "stride", "dy_mode", "in_slope", "scale", "accumulate", "precision"):
            setattr(a, k, p[k])
        a.x = a.dy = a.dw = 1 << 20
        a.db = (1 << 20) if p["db"] else None
        a.x_ldc, a.x_coff = shapes[p["x"][0]][3], p["x"][1]
        a.dy_ldc, a.dy_coff = shapes[p["dy"][0]][3], p["dy"][1]
    return arr


def _wgrad_kernel_name_of(probs, shapes):
    """name of the (main) kernel of one weight-gradient launch (len(probs) problems batched), as L.KernelTimer reports it"""
    arr = _wgrad_arr(probs, shapes)
    return L._wgrad_kernel_name(arr, len(probs)) + "+reduce"


STEPS = {"c2": dict(workload="gan", batch=32), "c1": dict(workload="g_only", batch=16)}


def record_step(tag, timer_names=None):
    """one step of the configs[2] ('c2') or configs[1] ('c1') fp32 training workload after one warm-up step; returns the recorded
    calls.  timer_names (a set): receives the kernel names L.KernelTimer reports for the recorded step (detail suffix removed)."""
    train = importlib.import_module("super-resolution_amd.train")
    cfg = STEPS[tag]
    torch.manual_seed(0)
    dev = torch.device("cuda")
    st = train.Stepper(workload=cfg["workload"], res_blocks=23, device=dev, hr=256, factor=4, channels=1)
    st.generator._engine.precision = "f32"
    g = torch.Generator().manual_seed(7)
    hr = 10.0 * torch.rand(cfg["batch"], 1, 256, 256, generator=g) * (torch.rand(cfg["batch"], 1, 256, 256, generator=g) < 0.1)
    lr = torch.nn.functional.avg_pool2d(hr, 4) * 16.0
    lr, hr = lr.to(dev), hr.to(dev)
    st.step(lr, hr)
    torch.cuda.synchronize()
    detail = L.KernelTimer.detail
    L.KernelTimer.detail = True
    try:
        with Recorder(tag) as rec:
            L.KernelTimer.start()
            try:
                st.step(lr, hr)
            finally:
                ran = L.KernelTimer.stop()
    finally:
        L.KernelTimer.detail = detail
    if timer_names is not None:
        timer_names.update(_strip_detail(n) for n in ran)
    del st
    torch.cuda.empty_cache()
    return rec.cases


def _strip_detail(name):
    return name.split(" Cin=")[0].split(" n=")[0]


def dedup(cases):
    """distinct cases, first-seen order; `count` = launches of that signature"""
    out, seen = [], {}
    for c in cases:
        key = json.dumps({k: v for k, v in c.items() if k != "step"}, sort_keys=True)
        if key in seen:
            seen[key]["count"] += 1
            continue
        c = dict(c, count=1)
        seen[key] = c
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------------- replay
def images_of(N):
    """images compared in a forward / data-gradient case: first, last, and two whose tiles sit at other workgroup / XCD positions"""
    return sorted({0, min(5, N - 1), min(N // 2 + 3, N - 1), N - 1})


def _regions_conv(s):
    """(reads, write) of one recorded conv: lists of (buffer, coff, channels, kind)"""
    cx = s["Cin"] // 4 if s["in_mode"] == 1 else s["Cin"]
    cs = s["Cout"] // 4 if s["ps_out"] else s["Cout"]
    reads = [(s["x"][0], s["x"][1], cx, "x")]
    for nm in ("r1", "r2", "mask"):
        if nm in s:
            reads.append((s[nm][0], s[nm][1], cs, nm))
    return reads, (s["y"][0], s["y"][1], cs)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ch(b, coff, c):
    return slice(coff, coff + c)


def _fill(bufs, done, b, chans, gen):
    """random data into the channels `chans` of buffer b that are not filled yet"""
    todo = [ch for ch in chans if not done[b][ch]]
    if not todo:
        return
    shape = list(bufs[b].shape[:3]) + [len(todo)]
    v = torch.randn(shape, generator=gen)
    bufs[b][..., todo] = v.to(bufs[b].device)
    for ch in todo:
        done[b][ch] = True


def _pack(w, fmt):
    co, ci = w.shape[:2]
    src = w.contiguous().cuda()
    dst = torch.empty(L.packed_floats(ci, co, fmt), dtype=torch.float32, device="cuda")
    t = L.PackTable(src.device, fmt)
    t.add(src, dst, M=co, k_off=0, k_len=ci, K_total=ci)
    t.run()
    return dst


def _view(bufs, s, nm, C_):
    return L.View(bufs[s[nm][0]], s[nm][1], C_) if nm in s else None


def run_conv_case(case, tau=None, wp_format=None, seed=0):
    """replays a recorded conv / conv sequence; returns {family: worst ratio}"""
    gen = torch.Generator().manual_seed(seed)
    convs = case["convs"]
    bufs = [torch.full(sh, NAN, dtype=torch.float32, device="cuda") for sh in case["bufs"]]
    done = [[False] * sh[3] for sh in case["bufs"]]
    written = [[False] * sh[3] for sh in case["bufs"]]
    for s in convs:                                   # what each conv reads that no earlier conv of the sequence writes: random
        reads, (yb, yc, yn) = _regions_conv(s)
        for b, coff, c, kind in reads:
            _fill(bufs, done, b, [ch for ch in range(coff, coff + c) if not written[b][ch]], gen)
        for ch in range(yc, yc + yn):
            assert not written[yb][ch], "a sequence writes one slice twice"
            written[yb][ch] = True
    init = [b.clone() for b in bufs]
    ws, bs, calls = [], [], []
    for s in convs:
        fmt = s["wp_format"] if wp_format is None else wp_format
        w = torch.randn(s["Cout"], s["Cin"], 3, 3, generator=gen) / math.sqrt(9 * s["Cin"])
        bias = (0.1 * torch.randn(s["Cout"], generator=gen)).cuda() if s["bias"] else None
        ws.append(w)
        bs.append(bias)
        cx = s["Cin"] // 4 if s["in_mode"] == 1 else s["Cin"]
        cs = s["Cout"] // 4 if s["ps_out"] else s["Cout"]
        kw = {k: s[k] for k in ("N", "H", "W", "OH", "OW", "Cin", "Cout", "stride", "in_mode", "ps_out", "alpha", "slope", "in_slope")}
        kw["wp_format"] = fmt
        for nm, beta in (("r1", "beta1"), ("r2", "beta2"), ("mask", "mask_slope")):
            if nm in s:
                kw[nm], kw[beta] = _view(bufs, s, nm, cs), s[beta]
        calls.append((_view(bufs, s, "x", cx), _pack(w, fmt), bias, _view(bufs, s, "y", cs), kw))
    torch.cuda.synchronize()
    # the kernel this case was recorded for
    arr = (L.ConvArgs * len(calls))()
    for a, (x, wp, bias, y, kw) in zip(arr, calls):
        L._fill_conv_args(a, x, wp, bias, y, **kw)
    if len(calls) > 1:
        buf = C.create_string_buffer(96)
        L.check(L.lib().srk_conv3x3_seq_kernel_name(arr, len(calls), buf, 96), "srk_conv3x3_seq_kernel_name")
        names = [buf.value.decode()] if buf.value else [L._conv_kernel_name(a) for a in arr]
    else:
        names = [L._conv_kernel_name(arr[0])]
    if wp_format is None:
        assert names == case["kernel"], f"dispatch changed: {names} != {case['kernel']}"
    L.poison_lds()
    if len(calls) > 1:
        L.conv3x3_seq(calls)
    else:
        L.conv3x3(*calls[0][:4], **calls[0][4])
    torch.cuda.synchronize()
    # nothing outside the written slices moved; no NaN in a result
    for b, (buf, ini) in enumerate(zip(bufs, init)):
        keep = [ch for ch in range(buf.shape[3]) if not written[b][ch]]
        if keep:
            assert _bits_equal(buf[..., keep], ini[..., keep]), f"buffer {b}: a channel outside the written slices changed"
        wr = [ch for ch in range(buf.shape[3]) if written[b][ch]]
        if wr:
            assert torch.isfinite(buf[..., wr]).all(), f"buffer {b}: non-finite values in a written slice"
    # float64, per conv, on the inputs it read
    imgs = images_of(convs[0]["N"])
    state = [ini[imgs].cpu() for ini in init]
    final = [buf[imgs].cpu() for buf in bufs]
    fams = [f64ref.family(n) for n in names] if len(names) == len(convs) else [f64ref.family(names[0])] * len(convs)
    worst = {}
    for k, (s, (x, wp, bias, y, kw)) in enumerate(zip(convs, calls)):
        cx, cs = x.C, y.C
        rv = {nm: state[s[nm][0]][..., _ch(*s[nm], cs)] for nm in ("r1", "r2", "mask") if nm in s}
        ref, A = f64ref.conv(state[s["x"][0]][..., _ch(*s["x"], cx)], ws[k], None if bias is None else bias.cpu(),
                             stride=s["stride"], in_mode=s["in_mode"], ps_out=bool(s["ps_out"]), alpha=s["alpha"],
                             r1=rv.get("r1"), beta1=s["beta1"], r2=rv.get("r2"), beta2=s["beta2"], slope=s["slope"],
                             mask=rv.get("mask"), mask_slope=s["mask_slope"], in_slope=s["in_slope"])
        got = final[s["y"][0]][..., _ch(*s["y"], cs)]
        t = f64ref.TAU[fams[k]] if tau is None else tau
        r = f64ref.check(got, ref, A, t, what=f"{names} conv {k} (Cin={s['Cin']} Cout={s['Cout']} {s['OH']}x{s['OW']})")
        worst[fams[k]] = max(worst.get(fams[k], 0.0), r)
        state[s["y"][0]][..., _ch(*s["y"], cs)] = got
    return worst


def run_wgrad_case(case, tau=None, precision=None, seed=0):
    """replays a recorded weight-gradient call (one problem, a sequence or a five-problem batch); returns {family: worst ratio}"""
    gen = torch.Generator().manual_seed(seed)
    probs = case["probs"]
    bufs = [torch.full(sh, NAN, dtype=torch.float32, device="cuda") for sh in case["bufs"]]
    done = [[False] * sh[3] for sh in case["bufs"]]
    for p in probs:
        cdy = p["Cout"] // 4 if p["dy_mode"] == 1 else p["Cout"]
        _fill(bufs, done, p["x"][0], range(p["x"][1], p["x"][1] + p["Cin"]), gen)
        _fill(bufs, done, p["dy"][0], range(p["dy"][1], p["dy"][1] + cdy), gen)
    init = [b.clone() for b in bufs]
    G = 256                                         # NaN guard elements on both sides of every dW / db
    outs = []
    for p in probs:
        nw = p["Cout"] * p["Cin"] * 9
        fw = torch.full((nw + 2 * G,), NAN, device="cuda")
        fb = torch.full((p["Cout"] + 2 * G,), NAN, device="cuda") if p["db"] else None
        if p["accumulate"]:
            fw[G:G + nw] = torch.randn(nw, generator=gen).cuda()
            if fb is not None:
                fb[G:G + p["Cout"]] = torch.randn(p["Cout"], generator=gen).cuda()
        outs.append((fw, fb, fw.clone(), None if fb is None else fb.clone()))
    prec = [p["precision"] if precision is None else precision for p in probs]
    views = []
    for p, (fw, fb, _, _) in zip(probs, outs):
        x = L.View(bufs[p["x"][0]], p["x"][1], p["Cin"])
        dy = L.View(bufs[p["dy"][0]], p["dy"][1], p["Cout"] // 4 if p["dy_mode"] == 1 else p["Cout"])
        dw = fw[G:G + p["Cout"] * p["Cin"] * 9].view(p["Cout"], p["Cin"], 3, 3)
        db = fb[G:G + p["Cout"]] if fb is not None else None
        views.append((x, dy, dw, db))
    pp = [dict(p, precision=pr) for p, pr in zip(probs, prec)]
    if case["op"] == "wgrad_batched":
        names = [_wgrad_kernel_name_of(pp, case["bufs"])]
    else:
        names = [_wgrad_kernel_name_of([p], case["bufs"]) for p in pp]
    if precision is None:
        assert names == case["kernel"], f"dispatch changed: {names} != {case['kernel']}"
    torch.cuda.synchronize()
    L.poison_lds()
    if case["op"] == "wgrad_batched":
        p0 = probs[0]
        L.conv3x3_wgrad_batched([dict(x=x, dy=dy, dw=dw, db=db, Cin=p["Cin"], Cout=p["Cout"], scale=p["scale"],
                                      accumulate=bool(p["accumulate"]), in_slope=p["in_slope"]) for p, (x, dy, dw, db) in zip(probs, views)],
                                N=p0["N"], H=p0["H"], W=p0["W"], OH=p0["OH"], OW=p0["OW"], stride=p0["stride"], dy_mode=p0["dy_mode"],
                                precision=prec[0])
    else:
        L.conv3x3_wgrad_seq([(x, dy, dw, db, dict(N=p["N"], H=p["H"], W=p["W"], OH=p["OH"], OW=p["OW"], Cin=p["Cin"], Cout=p["Cout"],
                                                  stride=p["stride"], dy_mode=p["dy_mode"], scale=p["scale"],
                                                  accumulate=bool(p["accumulate"]), in_slope=p["in_slope"], precision=pr))
                             for p, (x, dy, dw, db), pr in zip(probs, views, prec)])
    torch.cuda.synchronize()
    for b, (buf, ini) in enumerate(zip(bufs, init)):
        assert _bits_equal(buf, ini), f"buffer {b}: a weight gradient wrote into its input"
    worst = {}
    cpu = [ini.cpu() for ini in init]
    for k, (p, (fw, fb, fw0, fb0)) in enumerate(zip(probs, outs)):
        nw = p["Cout"] * p["Cin"] * 9
        assert _bits_equal(fw[:G], fw0[:G]) and _bits_equal(fw[G + nw:], fw0[G + nw:]), "dW written out of bounds"
        if fb is not None:
            assert _bits_equal(fb[:G], fb0[:G]) and _bits_equal(fb[G + p["Cout"]:], fb0[G + p["Cout"]:]), "db written out of bounds"
        x = cpu[p["x"][0]][..., p["x"][1]:p["x"][1] + p["Cin"]]
        cdy = p["Cout"] // 4 if p["dy_mode"] == 1 else p["Cout"]
        dy = cpu[p["dy"][0]][..., p["dy"][1]:p["dy"][1] + cdy]
        dw_ref, Aw, db_ref, Ab = f64ref.wgrad(x, dy, Cout=p["Cout"], stride=p["stride"], dy_mode=p["dy_mode"], in_slope=p["in_slope"],
                                              scale=p["scale"], accumulate=bool(p["accumulate"]),
                                              dw0=fw0[G:G + nw].view(p["Cout"], p["Cin"], 3, 3).cpu(),
                                              db0=None if fb0 is None else fb0[G:G + p["Cout"]].cpu(), want_db=fb is not None)
        fam = f64ref.family(names[0] if len(names) == 1 else names[k])
        t = f64ref.TAU[fam] if tau is None else tau
        what = f"{names} problem {k} (Cin={p['Cin']} Cout={p['Cout']} N={p['N']} {p['OH']}x{p['OW']})"
        r = f64ref.check(fw[G:G + nw].view(p["Cout"], p["Cin"], 3, 3), dw_ref, Aw, t, what=what + " dW")
        if fb is not None:
            r = max(r, f64ref.check(fb[G:G + p["Cout"]], db_ref, Ab, t, what=what + " db"))
        worst[fam] = max(worst.get(fam, 0.0), r)
    return worst


def run_case(case, **kw):
    return run_conv_case(case, **kw) if case["op"] == "seq" else run_wgrad_case(case, **kw)


def case_id(c):
    if c["op"] == "seq":
        s = c["convs"][0]
        return f"{c['step']}-{c['kernel'][0]}-n{len(c['convs'])}-N{s['N']}-{s['Cin']}to{s['Cout']}-{s['OH']}x{s['OW']}"
    p = c["probs"][0]
    return f"{c['step']}-{c['kernel'][0]}-n{len(c['probs'])}-N{p['N']}-{p['Cin']}to{p['Cout']}-{p['OH']}x{p['OW']}"


# Distinct launches of one configs[2] ('c2') and one configs[1] ('c1') fp32 step, recorded with record_step + dedup on an MI355X:
# (op, step, launches of that signature in the step, buffers [N, H, W, ldc] numbered per call, kernel names, one row per conv / problem).
# Views are [buffer, coff].  'c2+acc' is the configs[2] five-problem weight-gradient batch with accumulate = 1 (gradient accumulation;
# the step itself overwrites).
CONV_FIELDS = ("N", "H", "W", "OH", "OW", "Cin", "Cout", "stride", "in_mode", "ps_out", "wp_format", "alpha", "beta1", "beta2", "slope",
               "mask_slope", "in_slope", "bias", "x", "y", "r1", "r2", "mask")
WGRAD_FIELDS = ("N", "H", "W", "OH", "OW", "Cin", "Cout", "stride", "dy_mode", "in_slope", "scale", "accumulate", "precision", "db", "x",
                "dy")
_TABLE = [
    ('seq', 'c2', 1, [[32, 64, 64, 1], [32, 64, 64, 320]], ['conv3x3_cin_small_kernel<1>'], [
        [32, 64, 64, 64, 64, 1, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c2', 46, [[32, 64, 64, 320], [32, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 64], None, None, None],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 128], None, None, None],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 192], None, None, None],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 256], None, None, None],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 0.20000000298023224, 1.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [0, 0], None, None],
    ]),
    ('seq', 'c2', 22, [[32, 64, 64, 320], [32, 64, 64, 320], [32, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 64], None, None, None],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 128], None, None, None],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 192], None, None, None],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 256], None, None, None],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 0.03999999910593033, 0.20000000298023224, 1.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [0, 0], [2, 0], None],
    ]),
    ('seq', 'c2', 1, [[32, 64, 64, 320], [32, 64, 64, 64], [32, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 64], None, None, None],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 128], None, None, None],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 192], None, None, None],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 256], None, None, None],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 0.03999999910593033, 0.20000000298023224, 1.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [0, 0], [2, 0], None],
    ]),
    ('seq', 'c2', 1, [[32, 64, 64, 64], [32, 64, 64, 64], [32, 64, 64, 320]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [2, 0], None, None],
    ]),
    ('seq', 'c2', 1, [[32, 64, 64, 64], [32, 128, 128, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 64, 64, 64, 64, 64, 256, 1, 0, 1, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c2', 1, [[32, 128, 128, 64], [32, 256, 256, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 128, 128, 128, 128, 64, 256, 1, 0, 1, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c2', 1, [[32, 256, 256, 64], [32, 256, 256, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 256, 256, 256, 256, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c2', 1, [[32, 256, 256, 64], [32, 256, 256, 1]], ['conv3x3_cout_small_kernel<1>'], [
        [32, 256, 256, 256, 256, 64, 1, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c2', 10, [[32, 256, 256, 1], [32, 256, 256, 16], [32, 128, 128, 16], [32, 128, 128, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 32, 32, 32], [32, 32, 32, 64], [32, 16, 16, 64], [32, 16, 16, 1]], ['conv3x3_cin_small_kernel<1>', 'conv3x3_f32_kernel<32, 2, 0, true, 1, false>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_kernel<32, 2, 0, true, 1, false>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_kernel<32, 2, 0, true, 1, false>', 'conv3x3_f32_lw_kernel<64, 0>', 'conv3x3_f32_kernel<32, 2, 0, true, 1, false>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>'], [
        [32, 256, 256, 256, 256, 1, 16, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
        [32, 256, 256, 128, 128, 16, 16, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [1, 0], [2, 0], None, None, None],
        [32, 128, 128, 128, 128, 16, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [2, 0], [3, 0], None, None, None],
        [32, 128, 128, 64, 64, 32, 32, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [3, 0], [4, 0], None, None, None],
        [32, 64, 64, 64, 64, 32, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [4, 0], [5, 0], None, None, None],
        [32, 64, 64, 32, 32, 32, 32, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [5, 0], [6, 0], None, None, None],
        [32, 32, 32, 32, 32, 32, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [6, 0], [7, 0], None, None, None],
        [32, 32, 32, 16, 16, 64, 64, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [7, 0], [8, 0], None, None, None],
        [32, 16, 16, 16, 16, 64, 1, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.20000000298023224, True, [8, 0], [9, 0], None, None, None],
    ]),
    ('seq', 'c2', 2, [[32, 16, 16, 1], [32, 16, 16, 64], [32, 16, 16, 64], [32, 32, 32, 64], [32, 32, 32, 64], [32, 32, 32, 32], [32, 32, 32, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 128, 128, 32], [32, 128, 128, 32], [32, 128, 128, 16], [32, 128, 128, 16], [32, 256, 256, 16], [32, 256, 256, 16], [32, 256, 256, 1]], ['conv3x3_f32_kernel<64, 1, 0, false, 2, false>', 'conv3x3_f32_wino42_kernel<0, 1>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_wino42_kernel<0, 1>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_wino42_kernel<0, 2>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_wino42_kernel<0, 2>', 'conv3x3_cout_small_kernel<1>'], [
        [32, 16, 16, 16, 16, 1, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
        [32, 16, 16, 16, 16, 64, 256, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [1, 0], [3, 0], None, None, [4, 0]],
        [32, 32, 32, 32, 32, 64, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [3, 0], [5, 0], None, None, [6, 0]],
        [32, 32, 32, 32, 32, 32, 128, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [5, 0], [7, 0], None, None, [8, 0]],
        [32, 64, 64, 64, 64, 32, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [7, 0], [9, 0], None, None, [10, 0]],
        [32, 64, 64, 64, 64, 32, 128, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [9, 0], [11, 0], None, None, [12, 0]],
        [32, 128, 128, 128, 128, 32, 16, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [11, 0], [13, 0], None, None, [14, 0]],
        [32, 128, 128, 128, 128, 16, 64, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [13, 0], [15, 0], None, None, [16, 0]],
        [32, 256, 256, 256, 256, 16, 1, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [15, 0], [17, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 1, [[32, 256, 256, 64], [32, 256, 256, 1]], ['wgrad_f32_kernel<1, 0, false, 2>+reduce'], [
        [32, 256, 256, 256, 256, 64, 1, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 1, [[32, 256, 256, 1], [32, 256, 256, 64], [32, 256, 256, 64]], ['conv3x3_cin_small_kernel<1>'], [
        [32, 256, 256, 256, 256, 1, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('wgrad_seq', 'c2', 1, [[32, 256, 256, 64], [32, 256, 256, 64]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [32, 256, 256, 256, 256, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 1, [[32, 256, 256, 64], [32, 256, 256, 64], [32, 256, 256, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 256, 256, 256, 256, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('wgrad_seq', 'c2', 1, [[32, 128, 128, 64], [32, 256, 256, 64]], ['wgrad_f32_wino24_kernel<1>+reduce'], [
        [32, 128, 128, 128, 128, 64, 256, 1, 1, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 1, [[32, 256, 256, 64], [32, 128, 128, 64], [32, 128, 128, 64]], ['conv3x3_f32_wino42_kernel<1, 2>'], [
        [32, 128, 128, 128, 128, 256, 64, 1, 1, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('wgrad_seq', 'c2', 1, [[32, 64, 64, 64], [32, 128, 128, 64]], ['wgrad_f32_wino24_kernel<1>+reduce'], [
        [32, 64, 64, 64, 64, 64, 256, 1, 1, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 1, [[32, 128, 128, 64], [32, 64, 64, 64]], ['conv3x3_f32_wino42_kernel<1, 2>'], [
        [32, 64, 64, 64, 64, 256, 64, 1, 1, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 1, [[32, 64, 64, 64], [32, 64, 64, 64]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 1, [[32, 64, 64, 64], [32, 64, 64, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c2', 23, [[32, 64, 64, 320], [32, 64, 64, 320], [32, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 0.20000000298023224, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], None, None],
    ]),
    ('wgrad_batched', 'c2', 23, [[32, 64, 64, 320], [32, 64, 64, 320]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 256]],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 192]],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 128]],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 64]],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 1.0, 0.03999999910593033, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('wgrad_batched', 'c2+acc', 0, [[32, 64, 64, 320], [32, 64, 64, 320]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 1.0, 1.0, 1, 0, True, [0, 0], [1, 256]],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 1.0, 1.0, 1, 0, True, [0, 0], [1, 192]],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 1.0, 1.0, 1, 0, True, [0, 0], [1, 128]],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 1.0, 1.0, 1, 0, True, [0, 0], [1, 64]],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 1.0, 0.03999999910593033, 1, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 23, [[32, 64, 64, 320], [32, 64, 64, 320], [32, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], None, None],
    ]),
    ('wgrad_batched', 'c2', 46, [[32, 64, 64, 320], [32, 64, 64, 320]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 256]],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 192]],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 128]],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 64]],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 1.0, 0.20000000298023224, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 22, [[32, 64, 64, 320], [32, 64, 64, 320], [32, 64, 64, 320], [32, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], [3, 0], None],
    ]),
    ('seq', 'c2', 1, [[32, 64, 64, 320], [32, 64, 64, 320], [32, 64, 64, 64], [32, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<2>'], [
        [32, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [32, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [32, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [32, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [32, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], [3, 0], None],
    ]),
    ('wgrad_seq', 'c2', 1, [[32, 64, 64, 1], [32, 64, 64, 64]], ['wgrad_c1_kernel<1>+reduce'], [
        [32, 64, 64, 64, 64, 1, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 16, 16, 1], [32, 16, 16, 64], [32, 16, 16, 64]], ['conv3x3_f32_kernel<64, 1, 0, false, 2, false>'], [
        [32, 16, 16, 16, 16, 1, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 16, 16, 64], [32, 32, 32, 64], [32, 32, 32, 64]], ['conv3x3_f32_wino42_kernel<0, 1>'], [
        [32, 16, 16, 16, 16, 64, 256, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 32, 32, 64], [32, 32, 32, 32], [32, 32, 32, 32]], ['conv3x3_f32_kernel<32, 1, 0, true, 2, false>'], [
        [32, 32, 32, 32, 32, 64, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 32, 32, 32], [32, 64, 64, 32], [32, 64, 64, 32]], ['conv3x3_f32_wino42_kernel<0, 1>'], [
        [32, 32, 32, 32, 32, 32, 128, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 64, 64, 32], [32, 64, 64, 32], [32, 64, 64, 32]], ['conv3x3_f32_kernel<32, 1, 0, true, 2, false>'], [
        [32, 64, 64, 64, 64, 32, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 64, 64, 32], [32, 128, 128, 32], [32, 128, 128, 32]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 64, 64, 64, 64, 32, 128, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 128, 128, 32], [32, 128, 128, 16], [32, 128, 128, 16]], ['conv3x3_f32_kernel<32, 1, 0, true, 2, false>'], [
        [32, 128, 128, 128, 128, 32, 16, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 128, 128, 16], [32, 256, 256, 16], [32, 256, 256, 16]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 128, 128, 128, 128, 16, 64, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 256, 256, 16], [32, 256, 256, 1]], ['conv3x3_cout_small_kernel<1>'], [
        [32, 256, 256, 256, 256, 16, 1, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c2', 4, [[32, 16, 16, 1], [32, 16, 16, 64], [32, 16, 16, 64], [32, 32, 32, 64], [32, 32, 32, 64], [32, 32, 32, 32], [32, 32, 32, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 128, 128, 32], [32, 128, 128, 32], [32, 128, 128, 16], [32, 128, 128, 16], [32, 256, 256, 16], [32, 256, 256, 16]], ['conv3x3_f32_kernel<64, 1, 0, false, 2, false>', 'conv3x3_f32_wino42_kernel<0, 1>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_wino42_kernel<0, 1>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_wino42_kernel<0, 2>', 'conv3x3_f32_kernel<32, 1, 0, true, 2, false>', 'conv3x3_f32_wino42_kernel<0, 2>'], [
        [32, 16, 16, 16, 16, 1, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
        [32, 16, 16, 16, 16, 64, 256, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [1, 0], [3, 0], None, None, [4, 0]],
        [32, 32, 32, 32, 32, 64, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [3, 0], [5, 0], None, None, [6, 0]],
        [32, 32, 32, 32, 32, 32, 128, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [5, 0], [7, 0], None, None, [8, 0]],
        [32, 64, 64, 64, 64, 32, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [7, 0], [9, 0], None, None, [10, 0]],
        [32, 64, 64, 64, 64, 32, 128, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [9, 0], [11, 0], None, None, [12, 0]],
        [32, 128, 128, 128, 128, 32, 16, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [11, 0], [13, 0], None, None, [14, 0]],
        [32, 128, 128, 128, 128, 16, 64, 1, 0, 1, 6, 1.0, 0.0, 0.0, 1.0, 0.20000000298023224, 1.0, False, [13, 0], [15, 0], None, None, [16, 0]],
    ]),
    ('wgrad_seq', 'c2', 4, [[32, 256, 256, 1], [32, 256, 256, 16], [32, 256, 256, 16], [32, 128, 128, 16], [32, 128, 128, 16], [32, 128, 128, 32], [32, 128, 128, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 64, 64, 32], [32, 32, 32, 32], [32, 32, 32, 32], [32, 32, 32, 64], [32, 32, 32, 64], [32, 16, 16, 64], [32, 16, 16, 64], [32, 16, 16, 1]], ['wgrad_c1_kernel<1>+reduce', 'wgrad_f32_kernel<2, 0, true, 4>+reduce', 'wgrad_f32_kernel<1, 0, true, 4>+reduce', 'wgrad_f32_kernel<2, 0, true, 4>+reduce', 'wgrad_f32_kernel<1, 0, true, 4>+reduce', 'wgrad_f32_kernel<2, 0, true, 4>+reduce', 'wgrad_f32_kernel<1, 0, true, 2>+reduce', 'wgrad_f32_kernel<2, 0, true, 1>+reduce', 'wgrad_f32_kernel<1, 0, false, 2>+reduce'], [
        [32, 256, 256, 256, 256, 1, 16, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
        [32, 256, 256, 128, 128, 16, 16, 2, 0, 0.20000000298023224, 1.0, 0, 0, True, [2, 0], [3, 0]],
        [32, 128, 128, 128, 128, 16, 32, 1, 0, 0.20000000298023224, 1.0, 0, 0, True, [4, 0], [5, 0]],
        [32, 128, 128, 64, 64, 32, 32, 2, 0, 0.20000000298023224, 1.0, 0, 0, True, [6, 0], [7, 0]],
        [32, 64, 64, 64, 64, 32, 32, 1, 0, 0.20000000298023224, 1.0, 0, 0, True, [8, 0], [9, 0]],
        [32, 64, 64, 32, 32, 32, 32, 2, 0, 0.20000000298023224, 1.0, 0, 0, True, [10, 0], [11, 0]],
        [32, 32, 32, 32, 32, 32, 64, 1, 0, 0.20000000298023224, 1.0, 0, 0, True, [12, 0], [13, 0]],
        [32, 32, 32, 16, 16, 64, 64, 2, 0, 0.20000000298023224, 1.0, 0, 0, True, [14, 0], [15, 0]],
        [32, 16, 16, 16, 16, 64, 1, 1, 0, 0.20000000298023224, 1.0, 0, 0, True, [16, 0], [17, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 256, 256, 1], [32, 256, 256, 16]], ['conv3x3_cin_small_kernel<1>'], [
        [32, 256, 256, 256, 256, 1, 16, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 256, 256, 1], [32, 256, 256, 16]], ['wgrad_c1_kernel<1>+reduce'], [
        [32, 256, 256, 256, 256, 1, 16, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 256, 256, 16], [32, 128, 128, 16]], ['conv3x3_f32_kernel<32, 2, 0, true, 1, false>'], [
        [32, 256, 256, 128, 128, 16, 16, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 256, 256, 16], [32, 128, 128, 16]], ['wgrad_f32_kernel<2, 0, true, 4>+reduce'], [
        [32, 256, 256, 128, 128, 16, 16, 2, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 128, 128, 16], [32, 128, 128, 32]], ['conv3x3_f32_kernel<32, 1, 0, true, 2, false>'], [
        [32, 128, 128, 128, 128, 16, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 128, 128, 16], [32, 128, 128, 32]], ['wgrad_f32_kernel<1, 0, true, 4>+reduce'], [
        [32, 128, 128, 128, 128, 16, 32, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 128, 128, 32], [32, 64, 64, 32]], ['conv3x3_f32_kernel<32, 2, 0, true, 1, false>'], [
        [32, 128, 128, 64, 64, 32, 32, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 128, 128, 32], [32, 64, 64, 32]], ['wgrad_f32_kernel<2, 0, true, 4>+reduce'], [
        [32, 128, 128, 64, 64, 32, 32, 2, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 64, 64, 32], [32, 64, 64, 32]], ['conv3x3_f32_kernel<32, 1, 0, true, 2, false>'], [
        [32, 64, 64, 64, 64, 32, 32, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 64, 64, 32], [32, 64, 64, 32]], ['wgrad_f32_kernel<1, 0, true, 4>+reduce'], [
        [32, 64, 64, 64, 64, 32, 32, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 64, 64, 32], [32, 32, 32, 32]], ['conv3x3_f32_kernel<32, 2, 0, true, 1, false>'], [
        [32, 64, 64, 32, 32, 32, 32, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 64, 64, 32], [32, 32, 32, 32]], ['wgrad_f32_kernel<2, 0, true, 4>+reduce'], [
        [32, 64, 64, 32, 32, 32, 32, 2, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 32, 32, 32], [32, 32, 32, 64]], ['conv3x3_f32_lw_kernel<64, 0>'], [
        [32, 32, 32, 32, 32, 32, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 32, 32, 32], [32, 32, 32, 64]], ['wgrad_f32_kernel<1, 0, true, 2>+reduce'], [
        [32, 32, 32, 32, 32, 32, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c2', 2, [[32, 32, 32, 64], [32, 16, 16, 64]], ['conv3x3_f32_kernel<32, 2, 0, true, 1, false>'], [
        [32, 32, 32, 16, 16, 64, 64, 2, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 32, 32, 64], [32, 16, 16, 64]], ['wgrad_f32_kernel<2, 0, true, 1>+reduce'], [
        [32, 32, 32, 16, 16, 64, 64, 2, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('wgrad_seq', 'c2', 2, [[32, 16, 16, 64], [32, 16, 16, 1]], ['wgrad_f32_kernel<1, 0, false, 2>+reduce'], [
        [32, 16, 16, 16, 16, 64, 1, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 1, [[16, 64, 64, 1], [16, 64, 64, 320]], ['conv3x3_f32_kernel<64, 1, 0, false, 2, false>'], [
        [16, 64, 64, 64, 64, 1, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c1', 46, [[16, 64, 64, 320], [16, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 64], None, None, None],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 128], None, None, None],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 192], None, None, None],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 256], None, None, None],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 0.20000000298023224, 1.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [0, 0], None, None],
    ]),
    ('seq', 'c1', 22, [[16, 64, 64, 320], [16, 64, 64, 320], [16, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 64], None, None, None],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 128], None, None, None],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 192], None, None, None],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 256], None, None, None],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 0.03999999910593033, 0.20000000298023224, 1.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [0, 0], [2, 0], None],
    ]),
    ('seq', 'c1', 1, [[16, 64, 64, 320], [16, 64, 64, 64], [16, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 64], None, None, None],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 128], None, None, None],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 192], None, None, None],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [0, 256], None, None, None],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 0.03999999910593033, 0.20000000298023224, 1.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [0, 0], [2, 0], None],
    ]),
    ('seq', 'c1', 1, [[16, 64, 64, 64], [16, 64, 64, 64], [16, 64, 64, 320]], ['conv3x3_f32_wino42_kernel<0, 1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], [2, 0], None, None],
    ]),
    ('seq', 'c1', 1, [[16, 64, 64, 64], [16, 128, 128, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [16, 64, 64, 64, 64, 64, 256, 1, 0, 1, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c1', 1, [[16, 128, 128, 64], [16, 256, 256, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [16, 128, 128, 128, 128, 64, 256, 1, 0, 1, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c1', 1, [[16, 256, 256, 64], [16, 256, 256, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [16, 256, 256, 256, 256, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 0.009999999776482582, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c1', 1, [[16, 256, 256, 64], [16, 256, 256, 1]], ['conv3x3_cout_small_kernel<1>'], [
        [16, 256, 256, 256, 256, 64, 1, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, True, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c1', 1, [[16, 256, 256, 64], [16, 256, 256, 1]], ['wgrad_f32_kernel<1, 0, false, 2>+reduce'], [
        [16, 256, 256, 256, 256, 64, 1, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 1, [[16, 256, 256, 1], [16, 256, 256, 64], [16, 256, 256, 64]], ['conv3x3_cin_small_kernel<1>'], [
        [16, 256, 256, 256, 256, 1, 64, 1, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('wgrad_seq', 'c1', 1, [[16, 256, 256, 64], [16, 256, 256, 64]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [16, 256, 256, 256, 256, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 1, [[16, 256, 256, 64], [16, 256, 256, 64], [16, 256, 256, 64]], ['conv3x3_f32_wino42_kernel<0, 2>'], [
        [16, 256, 256, 256, 256, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('wgrad_seq', 'c1', 1, [[16, 128, 128, 64], [16, 256, 256, 64]], ['wgrad_f32_wino24_kernel<1>+reduce'], [
        [16, 128, 128, 128, 128, 64, 256, 1, 1, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 1, [[16, 256, 256, 64], [16, 128, 128, 64], [16, 128, 128, 64]], ['conv3x3_f32_wino42_kernel<1, 2>'], [
        [16, 128, 128, 128, 128, 256, 64, 1, 1, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [1, 0], None, None, [2, 0]],
    ]),
    ('wgrad_seq', 'c1', 1, [[16, 64, 64, 64], [16, 128, 128, 64]], ['wgrad_f32_wino24_kernel<1>+reduce'], [
        [16, 64, 64, 64, 64, 64, 256, 1, 1, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 1, [[16, 128, 128, 64], [16, 64, 64, 64]], ['conv3x3_f32_wino42_kernel<1, 1>'], [
        [16, 64, 64, 64, 64, 256, 64, 1, 1, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('wgrad_seq', 'c1', 1, [[16, 64, 64, 64], [16, 64, 64, 64]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 1, [[16, 64, 64, 64], [16, 64, 64, 64]], ['conv3x3_f32_wino42_kernel<0, 1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [1, 0], None, None, None],
    ]),
    ('seq', 'c1', 23, [[16, 64, 64, 320], [16, 64, 64, 320], [16, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 0.20000000298023224, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], None, None],
    ]),
    ('wgrad_batched', 'c1', 23, [[16, 64, 64, 320], [16, 64, 64, 320]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 256]],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 192]],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 128]],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 64]],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 1.0, 0.03999999910593033, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 23, [[16, 64, 64, 320], [16, 64, 64, 320], [16, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], None, None],
    ]),
    ('wgrad_batched', 'c1', 46, [[16, 64, 64, 320], [16, 64, 64, 320]], ['wgrad_f32_wino24_kernel<0>+reduce'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 256]],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 192]],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 128]],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 64]],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 1.0, 0.20000000298023224, 0, 0, True, [0, 0], [1, 0]],
    ]),
    ('seq', 'c1', 22, [[16, 64, 64, 320], [16, 64, 64, 320], [16, 64, 64, 320], [16, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], [3, 0], None],
    ]),
    ('seq', 'c1', 1, [[16, 64, 64, 320], [16, 64, 64, 320], [16, 64, 64, 64], [16, 64, 64, 320]], ['conv3x3_f32_wino42_chain_kernel<1>'], [
        [16, 64, 64, 64, 64, 64, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 64], None, None, [1, 256]],
        [16, 64, 64, 64, 64, 128, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 128], None, None, [1, 192]],
        [16, 64, 64, 64, 64, 192, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 192], None, None, [1, 128]],
        [16, 64, 64, 64, 64, 256, 64, 1, 0, 0, 6, 1.0, 0.0, 0.0, 1.0, 0.009999999776482582, 1.0, False, [0, 0], [0, 256], None, None, [1, 64]],
        [16, 64, 64, 64, 64, 320, 64, 1, 0, 0, 6, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, False, [0, 0], [2, 0], [0, 0], [3, 0], None],
    ]),
    ('wgrad_seq', 'c1', 1, [[16, 64, 64, 1], [16, 64, 64, 64]], ['wgrad_c1_kernel<1>+reduce'], [
        [16, 64, 64, 64, 64, 1, 64, 1, 0, 1.0, 1.0, 0, 0, True, [0, 0], [1, 0]],
    ]),
]


def _expand(op, step, count, bufs, kernel, rows):
    fields = CONV_FIELDS if op == "seq" else WGRAD_FIELDS
    rows = [{k: v for k, v in zip(fields, r) if v is not None} for r in rows]
    return dict(op=op, step=step, count=count, bufs=bufs, kernel=kernel, **({"convs": rows} if op == "seq" else {"probs": rows}))


CASES = [_expand(*c) for c in _TABLE]


# ------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_launch_vs_float64(case):
    run_case(case)


def test_launch_set_is_covered():
    """every kernel the configs[2] and configs[1] fp32 steps launch (names as L.KernelTimer reports them) has a case above"""
    covered = {n for c in CASES for n in c["kernel"]}
    ran = set()
    for tag in STEPS:
        names = set()
        rec = record_step(tag, names)
        assert {n for c in rec for n in c["kernel"]} == names, "the recorder and L.KernelTimer disagree on what the step launched"
        ran |= names
    missing = sorted(ran - covered)
    assert not missing, f"launched by the fp32 steps without a float64 parity case: {missing}"

