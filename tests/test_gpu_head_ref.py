"""The projection heads, called directly (tt_proj_head_fwd / _bwd, tt_proj_head1_fwd / _bwd),
against torch double with autograd.

  enhanced head: Linear(4h -> 2h) -> LayerNorm(2h) -> ReLU -> Linear(2h -> h)
  margin head:   Linear(2C -> C)  -> LayerNorm(C)  -> ReLU -> dropout_mask(seed, row, col)

The reference runs on the dt-rounded weights and inputs. In bf16 its later stages start from
the kernel's own stored p1 and u (substituted in value, gradients still flow through), so each
stage is judged alone: p1 against the exact Linear, LayerNorm + ReLU against the stored p1, the
last Linear against the stored u; the backward is the gradient at those stored points.

Shapes: LayerNorm widths of 16 and 8 columns (under one wave), 80 and 200 (no multiple of 64)
and 1024 (the limit of 16 columns per lane; one 8-column step above it is TT_EINVAL); 1, 17 and
130 rows (one row; one full 16-row partial block of the backward plus one row; tails of the
4-rows-per-workgroup forward). The backward scratch is filled with 1e30 and followed by a
guard that must survive, so the size functions are checked to be sufficient.

Tolerances: fp32 1e-4, bf16 2e-2; per row (oracle.gru_ref.row_err) for row-shaped outputs,
relative to the largest reference entry for weight and bias gradients. mean is measured
against the largest |p1| of its row (the scale of what it averages: a mean near zero has no
scale of its own), rstd against itself.
Largest errors measured on an MI355X:
  enhanced head   fp32 2.7e-6 (u, h 512)    bf16 4.5e-3 (dx, h 8)
  margin head     fp32 2.9e-6 (p1, C 1024)  bf16 8.5e-3 (dx, C 8, 130 rows)
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cpu_ref import dropout_mask  # noqa: E402
from oracle.gru_ref import dropout_err, row_err, vec_err  # noqa: E402
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import Head1BwdIO, Head1FwdIO, HeadBwdIO, HeadFwdIO, call, stream_ptr  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 1e-4, BF16: 2e-2}
EPS = 1e-5
GUARD = 256


def _dev(t):
    return t.to(DEV).contiguous()


def _ste(ref, stored):
    """ref's gradient path with stored's values (stored None: ref itself)."""
    return ref if stored is None else ref + (stored.double() - ref).detach()


def _ln_relu(p1, g, beta):
    mean = p1.mean(1, keepdim=True)
    rstd = ((p1 - mean).pow(2).mean(1, keepdim=True) + EPS).rsqrt()
    return mean, rstd, torch.relu((p1 - mean) * rstd * g + beta)


def _scratch(nbytes):
    """nbytes of 1e30 followed by a guard."""
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    ws[:nbytes // 4 * 4].view(torch.float32).fill_(1e30)
    ws[nbytes:] = 0xA5
    return ws


def _report(what, errs, tol):
    worst = max(errs, key=lambda e: e[1])
    print(f"{what}: worst error {worst[1]:.3g} ({worst[0]} at {worst[2]})")
    for name, e, idx in errs:
        assert e <= tol, f"{what}: {name} error {e:.3g} > {tol:g} at {idx}"


def _mean_err(got, ref, p1):
    scale = p1.detach().double().abs().amax(1)
    e = torch.nan_to_num((got.double().cpu() - ref.detach().reshape(-1)).abs() / scale, nan=float("inf"))
    k = int(e.argmax())
    return float(e[k]), (k,)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B", [1, 17, 130])
@pytest.mark.parametrize("h,ntower", [(8, 2), (40, 1), (512, 2)])
def test_enhanced_head_matches_float64(h, ntower, B, dt):
    lib = _lib.load()
    dtc = _lib.dtype_code(dt)
    C = 2 * h
    g = torch.Generator().manual_seed(100 * h + B)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    tw = []
    for _ in range(ntower):
        t = dict(x=rnd(B, 4 * h).to(dt), w1=(rnd(C, 4 * h) * (4 * h) ** -0.5).to(dt), b1=rnd(C) * 0.5,
                 g=1.0 + 0.3 * rnd(C), beta=0.3 * rnd(C), w2=(rnd(h, C) * C ** -0.5).to(dt), b2=rnd(h) * 0.5,
                 dout=rnd(B, h).to(dt).float())
        t["d"] = {k: _dev(v) for k, v in t.items()}
        t["o"] = dict(p1=torch.empty(B, C, dtype=dt, device=DEV), u=torch.empty(B, C, dtype=dt, device=DEV),
                      mean=torch.empty(B, device=DEV), rstd=torch.empty(B, device=DEV), out=torch.empty(B, h, device=DEV))
        tw.append(t)
    io = (HeadFwdIO * ntower)()
    for q, t in zip(io, tw):
        d, o = t["d"], t["o"]
        q.w1, q.b1, q.ln_g, q.ln_b, q.w2, q.b2 = (d[k].data_ptr() for k in ("w1", "b1", "g", "beta", "w2", "b2"))
        q.x, q.p1, q.mean, q.rstd, q.u, q.out = (d["x"].data_ptr(), o["p1"].data_ptr(), o["mean"].data_ptr(),
                                                  o["rstd"].data_ptr(), o["u"].data_ptr(), o["out"].data_ptr())
    call("tt_proj_head_fwd", dtc, io, ntower, B, h, EPS, stream_ptr())
    nws = lib.tt_proj_head_bwd_ws_size(dtc, B, h)
    assert nws > 0
    bio = (HeadBwdIO * ntower)()
    for q, t in zip(bio, tw):
        d, o = t["d"], t["o"]
        t["gr"] = dict(dx=torch.empty(B, 4 * h, device=DEV), dw1=torch.empty(C, 4 * h, device=DEV),
                       db1=torch.empty(C, device=DEV), dg=torch.empty(C, device=DEV), dbeta=torch.empty(C, device=DEV),
                       dw2=torch.empty(h, C, device=DEV), db2=torch.empty(h, device=DEV))
        t["ws"] = _scratch(nws)
        q.w1, q.ln_g, q.ln_b, q.w2, q.x = (d[k].data_ptr() for k in ("w1", "g", "beta", "w2", "x"))
        q.p1, q.mean, q.rstd, q.u = (o[k].data_ptr() for k in ("p1", "mean", "rstd", "u"))
        q.dout = d["dout"].data_ptr()
        for k, v in t["gr"].items():
            setattr(q, k, v.data_ptr())
        q.ws = t["ws"].data_ptr()
    call("tt_proj_head_bwd", dtc, bio, ntower, B, h, EPS, stream_ptr())
    torch.cuda.synchronize()
    errs = []
    for ti, t in enumerate(tw):
        o = {k: v.cpu() for k, v in t["o"].items()}
        gr = {k: v.cpu() for k, v in t["gr"].items()}
        assert bool((t["ws"][nws:] == 0xA5).all()), "tt_proj_head_bwd wrote past tt_proj_head_bwd_ws_size"
        L = {k: t[k].double().requires_grad_(True) for k in ("x", "w1", "b1", "g", "beta", "w2", "b2")}
        p1 = L["x"] @ L["w1"].t() + L["b1"]
        p1e = _ste(p1, o["p1"] if dt == BF16 else None)
        mean, rstd, u = _ln_relu(p1e, L["g"], L["beta"])
        out = _ste(u, o["u"] if dt == BF16 else None) @ L["w2"].t() + L["b2"]
        out.backward(t["dout"].double())
        tag = f"tower {ti} "
        errs += [(tag + "p1", *row_err(o["p1"], p1.detach().to(dt))), (tag + "u", *row_err(o["u"], u.detach().to(dt))),
                 (tag + "out", *row_err(o["out"], out)), (tag + "mean", *_mean_err(o["mean"], mean, p1e)),
                 (tag + "rstd", *row_err(o["rstd"].reshape(B, 1), rstd)), (tag + "dx", *row_err(gr["dx"], L["x"].grad))]
        for k, leaf in (("dw1", "w1"), ("db1", "b1"), ("dg", "g"), ("dbeta", "beta"), ("dw2", "w2"), ("db2", "b2")):
            errs.append((tag + k, *vec_err(gr[k], L[leaf].grad)))
    _report(f"enhanced head {dt} h {h} B {B} ntower {ntower}", errs, TOL[dt])


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", [1, 17, 130])
@pytest.mark.parametrize("C", [8, 200, 1024])
def test_margin_head_matches_float64(C, rows, p, dt):
    lib = _lib.load()
    dtc = _lib.dtype_code(dt)
    seed = 4242 + C
    g = torch.Generator().manual_seed(10 * C + rows)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(x=rnd(rows, 2 * C).to(dt), w1=(rnd(C, 2 * C) * (2 * C) ** -0.5).to(dt), b1=rnd(C) * 0.5,
             g=1.0 + 0.3 * rnd(C), beta=0.3 * rnd(C), dout=rnd(rows, C))
    d = {k: _dev(v) for k, v in t.items()}
    o = dict(p1=torch.empty(rows, C, dtype=dt, device=DEV), mean=torch.empty(rows, device=DEV),
             rstd=torch.empty(rows, device=DEV), out=torch.empty(rows, C, device=DEV))
    io = Head1FwdIO()
    io.x, io.w1, io.b1, io.ln_g, io.ln_b = (d[k].data_ptr() for k in ("x", "w1", "b1", "g", "beta"))
    io.p1, io.mean, io.rstd, io.out = (o[k].data_ptr() for k in ("p1", "mean", "rstd", "out"))
    call("tt_proj_head1_fwd", dtc, ctypes.byref(io), rows, C, EPS, p, seed, stream_ptr())
    nws = lib.tt_proj_head1_bwd_ws_size(dtc, rows, C)
    assert nws > 0
    ws = _scratch(nws)
    gr = dict(dx=torch.empty(rows, 2 * C, device=DEV), dw1=torch.empty(C, 2 * C, device=DEV),
              db1=torch.empty(C, device=DEV), dg=torch.empty(C, device=DEV), dbeta=torch.empty(C, device=DEV))
    bio = Head1BwdIO()
    bio.x, bio.w1, bio.ln_g, bio.ln_b = (d[k].data_ptr() for k in ("x", "w1", "g", "beta"))
    bio.p1, bio.mean, bio.rstd, bio.dout = o["p1"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), d["dout"].data_ptr()
    for k, v in gr.items():
        setattr(bio, k, v.data_ptr())
    bio.ws = ws.data_ptr()
    call("tt_proj_head1_bwd", dtc, ctypes.byref(bio), rows, C, p, seed, stream_ptr())
    torch.cuda.synchronize()
    assert bool((ws[nws:] == 0xA5).all()), "tt_proj_head1_bwd wrote past tt_proj_head1_bwd_ws_size"
    o = {k: v.cpu() for k, v in o.items()}
    gr = {k: v.cpu() for k, v in gr.items()}
    L = {k: t[k].double().requires_grad_(True) for k in ("x", "w1", "b1", "g", "beta")}
    p1 = L["x"] @ L["w1"].t() + L["b1"]
    p1e = _ste(p1, o["p1"] if dt == BF16 else None)
    mean, rstd, u = _ln_relu(p1e, L["g"], L["beta"])
    mult = torch.from_numpy(dropout_mask(seed, rows, C, p).astype(np.float64))
    out = u * mult
    out.backward(t["dout"].double())
    wrong, e_out = dropout_err(o["out"], u.detach(), mult)
    assert wrong == 0, f"out: {wrong} elements differ from the dropout mask's zero pattern"
    errs = [("p1", *row_err(o["p1"], p1.detach().to(dt))), ("out", *e_out), ("mean", *_mean_err(o["mean"], mean, p1e)),
            ("rstd", *row_err(o["rstd"].reshape(rows, 1), rstd)), ("dx", *row_err(gr["dx"], L["x"].grad))]
    for k, leaf in (("dw1", "w1"), ("db1", "b1"), ("dg", "g"), ("dbeta", "beta")):
        errs.append((k, *vec_err(gr[k], L[leaf].grad)))
    _report(f"margin head {dt} C {C} rows {rows} p {p}", errs, TOL[dt])


def test_heads_reject_more_than_16_columns_per_lane():
    """LayerNorm holds 16 columns per lane: C = 2h = 1040 and C = 1032 are TT_EINVAL in all four
    entry points, before anything is read or launched."""
    lib = _lib.load()
    st = stream_ptr()
    for dtc in (_lib.DT_F32, _lib.DT_BF16):
        assert lib.tt_proj_head_fwd(dtc, (HeadFwdIO * 1)(), 1, 4, 520, EPS, st) == _lib.TT_EINVAL
        assert lib.tt_proj_head_bwd(dtc, (HeadBwdIO * 1)(), 1, 4, 520, EPS, st) == _lib.TT_EINVAL
        assert lib.tt_proj_head1_fwd(dtc, ctypes.byref(Head1FwdIO()), 4, 1032, EPS, 0.0, 0, st) == _lib.TT_EINVAL
        assert lib.tt_proj_head1_bwd(dtc, ctypes.byref(Head1BwdIO()), 4, 1032, 0.0, 0, st) == _lib.TT_EINVAL
    torch.cuda.synchronize()
