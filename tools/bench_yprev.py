"""Kernel-level A/B of the previous-state layout of the GRU layer output (option gru_yprev) at the
bench shape, both layouts alternated in one process, HIP-event timed:
  fwd_drop / fwd_plain  tt_gru_fwd vs tt_gru_fwd_yprev (with the dropout copy: layer 0; without: layer 1)
  bwd                   tt_gru_bwd vs tt_gru_bwd_yprev (gru_bwd_rows)
  wgrad_hh              dW_hh with its split-K reduction: the time-shifted TN GEMM on Y vs the plain one
                        on Yp (M 3H, N H, K B*T, 4 problems, random operands)
One JSON line per kernel: median, min, max and spread (max - min) per arm over --alternations
timings of --iters calls each, and whether the new arm won every alternation."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_gru  # noqa: E402
from two_towers_amd import _lib, ops  # noqa: E402
from two_towers_amd._lib import call, stream_ptr  # noqa: E402


def timed(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def ab(name, arms, a, extra=None):
    for f in arms.values():
        f()  # warm-up: code objects, occupancy queries, allocator
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.alternations):
        for k, f in arms.items():
            ms[k].append(timed(f, a.iters))
    out = {"kernel": name, "B": a.B, "T": a.T, "H": a.H, "iters": a.iters, "alternations": a.alternations}
    for k, v in ms.items():
        out[k] = {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "spread_ms": round(max(v) - min(v), 4), "all_ms": [round(x, 4) for x in v]}
    out["yprev_faster_every_time"] = all(y < x for x, y in zip(ms["default"], ms["yprev"]))
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated subset of fwd_drop,fwd_plain,bwd,wgrad_hh")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    dev = torch.device("cuda")
    B, T, H, dt = a.B, a.T, a.H, torch.bfloat16
    lib = _lib.load()
    assert lib.tt_gru_yprev_supported(1, 4, B, T, H, 6 * H, 2 * H) == 1, "the previous-state layout does not apply"
    st = stream_ptr(dev)
    recs, keep = bench_gru.setup(B, T, H, dev)
    G, whh, bhn, Y, X1, S, hs = keep
    nb = lib.tt_gru_fwd_ws_size(1, 4, B, T, H, 6 * H, 2 * H)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    F = [torch.empty(B, 2 * H, device=dev, dtype=dt) for _ in range(2)]
    fin = (ctypes.c_void_p * 4)(*[F[ti][:, d * H:].data_ptr() for ti in range(2) for d in range(2)])

    def fwd(yprev, drop):
        for i in range(4):
            ti, d = i // 2, i % 2
            recs[i].x1 = X1[ti][:, d * H:].data_ptr() if drop else None
        if yprev:
            call("tt_gru_fwd_yprev", 1, recs, fin, 4, B, T, H, 6 * H, 2 * H, 2 * H, 0.1 if drop else 0.0, ws.data_ptr(),
                 ws.numel(), st)
        else:
            call("tt_gru_fwd", 1, recs, 4, B, T, H, 6 * H, 2 * H, 0.1 if drop else 0.0, ws.data_ptr(), ws.numel(), st)

    for drop in (True, False):
        name = "fwd_drop" if drop else "fwd_plain"
        if not only or name in only:
            ab(name, {"default": lambda: fwd(0, drop), "yprev": lambda: fwd(1, drop)}, a,
               {"xc_status": int(ws[:4].view(torch.int32).item())})
    # the backward and dW_hh read real S and both layouts of a real Y
    fwd(1, True)
    Yp = [y.clone() for y in Y]
    fwd(0, True)
    torch.cuda.synchronize()
    brecs, bkeep = bench_gru.setup_bwd(B, T, H, keep, dev)
    dG = bkeep[2]

    def bwd(yprev):
        for i in range(4):
            ti, d = i // 2, i % 2
            brecs[i].y = (Yp if yprev else Y)[ti][:, d * H:].data_ptr()
        call("tt_gru_bwd_yprev" if yprev else "tt_gru_bwd", 1, brecs, 4, B, T, H, 2 * H, 8 * H, 2 * H, st)

    if not only or "bwd" in only:
        ab("bwd", {"default": lambda: bwd(0), "yprev": lambda: bwd(1)}, a)
    if not only or "wgrad_hh" in only:
        for ti in range(2):  # random operands (the BPTT's own dG is far from uniform), Yp the shifted Y
            dG[ti].copy_(torch.randn(dG[ti].shape, device=dev).to(dt))
            Y[ti].copy_(torch.randn(Y[ti].shape, device=dev).to(dt))
            y, yp = Y[ti].view(B, T, 2 * H), Yp[ti].view(B, T, 2 * H)
            yp.zero_()
            yp[:, 1:, :H] = y[:, :-1, :H]
            yp[:, :-1, H:] = y[:, 1:, H:]
        a_hh = [dG[ti][:, d * 3 * H:] for ti in range(2) for d in range(2)]
        a_hi = [dG[ti][:, 6 * H + d * H:] for ti in range(2) for d in range(2)]
        c_hh = [torch.empty(3 * H, H, device=dev) for _ in range(4)]
        splits = ops.gemm_splits(3 * H, H, B * T, 4, dt)

        def wgrad(yprev):
            b_hh = [(Yp if yprev else Y)[ti][:, d * H:] for ti in range(2) for d in range(2)]
            kw = {} if yprev else dict(bshift=[-1, 1, -1, 1], seq_t=T)
            ops.gemm(a_hh, b_hh, c_hh, m=3 * H, n=H, k=B * T, lda=8 * H, ldb=2 * H, ldc=H, a_kouter=True, b_kouter=True,
                     dtype=dt, out_dtype=torch.float32, a_hi=a_hi, a_split=2 * H, **kw)

        flop = 2.0 * 3 * H * H * B * T * 4
        ab("wgrad_hh", {"default": lambda: wgrad(0), "yprev": lambda: wgrad(1)}, a, {"splits": splits, "tflop": flop / 1e12})


if __name__ == "__main__":
    main()
