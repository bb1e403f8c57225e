"""A/B: the fused symmetric InfoNCE (tt_infonce_sym_fwd + tt_infonce_sym_bwd) against the
two-call composition a user had before it (tt_infonce_fwd/_bwd on (q, d) and on (d, q), plus
the two gradient adds), forward + backward, through the C ABI in one process.

    python tools/bench_symloss.py [--n 8192] [--h 256] [--iters 50] [--out profiles/symloss_ab.json]

Device-event times per iteration, both variants interleaved in every round so clock and
neighbour drift hit both alike; reports min / median per variant and checks that the two
give the same loss and gradients.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import call, dtype_code  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--h", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inv-tau", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    dev, bf = "cuda", torch.bfloat16
    n, h, it = a.n, a.h, a.inv_tau
    g = torch.Generator().manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(n, h, generator=g), dim=1).to(dev, bf).contiguous()
    d = torch.nn.functional.normalize(torch.randn(n, h, generator=g), dim=1).to(dev, bf).contiguous()
    dc = dtype_code(bf)
    st = torch.cuda.current_stream().cuda_stream
    f32 = dict(dtype=torch.float32, device=dev)
    gs = torch.tensor([1.0 / n], **f32)
    lr, lc, row = (torch.empty(n, **f32) for _ in range(3))
    dq, dd = torch.empty(n, h, **f32), torch.empty(n, h, **f32)
    wsf = torch.empty(lib.tt_infonce_sym_fwd_ws_size(n, h), dtype=torch.uint8, device=dev)
    wsb = torch.empty(lib.tt_infonce_sym_bwd_ws_size(dc, n, h), dtype=torch.uint8, device=dev)

    def fused():
        call("tt_infonce_sym_fwd", dc, q.data_ptr(), d.data_ptr(), n, h, it, lr.data_ptr(), lc.data_ptr(),
             row.data_ptr(), wsf.data_ptr(), st)
        call("tt_infonce_sym_bwd", dc, q.data_ptr(), d.data_ptr(), n, h, it, lr.data_ptr(), lc.data_ptr(),
             gs.data_ptr(), dq.data_ptr(), dd.data_ptr(), wsb.data_ptr(), st)

    l1, l2, r1, r2 = (torch.empty(n, **f32) for _ in range(4))
    dq1, dd1, dq2, dd2 = (torch.empty(n, h, **f32) for _ in range(4))
    half = torch.tensor([0.5 / n], **f32)
    w1 = torch.empty(lib.tt_infonce_fwd_ws_size(n, n), dtype=torch.uint8, device=dev)
    w2 = torch.empty(lib.tt_infonce_bwd_ws_size(dc, n, n, h), dtype=torch.uint8, device=dev)

    def composed():
        for x, y, l, r, gx, gy in ((q, d, l1, r1, dq1, dd1), (d, q, l2, r2, dd2, dq2)):
            call("tt_infonce_fwd", dc, x.data_ptr(), n, y.data_ptr(), n, h, it, 0.0, 0, l.data_ptr(), r.data_ptr(),
                 w1.data_ptr(), st)
        for x, y, l, r, gx, gy in ((q, d, l1, r1, dq1, dd1), (d, q, l2, r2, dd2, dq2)):
            call("tt_infonce_bwd", dc, x.data_ptr(), n, y.data_ptr(), n, h, it, 0.0, 0, l.data_ptr(), half.data_ptr(),
                 gx.data_ptr(), gy.data_ptr(), w2.data_ptr(), st)
        dq1.add_(dq2)
        dd1.add_(dd2)

    for _ in range(a.warmup):
        fused()
        composed()
    torch.cuda.synchronize()
    loss_f = float(row.sum() / n)
    loss_c = float(0.5 * (r1.sum() + r2.sum()) / n)
    gerr = max(float((dq - dq1).abs().max() / dq1.abs().max()), float((dd - dd1).abs().max() / dd1.abs().max()))
    times = {"fused": [], "composed": []}
    for _ in range(a.iters):
        for name, fn in (("fused", fused), ("composed", composed)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {"n": n, "h": h, "dtype": "bf16", "inv_tau": it, "iters": a.iters, "unit": "us",
           "loss_fused": loss_f, "loss_composed": loss_c, "grad_rel_diff": gerr}
    for name, ts in times.items():
        res[name] = {"min": round(min(ts), 1), "median": round(statistics.median(ts), 1), "max": round(max(ts), 1)}
    res["fused_over_composed_median"] = round(res["fused"]["median"] / res["composed"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
