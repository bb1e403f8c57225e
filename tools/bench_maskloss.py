"""A/B: what the group masks cost. Through the C ABI in one process, on one box:

  InfoNCE forward + backward (tt_infonce_fwd/_bwd) at B x B, h, bf16:
      plain      the ungrouped entry points
      grp_none   tt_infonce_fwd_grp/_bwd_grp with every id -1 (the grouped kernels, nothing excluded)
      grp_1pct   the same with about 1 % of the pairs in groups of 2-3
  mining at k = 5 (losses.mine_hard_negatives, l2norm included in both):
      mine_plain   tt_hardneg_topk k = 5
      mine_grp     k = 5, max_group_size = 3 (g = 2): tt_hardneg_topk k = 7 + tt_topk_drop_groups

    python tools/bench_maskloss.py [--n 8192] [--h 256] [--iters 50] [--out profiles/maskloss_ab.json]

Device-event times per iteration, the variants interleaved in every round so clock and
neighbour drift hit all alike; reports min / median / max per variant, the spread of the plain
variant ((max - min) / median, and the interquartile range) against which a difference is to be
read, and checks that grp_none reproduces the plain bits.
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
from two_towers_amd.losses import mine_hard_negatives  # noqa: E402


def make_groups(n: int, frac: float, seed: int = 1) -> torch.Tensor:
    """int32 [n]: about frac of the pairs in groups of 2 or 3 (random members), the rest -1."""
    gen = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n, generator=gen)
    g = torch.full((n,), -1, dtype=torch.int32)
    want, pos, gid = int(frac * n), 0, 0
    while pos + 3 <= want:
        size = 2 + gid % 2
        g[perm[pos:pos + size]] = gid
        pos += size
        gid += 1
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--h", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inv-tau", type=float, default=1 / 0.07)
    ap.add_argument("--frac", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_maskloss.py measures on the GPU; none is visible")
    dev, bf = "cuda", torch.bfloat16
    n, h, it = a.n, a.h, a.inv_tau
    gen = torch.Generator().manual_seed(0)
    q32 = torch.randn(n, h, generator=gen).to(dev)
    d32 = torch.randn(n, h, generator=gen).to(dev)
    q = torch.nn.functional.normalize(q32, dim=1).to(bf).contiguous()
    d = torch.nn.functional.normalize(d32, dim=1).to(bf).contiguous()
    dc = dtype_code(bf)
    st = torch.cuda.current_stream().cuda_stream
    f32 = dict(dtype=torch.float32, device=dev)
    gs = torch.tensor([1.0 / n], **f32)
    wf = torch.empty(lib.tt_infonce_fwd_ws_size(n, n), dtype=torch.uint8, device=dev)
    wb = torch.empty(lib.tt_infonce_bwd_ws_size(dc, n, n, h), dtype=torch.uint8, device=dev)
    none = torch.full((n,), -1, dtype=torch.int32, device=dev)
    some = make_groups(n, a.frac).to(dev)
    in_groups = int((some >= 0).sum())
    mgs = int(torch.unique(some[some >= 0], return_counts=True)[1].max()) if in_groups else 1

    outs = {name: (torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, h, **f32), torch.empty(n, h, **f32))
            for name in ("plain", "grp_none", "grp_1pct")}

    def plain():
        lse, row, dq, dd = outs["plain"]
        call("tt_infonce_fwd", dc, q.data_ptr(), n, d.data_ptr(), n, h, it, 0.0, 0, lse.data_ptr(), row.data_ptr(),
             wf.data_ptr(), st)
        call("tt_infonce_bwd", dc, q.data_ptr(), n, d.data_ptr(), n, h, it, 0.0, 0, lse.data_ptr(), gs.data_ptr(),
             dq.data_ptr(), dd.data_ptr(), wb.data_ptr(), st)

    def grouped(name, ids):
        def run():
            lse, row, dq, dd = outs[name]
            call("tt_infonce_fwd_grp", dc, q.data_ptr(), n, d.data_ptr(), n, h, it, 0.0, 0, ids.data_ptr(),
                 ids.data_ptr(), lse.data_ptr(), row.data_ptr(), wf.data_ptr(), st)
            call("tt_infonce_bwd_grp", dc, q.data_ptr(), n, d.data_ptr(), n, h, it, 0.0, 0, ids.data_ptr(),
                 ids.data_ptr(), lse.data_ptr(), gs.data_ptr(), dq.data_ptr(), dd.data_ptr(), wb.data_ptr(), st)
        return run

    def mine_plain():
        return mine_hard_negatives(q32, d32, 0, 5, bf)

    def mine_grp():
        return mine_hard_negatives(q32, d32, 0, 5, bf, row_groups=some, col_groups=some, max_group_size=max(mgs, 3))

    variants = [("plain", plain), ("grp_none", grouped("grp_none", none)), ("grp_1pct", grouped("grp_1pct", some)),
                ("mine_plain", mine_plain), ("mine_grp", mine_grp)]
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
               for x, y in zip(outs["plain"], outs["grp_none"]))
    times = {name: [] for name, _ in variants}
    for _ in range(a.iters):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {"n": n, "h": h, "dtype": "bf16", "inv_tau": it, "iters": a.iters, "unit": "us",
           "pairs_in_groups": in_groups, "max_group_size": mgs, "grp_none_bits_equal_plain": same,
           "loss_plain": float(outs["plain"][1].sum() / n), "loss_grp_1pct": float(outs["grp_1pct"][1].sum() / n)}
    for name, ts in times.items():
        qs = statistics.quantiles(ts, n=4)
        res[name] = {"min": round(min(ts), 1), "median": round(statistics.median(ts), 1), "max": round(max(ts), 1),
                     "iqr": round(qs[2] - qs[0], 1)}
    for base, names in (("plain", ("grp_none", "grp_1pct")), ("mine_plain", ("mine_grp",))):
        b = res[base]
        res[base + "_spread"] = round((b["max"] - b["min"]) / b["median"], 4)
        for name in names:
            res[f"{name}_over_{base}_median"] = round(res[name]["median"] / b["median"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
