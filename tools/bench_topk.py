"""Micro-benchmark of the k > 16 top-k (HIP-event timed on the launching stream): the
selection on its own (tt_topk_rows over a stored score block), the whole tt_search_topk /
tt_hardneg_topk call (cast + cosine GEMM + selection), and torch.topk over the same score
block on the same device as the baseline. One JSON line per (shape, k); no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import call, dtype_code  # noqa: E402


def timed(f, iters):
    f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def operands(rows, n, h, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(rows, h, device="cuda", generator=g), dim=1)
    d = torch.nn.functional.normalize(torch.randn(n, h, device="cuda", generator=g), dim=1).to(dt)
    return q, d


def select_and_baseline(S, lab, k, iters):
    """tt_topk_rows and torch.topk over the block S (label column already -1 in S for torch)."""
    lib = _lib.load()
    rows, cols = S.shape
    idx = torch.empty(rows, k, dtype=torch.int32, device="cuda")
    val = torch.empty(rows, k, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(lib.tt_topk_rows_ws_size(rows, cols, k), 1), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms_sel = timed(lambda: call("tt_topk_rows", S.data_ptr(), rows, cols, cols, lab, k, idx.data_ptr(), val.data_ptr(),
                                ws.data_ptr(), st), iters)
    ms_torch = timed(lambda: torch.topk(S, k, dim=1), iters)
    tv = torch.topk(S, k, dim=1).values
    return ms_sel, ms_torch, bool(torch.equal(tv, val))


def search(Q, N, h, k, dt, iters):
    lib = _lib.load()
    q, d = operands(Q, N, h, dt, 5)
    idx = torch.empty(Q, k, dtype=torch.int32, device="cuda")
    val = torch.empty(Q, k, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.tt_search_ws_size(dtype_code(dt), Q, N, h, k), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: call("tt_search_topk", dtype_code(dt), q.data_ptr(), Q, d.data_ptr(), N, h, k, idx.data_ptr(),
                            val.data_ptr(), ws.data_ptr(), st), iters)
    S = q.to(dt).float() @ d.float().t()
    ms_sel, ms_torch, same = select_and_baseline(S, -1, k, iters)
    return {"op": "search_topk", "Q": Q, "N": N, "h": h, "k": k, "dtype": str(dt)[6:], "call_ms": round(ms, 4),
            "topk_rows_ms": round(ms_sel, 4), "torch_topk_ms": round(ms_torch, 4), "values_equal_torch": same}


def mining(B, nd, h, k, dt, iters):
    lib = _lib.load()
    q, d = operands(B, nd, h, dt, 6)
    q = q.to(dt)
    idx = torch.empty(B, k, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.tt_hardneg_ws_size(dtype_code(dt), B, nd, h, k), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: call("tt_hardneg_topk", dtype_code(dt), q.data_ptr(), B, d.data_ptr(), nd, h, 0, k,
                            idx.data_ptr(), None, ws.data_ptr(), st), iters)
    S = q.float() @ d.float().t()
    S.fill_diagonal_(-1.0)
    ms_sel, ms_torch, same = select_and_baseline(S, 0, k, iters)
    return {"op": "hardneg_topk", "B": B, "nd": nd, "h": h, "k": k, "dtype": str(dt)[6:], "call_ms": round(ms, 4),
            "topk_rows_ms": round(ms_sel, 4), "torch_topk_ms": round(ms_torch, 4), "values_equal_torch": same}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--search", default="1x1048576x256,64x1048576x256", help="search shapes Q x N x h")
    ap.add_argument("--search-k", default="100,1000")
    ap.add_argument("--mining", default="8192x8192x256", help="mining shapes B x N x h")
    ap.add_argument("--mining-k", default="64")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_topk.py needs the GPU")
    bf = torch.bfloat16
    for shp in filter(None, a.search.split(",")):
        Q, N, h = (int(x) for x in shp.split("x"))
        for k in (int(x) for x in a.search_k.split(",")):
            print(json.dumps(search(Q, N, h, k, bf, a.iters)), flush=True)
    for shp in filter(None, a.mining.split(",")):
        B, nd, h = (int(x) for x in shp.split("x"))
        for k in (int(x) for x in a.mining_k.split(",")):
            print(json.dumps(mining(B, nd, h, k, bf, a.iters)), flush=True)
