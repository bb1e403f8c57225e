"""Micro-benchmark of the full-rank count (HIP-event timed on the launching stream): the
streamed scan with the counting epilogue (tt_rank_count, bf16, h 256) against the stored path
in the same process (option rank_gemm = 1: tt_gemm into a row block + a count over it, what
the pieces cost without the fused kernel), tt_rank_best_relevant on its own, and
tt_hardneg_topk with k 5 on the same operands as the comparison point. A large corpus is
counted in document blocks with col_offset and accumulate. One JSON line per shape; the
two paths' counts are compared (counts_equal); no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import call, dtype_code, option  # noqa: E402


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


def operands(Q, N, h, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(Q, h, device="cuda", generator=g), dim=1).to(dt)
    d = torch.nn.functional.normalize(torch.randn(N, h, device="cuda", generator=g), dim=1).to(dt)
    # one relevant document per query, anywhere in the corpus
    idx = torch.randint(0, N, (Q,), device="cuda", generator=g, dtype=torch.int32)
    ptr = torch.arange(Q + 1, device="cuda", dtype=torch.int32)
    return q, d, ptr, idx


def counter(q, d, theta, tcol, dt, block):
    """A closure counting all of d in blocks of `block` rows under the current options."""
    lib = _lib.load()
    Q, h = q.shape
    N = d.shape[0]
    dc = dtype_code(dt)
    count = torch.empty(Q, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(lib.tt_rank_count_ws_size(dc, Q, min(block, N), h), 1), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def run():
        for b0 in range(0, N, block):
            n = min(N, b0 + block) - b0
            call("tt_rank_count", dc, q.data_ptr(), Q, d[b0:].data_ptr(), n, h, b0, theta.data_ptr(), tcol.data_ptr(),
                 count.data_ptr(), 1 if b0 else 0, ws.data_ptr(), st)
    return run, count


def bench(Q, N, h, block, dt, iters, mining):
    lib = _lib.load()
    q, d, ptr, idx = operands(Q, N, h, dt, 9)
    dc = dtype_code(dt)
    theta = torch.empty(Q, dtype=torch.float32, device="cuda")
    tcol = torch.empty(Q, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms_best = timed(lambda: call("tt_rank_best_relevant", dc, q.data_ptr(), Q, d.data_ptr(), N, h, ptr.data_ptr(),
                                 idx.data_ptr(), theta.data_ptr(), tcol.data_ptr(), None, st), iters)
    block = block or N
    with option("rank_gemm", 0):
        run, count = counter(q, d, theta, tcol, dt, block)
        ms_scan = timed(run, iters)
        scan = count.clone()
    with option("rank_gemm", 1):
        run, count = counter(q, d, theta, tcol, dt, block)
        ms_stored = timed(run, max(1, iters // 4))
        stored = count.clone()
    out = {"op": "rank_count", "Q": Q, "N": N, "h": h, "dtype": str(dt)[6:], "doc_block": block,
           "best_relevant_ms": round(ms_best, 4), "scan_ms": round(ms_scan, 4), "stored_ms": round(ms_stored, 4),
           "scan_tflops": round(2.0 * Q * N * h / ms_scan * 1e-9, 1), "counts_equal": bool(torch.equal(scan, stored)),
           "mean_rank": round(float((scan + 1).double().mean()), 1), "device": torch.cuda.get_device_name(0)}
    if mining:
        mi = torch.empty(Q, 5, dtype=torch.int32, device="cuda")
        mws = torch.empty(lib.tt_hardneg_ws_size(dc, Q, N, h, 5), dtype=torch.uint8, device="cuda")
        out["hardneg_k5_ms"] = round(timed(lambda: call("tt_hardneg_topk", dc, q.data_ptr(), Q, d.data_ptr(), N, h, -1, 5,
                                                       mi.data_ptr(), None, mws.data_ptr(), st), iters), 4)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="8192x8192x256,8192x65536x256,1024x1000000x256:131072",
                    help="Q x N x h[:doc_block], comma separated")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rank.py needs the GPU")
    for shp in filter(None, a.shapes.split(",")):
        dims, _, blk = shp.partition(":")
        Q, N, h = (int(x) for x in dims.split("x"))
        print(json.dumps(bench(Q, N, h, int(blk) if blk else 0, torch.bfloat16, a.iters, mining=N <= 65536)), flush=True)
