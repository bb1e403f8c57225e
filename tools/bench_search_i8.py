"""A/B of the serving search over one random unit-vector corpus in one process: tt_search_topk
with fp32 documents, tt_search_topk with bf16 documents and tt_search_topk_i8, timed with
device events in interleaved rounds (every round times each variant once; the median over the
rounds is reported), plus the int8 scan's group size (option search_i8_qb) and recall@k of the
int8 top-k, plain and rescored, against the fp32 top-k.

Rates are the index bytes one call has to read (N h esz, plus N 4 of scales for int8) over the
call time, against the 8 TB/s HBM spec; a call that stores a score block (Q > 64 or k > 16)
moves Q N 8 more bytes that this figure leaves out, so there it is not a share of a bound.
Plain text, one line per measurement; no threshold."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_towers_amd import _lib, ops  # noqa: E402
from two_towers_amd._lib import call, dtype_code  # noqa: E402
from two_towers_amd.serving import topk_i8  # noqa: E402

HBM_SPEC = 8.0e12


def unit_rows(n, h, seed, block=1 << 18):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(n, h, device="cuda")
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        out[r0:r1] = torch.nn.functional.normalize(torch.randn(r1 - r0, h, device="cuda", generator=g), dim=1)
    return out


def float_search(dt, qn, dn, k):
    lib = _lib.load()
    (Q, h), N = qn.shape, dn.shape[0]
    idx = torch.empty(Q, k, dtype=torch.int32, device="cuda")
    val = torch.empty(Q, k, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(lib.tt_search_ws_size(dtype_code(dt), Q, N, h, k), 1), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def run():
        call("tt_search_topk", dtype_code(dt), qn.data_ptr(), Q, dn.data_ptr(), N, h, k, idx.data_ptr(), val.data_ptr(),
             ws.data_ptr(), st)
    return run, idx, val


def i8_search(qc, qs, dc, ds, k):
    lib = _lib.load()
    (Q, h), N = qc.shape, dc.shape[0]
    idx = torch.empty(Q, k, dtype=torch.int32, device="cuda")
    val = torch.empty(Q, k, dtype=torch.float32, device="cuda")
    with _lib.option("search_i8_qb", -1):  # the larger workspace: a score block at every Q
        ws = torch.empty(max(lib.tt_search_i8_ws_size(Q, N, h, k), 1), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def run():
        call("tt_search_topk_i8", qc.data_ptr(), qs.data_ptr(), Q, dc.data_ptr(), ds.data_ptr(), N, h, k,
             idx.data_ptr(), val.data_ptr(), ws.data_ptr(), st)
    return run, idx, val


def interleaved(runs, rounds, inner):
    """{name: median microseconds per call}; every round times each variant once, in turn."""
    for f in runs.values():  # warm up every variant
        f()
    torch.cuda.synchronize()
    times = {n: [] for n in runs}
    for _ in range(rounds):
        for n, f in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                f()
            e.record()
            torch.cuda.synchronize()
            times[n].append(s.elapsed_time(e) * 1e3 / inner)
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def line(name, us, nbytes):
    med, lo, hi = us
    rate = nbytes / (med * 1e-6)
    return f"{name:>8}: {med:9.1f} us (min {lo:.1f}, max {hi:.1f})  {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_SPEC:4.1f} % of 8 TB/s"


def recall(ref_idx, idx):
    hits = (idx[:, :, None] == ref_idx[:, None, :]).any(dim=2).float().sum(dim=1)
    return float(hits.mean()) / ref_idx.shape[1]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--q", default="1,8,64,256")
    ap.add_argument("--k", default="3,100")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--recall-h", default="256,512")
    ap.add_argument("--recall-q", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_search_i8.py needs the GPU")
    N, h = a.n, a.h
    print(f"# {torch.cuda.get_device_name(0)}, {_lib.load().tt_version().decode()}; corpus N={N} h={h} random unit rows; "
          f"device events, {a.rounds} interleaved rounds of {a.inner} calls, median (min, max) per call")
    d32 = unit_rows(N, h, 1)
    dbf = d32.to(torch.bfloat16)
    dc, ds = ops.quantize_rows_i8(d32)
    nbytes = {"fp32": N * h * 4, "bf16": N * h * 2, "int8": N * h + N * 4}
    print(f"# index bytes: fp32 {nbytes['fp32'] / 2**30:.2f} GiB, bf16 {nbytes['bf16'] / 2**30:.2f} GiB, "
          f"int8 {nbytes['int8'] / 2**30:.3f} GiB")
    qmax = max(int(x) for x in a.q.split(","))
    qall = unit_rows(max(qmax, a.recall_q), h, 2)
    for Q in (int(x) for x in a.q.split(",")):
        qn = qall[:Q].contiguous()
        qc, qs = ops.quantize_rows_i8(qn)
        for k in (int(x) for x in a.k.split(",")):
            f32, _, _ = float_search(torch.float32, qn, d32, k)
            fbf, _, _ = float_search(torch.bfloat16, qn, dbf, k)
            fi8, _, _ = i8_search(qc, qs, dc, ds, k)
            res = interleaved({"fp32": f32, "bf16": fbf, "int8": fi8}, a.rounds, a.inner)
            form = "score block + radix selection" if k > 16 else (
                "scan" if Q <= 64 else "score block + split top-k")
            i8form = form if k > 16 or Q > 64 else ("scan" if Q <= (4 if k <= 4 else 2) else
                                                    "score block + split top-k")
            print(f"Q={Q} k={k} (fp32, bf16: {form}; int8: {i8form})")
            for n in ("fp32", "bf16", "int8"):
                print("  " + line(n, res[n], nbytes[n]))
            print(f"  int8 / bf16 time {res['int8'][0] / res['bf16'][0]:.3f}, int8 / fp32 time "
                  f"{res['int8'][0] / res['fp32'][0]:.3f}", flush=True)
    # the scan's queries per pass
    print("# int8, k <= 16: scan against score block and queries per scan pass (option search_i8_qb), same corpus")
    # qb=n: the fused scan, at most n queries per pass; qb=-1: the score block + column-split top-k
    for Q, k, caps in ((1, 3, (1, -1)), (8, 3, (1, 2, 4, 8, -1)), (64, 3, (2, 4, 8, -1)), (1, 10, (1, -1)),
                       (8, 10, (1, 2, -1)), (64, 10, (1, 2, -1))):
        qn = qall[:Q].contiguous()
        qc, qs = ops.quantize_rows_i8(qn)
        fi8, _, _ = i8_search(qc, qs, dc, ds, k)
        runs = {}
        for cap in caps:
            def f(cap=cap):
                _lib.set_option("search_i8_qb", cap)
                fi8()
            runs[f"qb={cap}"] = f
        res = interleaved(runs, a.rounds, a.inner)
        _lib.set_option("search_i8_qb", 0)
        print(f"Q={Q} k={k}")
        for n, us in res.items():
            print("  " + line(n, us, nbytes["int8"]), flush=True)
    # recall@10 of the int8 top-k against the fp32 top-k
    print(f"# recall@10 against tt_search_topk fp32, {a.recall_q} random unit queries, N={N}")
    k = 10
    for hh in sorted((int(x) for x in a.recall_h.split(",")), key=lambda x: x != h):  # the timed corpus first
        if hh == h:
            dd, cc, ss = d32, dc, ds
        else:
            del d32, dbf
            torch.cuda.empty_cache()
            dd = unit_rows(N, hh, 3)
            cc, ss = ops.quantize_rows_i8(dd)
        qn = unit_rows(a.recall_q, hh, 4)
        run, ridx, _ = float_search(torch.float32, qn, dd, k)
        run()
        for r in (0, 4):
            idx, _ = topk_i8(qn, cc, ss, dd if r else None, k, rescore=r)
            print(f"h={hh} rescore={r}: recall@{k} {recall(ridx.long(), idx.long()):.4f}", flush=True)
