"""Micro-benchmark of the trainable-embedding path at the bench shape (2 towers, B 8192, T 64,
E 300, H 512, bf16), each piece alone, HIP-event timed on the launching stream:
  dgrad_l0           dX0 = dG0[:, 0:6H] W_ih0 in fp32 (tt_gemm), TFLOP/s and the MFMA fraction
  embed_grad_rows    the segment sum of dX0's rows by token id (tt_embed_grad_rows, both launches)
  sparse_adam_rows   the lazy Adam step on the touched rows (tt_sparse_adam_rows)
for ids drawn uniformly and Zipf(1.0) over 20 000 and 3 000 000 rows with 10 % pads. Bytes are
algorithmic (rows read once, outputs written once, indices); the fraction is of the 8.0 TB/s
HBM spec. One JSON line per measurement; no threshold.
--union 2,4,8 times the data-parallel form instead (tt_embed_grad_rows_at, see union())."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_towers_amd import _lib, ops  # noqa: E402

HBM_PEAK_GBS = 8000.0
BF16_PEAK_TFS = 2500.0


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


def draw_ids(n, vocab, dist, pad, g):
    if dist == "uniform":
        ids = torch.randint(0, vocab, (n,), device="cuda", generator=g)
    else:  # Zipf(1.0): p(rank r) ~ 1 / r, ranks scattered over the table
        w = 1.0 / torch.arange(1, vocab + 1, device="cuda", dtype=torch.float32)
        ids = torch.multinomial(w, n, replacement=True, generator=g)
        ids = torch.randperm(vocab, device="cuda", generator=g)[ids]
    ids[torch.rand(n, device="cuda", generator=g) < pad] = -1
    return ids


def dgrad_l0(ntowers, BT, E, H, iters):
    dt = torch.bfloat16
    ep = ops.pad_cols(E, dt)
    g = torch.Generator(device="cuda").manual_seed(1)
    dG = [(torch.randn(BT, 8 * H, device="cuda", generator=g) * 0.1).to(dt) for _ in range(ntowers)]
    w = [torch.zeros(6 * H, ep, dtype=dt, device="cuda") for _ in range(ntowers)]
    for x in w:
        x[:, :E] = (torch.randn(6 * H, E, device="cuda", generator=g) * 0.05).to(dt)
    dX = torch.empty(ntowers * BT, E, dtype=torch.float32, device="cuda")
    parts = [dX[i * BT:(i + 1) * BT] for i in range(ntowers)]
    ms = timed(lambda: ops.gemm(dG, w, parts, m=BT, n=E, k=6 * H, lda=8 * H, ldb=ep, ldc=E, a_kouter=False,
                                b_kouter=True, dtype=dt, out_dtype=torch.float32), iters)
    flops = 2.0 * BT * E * 6 * H * ntowers
    nbytes = ntowers * (2 * (BT * 6 * H + 6 * H * E) + 4 * BT * E)
    tf = flops / ms / 1e9
    return {"op": "dgrad_l0", "towers": ntowers, "BT": BT, "E": E, "H": H, "ms": round(ms, 4), "tflops": round(tf, 1),
            "mfma_frac": round(tf / BF16_PEAK_TFS, 4), "gbs": round(nbytes / ms / 1e6, 1),
            "hbm_frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)}, dX


def embed(dX, vocab, dist, pad, E, iters, with_adam):
    n = dX.shape[0]
    g = torch.Generator(device="cuda").manual_seed(vocab % 1000 + len(dist))
    ids = draw_ids(n, vocab, dist, pad, g)
    perm, seg_ptr, uniq = ops.embed_plan(ids)
    m, U = perm.numel(), uniq.numel()
    counts = (seg_ptr[1:] - seg_ptr[:-1])
    rows = torch.empty(U, E, dtype=torch.float32, device="cuda")
    ws = torch.empty(_lib.load().tt_embed_grad_ws_size(m, E), dtype=torch.uint8, device="cuda")
    ms = timed(lambda: ops.embed_grad_rows(dX, perm, seg_ptr, E, rows=rows, ws=ws), iters)
    nbytes = 4.0 * (m * E + U * E) + 4.0 * (m + U + 1)
    out = [{"op": "embed_grad_rows", "vocab": vocab, "ids": dist, "n": n, "m": m, "U": U,
            "longest_segment": int(counts.max()), "ms": round(ms, 4), "gbs": round(nbytes / ms / 1e6, 1),
            "hbm_frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)}]
    if with_adam:
        dt = torch.bfloat16
        ep = ops.pad_cols(E, dt)
        w = torch.randn(vocab, E, device="cuda", generator=g)
        mom = [torch.zeros(vocab, E, device="cuda") for _ in range(2)]
        copy = torch.zeros(vocab, ep, dtype=dt, device="cuda")
        copy[:, :E] = w.to(dt)
        ids32 = uniq.to(torch.int32)
        step = [0]

        def f():
            step[0] += 1
            ops.sparse_adam_rows(w, mom[0], mom[1], ids32, rows, copy, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                                 step=step[0])
        ms = timed(f, iters)
        nbytes = U * (E * 4.0 * 7 + E * 2.0 + 4)  # g, w, m, v read; w, m, v written; the bf16 row; the id
        out.append({"op": "sparse_adam_rows", "vocab": vocab, "ids": dist, "U": U, "ms": round(ms, 4),
                    "gbs": round(nbytes / ms / 1e6, 1), "hbm_frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)})
    return out


def union(dX, vocab, pad, E, iters, ratios, reps):
    """The data-parallel form on one (dx, perm, seg_ptr) with Zipf ids: tt_embed_grad_rows, then
    tt_embed_grad_rows_at with the identity dst (nrows = U) and with nrows = R U, dst spread
    evenly (every R-th row named), which adds (R - 1) U E 4 bytes of zero stores. The variants
    are timed in turn, `reps` rounds of `iters` calls; ms is the median round, ms_min / ms_max
    the spread between rounds. Bytes are algorithmic, as above, plus the dst entries."""
    n = dX.shape[0]
    g = torch.Generator(device="cuda").manual_seed(vocab % 1000 + 4)
    ids = draw_ids(n, vocab, "zipf", pad, g)
    perm, seg_ptr, uniq = ops.embed_plan(ids)
    m, U = perm.numel(), uniq.numel()
    ws = torch.empty(_lib.load().tt_embed_grad_ws_size(m, E), dtype=torch.uint8, device="cuda")
    base = torch.empty(U, E, dtype=torch.float32, device="cuda")
    variants = [("embed_grad_rows", 0, lambda: ops.embed_grad_rows(dX, perm, seg_ptr, E, rows=base, ws=ws))]
    variants[0][2]()
    for r in [1] + list(ratios):
        dst = (torch.arange(U, device="cuda", dtype=torch.int64) * r).to(torch.int32)
        rows = torch.empty(r * U, E, dtype=torch.float32, device="cuda")
        variants.append(("embed_grad_rows_at", r, lambda dst=dst, rows=rows, r=r: ops.embed_grad_rows_at(
            dX, perm, seg_ptr, dst, r * U, E, rows=rows, ws=ws)))
        variants[-1][2]()
        assert torch.equal(rows[::r], base), "not the plain kernel's bits"
        assert r == 1 or not bool(rows.view(U, r, E)[:, 1:].any()), "an unnamed row is not zero"
    times = [[] for _ in variants]
    for _ in range(reps):
        for i, (_, _, f) in enumerate(variants):
            times[i].append(timed(f, iters))
    out = []
    for (op, r, _), t in zip(variants, times):
        t = sorted(t)
        ms = t[len(t) // 2]
        nbytes = 4.0 * (m * E + max(r, 1) * U * E) + 4.0 * (m + U + 1 + (U if r else 0))
        out.append({"op": op, "nrows_over_U": r, "vocab": vocab, "ids": "zipf", "n": n, "m": m, "U": U,
                    "ms": round(ms, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
                    "gbs": round(nbytes / ms / 1e6, 1), "hbm_frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--towers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--seq", type=int, default=64)
    ap.add_argument("--emb", type=int, default=300)
    ap.add_argument("--hidden", type=int, default=256, help="model hidden_dim (GRU H = 2 x hidden)")
    ap.add_argument("--vocabs", default="20000,3000000")
    ap.add_argument("--pad", type=float, default=0.1)
    ap.add_argument("--no-adam", action="store_true")
    ap.add_argument("--union", default="", metavar="R[,R...]",
                    help="time tt_embed_grad_rows_at instead: identity dst, then nrows = R U for each R (2,4,8)")
    ap.add_argument("--reps", type=int, default=7, help="--union: rounds over the variants (spread)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_embed_grad.py needs the GPU")
    rec, dX = dgrad_l0(a.towers, a.batch * a.seq, a.emb, 2 * a.hidden, a.iters)
    print(json.dumps(rec), flush=True)
    if a.union:
        for vocab in (int(v) for v in a.vocabs.split(",")):
            for r in union(dX, vocab, a.pad, a.emb, a.iters, [int(x) for x in a.union.split(",")], a.reps):
                print(json.dumps(r), flush=True)
        sys.exit(0)
    for vocab in (int(v) for v in a.vocabs.split(",")):
        for dist in ("uniform", "zipf"):
            for r in embed(dX, vocab, dist, a.pad, a.emb, a.iters, not a.no_adam):
                print(json.dumps(r), flush=True)
