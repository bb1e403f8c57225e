"""Thin tensor-level wrappers over the C ABI (one function per entry point family).

Every wrapper checks the operands it is handed (device, dtype, contiguity, size) so
shape mistakes fail in Python with a clear message before any kernel launches.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import torch

from . import _lib
from ._lib import GemmBatch, call, dtype_code, ptr, stream_ptr


def _esz(dt: torch.dtype) -> int:
    return 2 if dt == torch.bfloat16 else 4


def pad_cols(e: int, dt: torch.dtype) -> int:
    """Padded width of gathered embedding rows: whole 128-byte lines (one GEMM K-tile), so
    every K-tile of the layer-0 GEMMs starts on a cache line (E 300 bf16 -> 320: input
    projection l0 3.70-3.78 vs 3.82-3.85 ms per step at 304 columns, the step 0.1-1.1 %
    faster, profiles/r02_ep_align_ab.txt; the extra columns are zeros in the table and in
    W_ih l0 and add no K-tile)."""
    epc = 128 // _esz(dt)
    return (e + epc - 1) // epc * epc


def gemm(a: Sequence[torch.Tensor], b: Sequence[torch.Tensor], c: Sequence[torch.Tensor], *, m: int, n: int,
         k: int, lda: int, ldb: int, ldc: int, a_kouter: bool, b_kouter: bool, dtype: torch.dtype,
         out_dtype: torch.dtype, bias: Sequence[torch.Tensor | None] | None = None,
         bshift: Sequence[int] | None = None, alpha: float = 1.0, accumulate: bool = False,
         relu: bool = False, seq_t: int = 0, drop_seed: int = 0, drop_p: float = 0.0, drop_row0: int = 0,
         splits: int | None = None, a_hi: Sequence[torch.Tensor] | None = None, a_split: int = 0,
         c_trans: bool = False):
    """Batched C_i = alpha * op(A_i) op(B_i)^T (+bias) for up to 4 problems of one shape.
    With a_kouter and a_split > 0, A columns >= a_split are read from a_hi[i].
    c_trans: C_i is stored [n][m] (ldc >= m), written by the split-K reduction (tt_gemm_ct):
    the call must split K (see gemm_splits)."""
    nb = len(a)
    assert 1 <= nb <= 4 and len(b) == nb and len(c) == nb
    bt = GemmBatch()
    for i in range(nb):
        assert a[i].dtype == dtype and b[i].dtype == dtype, (a[i].dtype, b[i].dtype, dtype)
        assert c[i].dtype == out_dtype, (c[i].dtype, out_dtype)
        bt.a[i] = a[i].data_ptr()
        bt.b[i] = b[i].data_ptr()
        bt.c[i] = c[i].data_ptr()
        bt.bias[i] = bias[i].data_ptr() if bias is not None and bias[i] is not None else None
        bt.bshift[i] = bshift[i] if bshift is not None else 0
        if a_split:
            bt.a_hi[i] = a_hi[i].data_ptr()
    bt.a_split = a_split
    bt.drop_row0 = drop_row0 & 0xFFFFFFFF
    lib = _lib.load()
    if splits is None:
        splits = gemm_splits(m, n, k, nb, dtype)
    ws = None
    if splits > 1 and not relu and drop_p == 0.0:
        ws = torch.empty(lib.tt_gemm_ws_size(m, n, nb, splits), dtype=torch.float32, device=c[0].device)
    else:
        splits = 1
    call("tt_gemm_ct", dtype_code(dtype), dtype_code(out_dtype), int(a_kouter), int(b_kouter), m, n, k,
         ctypes.byref(bt), nb, lda, ldb, ldc, alpha, int(accumulate), int(relu), seq_t, drop_seed & 0xFFFFFFFF,
         drop_p, splits, ptr(ws), int(c_trans), stream_ptr(c[0].device))


def gemm_splits(m: int, n: int, k: int, nb: int, dtype: torch.dtype) -> int:
    """The split count gemm() uses when none is given, after tt_gemm's clamping to one
    K-tile (128 bytes of K) per split at least."""
    s = _lib.load().tt_gemm_pick_splits(m, n, k, nb)
    nk = (k * _esz(dtype) + 127) // 128
    if nk <= 0:
        return 1
    per = (nk + min(max(s, 1), nk) - 1) // min(max(s, 1), nk)
    return (nk + per - 1) // per


def embed_gather(table: torch.Tensor, ids: torch.Tensor, out: torch.Tensor):
    assert ids.dtype == torch.int32 and ids.is_contiguous()
    assert table.dim() == 2 and out.shape[-1] == table.shape[1] and out.dtype == table.dtype
    call("tt_embed_gather", dtype_code(table.dtype), table.data_ptr(), table.shape[0], table.shape[1],
         ids.data_ptr(), ids.numel(), out.data_ptr(), stream_ptr(out.device))


def embed_plan(ids: torch.Tensor):
    """(perm, seg_ptr, unique) of token ids for tt_embed_grad_rows: perm int32 [m] lists the
    flat positions of the ids >= 0 ordered by id (stable), seg_ptr int32 [U + 1] delimits one
    segment of perm per distinct id, unique int64 [U] are those ids, ascending. Index
    plumbing only (torch sort / unique_consecutive); it depends on the ids alone."""
    flat = ids.reshape(-1).to(torch.int64)
    vals, order = torch.sort(flat, stable=True)
    keep = vals >= 0
    vals, order = vals[keep], order[keep]
    uniq, counts = torch.unique_consecutive(vals, return_counts=True)
    seg_ptr = torch.zeros(uniq.numel() + 1, dtype=torch.int32, device=flat.device)
    seg_ptr[1:] = torch.cumsum(counts, 0)
    return order.to(torch.int32).contiguous(), seg_ptr, uniq


def embed_grad_chunk() -> int:
    """Sorted positions per workgroup of tt_embed_grad_rows."""
    return int(_lib.load().tt_embed_grad_chunk())


def embed_grad_rows(dx: torch.Tensor, perm: torch.Tensor, seg_ptr: torch.Tensor, e: int | None = None,
                    rows: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> torch.Tensor:
    """rows[u] = sum of dx[perm[p], :e] over segment u of (perm, seg_ptr), fp32 [U, e]
    (tt_embed_grad_rows: fixed summation order, no atomics)."""
    assert dx.dtype == torch.float32 and dx.dim() == 2 and dx.stride(1) == 1
    assert perm.dtype == torch.int32 and perm.is_contiguous() and seg_ptr.dtype == torch.int32 and seg_ptr.is_contiguous()
    _lib.require_gpu(dx, perm, seg_ptr)
    e = dx.shape[1] if e is None else e
    u, m = seg_ptr.numel() - 1, perm.numel()
    if rows is None:
        rows = torch.empty(u, e, dtype=torch.float32, device=dx.device)
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() >= u * e
    if ws is None:
        ws = torch.empty(_lib.load().tt_embed_grad_ws_size(m, e), dtype=torch.uint8, device=dx.device)
    assert ws.numel() * ws.element_size() >= _lib.load().tt_embed_grad_ws_size(m, e)
    call("tt_embed_grad_rows", dx.data_ptr(), dx.shape[0], dx.stride(0), perm.data_ptr(), m, seg_ptr.data_ptr(), u, e,
         rows.data_ptr(), ws.data_ptr(), stream_ptr(dx.device))
    return rows


def embed_grad_rows_at(dx: torch.Tensor, perm: torch.Tensor, seg_ptr: torch.Tensor, dst: torch.Tensor, nrows: int,
                       e: int | None = None, rows: torch.Tensor | None = None,
                       ws: torch.Tensor | None = None) -> torch.Tensor:
    """embed_grad_rows with segment u's sum at rows[dst[u]] of an fp32 [nrows, e] buffer whose
    other rows the call zeroes (tt_embed_grad_rows_at): dst int32 [U], strictly ascending."""
    assert dx.dtype == torch.float32 and dx.dim() == 2 and dx.stride(1) == 1
    assert perm.dtype == torch.int32 and perm.is_contiguous() and seg_ptr.dtype == torch.int32 and seg_ptr.is_contiguous()
    assert dst.dtype == torch.int32 and dst.is_contiguous()
    _lib.require_gpu(dx, perm, seg_ptr, dst)
    e = dx.shape[1] if e is None else e
    u, m = seg_ptr.numel() - 1, perm.numel()
    assert dst.numel() == u and nrows >= u
    if rows is None:
        rows = torch.empty(nrows, e, dtype=torch.float32, device=dx.device)
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() >= nrows * e
    if ws is None:
        ws = torch.empty(_lib.load().tt_embed_grad_ws_size(m, e), dtype=torch.uint8, device=dx.device)
    assert ws.numel() * ws.element_size() >= _lib.load().tt_embed_grad_ws_size(m, e)
    call("tt_embed_grad_rows_at", dx.data_ptr(), dx.shape[0], dx.stride(0), perm.data_ptr(), m, seg_ptr.data_ptr(), u,
         dst.data_ptr(), nrows, e, rows.data_ptr(), ws.data_ptr(), stream_ptr(dx.device))
    return rows


def sparse_adam_rows(weight: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, ids: torch.Tensor,
                     rows: torch.Tensor, copy: torch.Tensor | None, *, lr: float, beta1: float, beta2: float,
                     eps: float, step: int, guard: torch.Tensor | None = None):
    """torch.optim.SparseAdam's update of weight[ids] (and the moments) from the gradient rows;
    copy: the padded compute-dtype table whose rows follow (tt_sparse_adam_rows)."""
    v, e = weight.shape
    for t in (weight, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (v, e)
    assert ids.dtype == torch.int32 and ids.is_contiguous()
    assert rows.dtype == torch.float32 and rows.is_contiguous() and tuple(rows.shape) == (ids.numel(), e)
    _lib.require_gpu(weight, exp_avg, exp_avg_sq, ids, rows, copy)
    if copy is not None:
        assert copy.is_contiguous() and copy.shape[0] == v and copy.shape[1] >= e
    call("tt_sparse_adam_rows", weight.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), v, e, ids.data_ptr(),
         rows.data_ptr(), ids.numel(), dtype_code(copy.dtype) if copy is not None else 0, ptr(copy),
         copy.shape[1] if copy is not None else 0, lr, beta1, beta2, eps, step, ptr(guard), stream_ptr(weight.device))


def pack_rows(src: torch.Tensor, out: torch.Tensor):
    assert src.dtype == torch.float32 and src.is_contiguous()
    e = src.shape[-1]
    n = src.numel() // e
    call("tt_pack_rows", dtype_code(out.dtype), src.data_ptr(), n, e, out.shape[-1], out.data_ptr(),
         stream_ptr(out.device))


def cast(x: torch.Tensor, out: torch.Tensor):
    assert x.dtype == torch.float32 and x.is_contiguous() and out.numel() == x.numel()
    call("tt_cast", dtype_code(out.dtype), x.data_ptr(), x.numel(), out.data_ptr(), stream_ptr(out.device))


def colsum(x: torch.Tensor, rows: int, cols: int, ld: int, out: torch.Tensor, accumulate: bool = False):
    assert x.dtype == torch.float32 and out.dtype == torch.float32
    call("tt_colsum", x.data_ptr(), rows, cols, ld, out.data_ptr(), int(accumulate), stream_ptr(out.device))


def total(x: torch.Tensor, scale: float, out: torch.Tensor):
    call("tt_sum", x.data_ptr(), x.numel(), scale, out.data_ptr(), stream_ptr(out.device))


def l2norm_fwd(x: torch.Tensor, eps: float, dt: torch.dtype, want_f32: bool = True):
    """Returns (y in dt, y32 fp32 or None, norm [rows])."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    rows, cols = x.shape
    y = torch.empty(rows, cols, dtype=dt, device=x.device)
    y32 = y if dt == torch.float32 else (torch.empty_like(x) if want_f32 else None)
    norm = torch.empty(rows, dtype=torch.float32, device=x.device)
    call("tt_l2norm_fwd", dtype_code(dt), x.data_ptr(), rows, cols, eps, y.data_ptr(),
         None if y32 is y else ptr(y32), norm.data_ptr(), stream_ptr(x.device))
    return y, y32, norm


def l2norm_bwd(dy: torch.Tensor, y32: torch.Tensor, norm: torch.Tensor, eps: float, dx: torch.Tensor | None = None,
               accumulate: bool = False):
    assert dy.dtype == torch.float32 and dy.is_contiguous() and y32.dtype == torch.float32
    rows, cols = dy.shape
    if dx is None:
        dx = torch.empty_like(dy)
        accumulate = False
    call("tt_l2norm_bwd", dy.data_ptr(), y32.data_ptr(), norm.data_ptr(), rows, cols, eps, dx.data_ptr(),
         int(accumulate), stream_ptr(dy.device))
    return dx


# ------------------------------------------------------------------ int8 index
def quantize_rows_i8(x: torch.Tensor):
    """Symmetric per-row int8 codes of fp32 rows (tt_quantize_rows_i8): (codes int8 [rows,
    cols], scale fp32 [rows]) with codes = clamp(round(x * (127 / amax)), -127, 127) and
    scale = amax / 127 per row. x may be a column slice of a wider matrix (row stride a
    multiple of 4)."""
    _lib.require_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.TTError("quantize_rows_i8: x must be fp32 [rows, cols] with unit column stride")
    rows, cols = x.shape
    ld = x.stride(0) if rows > 1 else max(x.stride(0), cols)
    if cols % 16 or not 0 < cols <= 1024:
        raise _lib.TTError(f"quantize_rows_i8: cols={cols} must be a multiple of 16 and at most 1024")
    if ld < cols or ld % 4 or x.data_ptr() % 16:
        raise _lib.TTError(f"quantize_rows_i8: row stride {ld} must be a multiple of 4 (>= cols) and x 16-byte aligned")
    codes = torch.empty(rows, cols, dtype=torch.int8, device=x.device)
    scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    call("tt_quantize_rows_i8", x.data_ptr(), rows, cols, ld, codes.data_ptr(), scale.data_ptr(), stream_ptr(x.device))
    return codes, scale


def search_topk_i8(qc: torch.Tensor, qs: torch.Tensor, dc: torch.Tensor, ds: torch.Tensor, k: int):
    """Top-k of every query over an int8 index (tt_search_topk_i8): (idx int32 [Q, k], val fp32
    [Q, k]), val = ((float)dot * ds) * qs. The queries go in chunks so that a stored score
    block stays within 1 GiB (k > 16) / 4 GiB (k <= 16)."""
    _lib.require_gpu(qc, qs, dc, ds)
    for c, s, what in ((qc, qs, "query"), (dc, ds, "document")):
        if c.dtype != torch.int8 or c.dim() != 2 or not c.is_contiguous():
            raise _lib.TTError(f"search_topk_i8: {what} codes must be a contiguous int8 matrix")
        if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() != c.shape[0]:
            raise _lib.TTError(f"search_topk_i8: {what} scales must be fp32 [{c.shape[0]}]")
    if qc.shape[1] != dc.shape[1]:
        raise _lib.TTError(f"search_topk_i8: query width {qc.shape[1]} != document width {dc.shape[1]}")
    lib = _lib.load()
    (Q, h), nd = qc.shape, dc.shape[0]
    idx = torch.empty(Q, k, dtype=torch.int32, device=qc.device)
    val = torch.empty(Q, k, dtype=torch.float32, device=qc.device)
    if k > 16:
        step = max(1, min(Q, (1 << 28) // max(nd, 1)))
    else:
        step = max(1, min(Q, (1 << 30) // max(nd, 1)))
    for r0 in range(0, Q, max(step, 1)):
        r1 = min(Q, r0 + step)
        ws = torch.empty(max(lib.tt_search_i8_ws_size(r1 - r0, nd, h, k), 1), dtype=torch.uint8, device=qc.device)
        call("tt_search_topk_i8", qc[r0:r1].data_ptr(), qs[r0:r1].data_ptr(), r1 - r0, dc.data_ptr(), ds.data_ptr(), nd,
             h, k, idx[r0:r1].data_ptr(), val[r0:r1].data_ptr(), ws.data_ptr(), stream_ptr(qc.device))
    return idx, val


def gather_scores(qn: torch.Tensor, dn: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """out[i, r] = qn[i] . dn[cand[i, r]] in fp32 (tt_gather_scores): qn fp32 [Q, h], dn [N, h]
    fp32 or bf16, cand int32 [Q, R] with 1 <= R <= 1024; a candidate outside [0, N) scores
    -FLT_MAX."""
    _lib.require_gpu(qn, dn, cand)
    if qn.dtype != torch.float32 or qn.dim() != 2 or not qn.is_contiguous():
        raise _lib.TTError("gather_scores: qn must be a contiguous fp32 matrix")
    if dn.dim() != 2 or not dn.is_contiguous() or dn.shape[1] != qn.shape[1]:
        raise _lib.TTError(f"gather_scores: dn must be contiguous [N, {qn.shape[1]}]")
    if cand.dtype != torch.int32 or cand.dim() != 2 or not cand.is_contiguous() or cand.shape[0] != qn.shape[0]:
        raise _lib.TTError(f"gather_scores: cand must be contiguous int32 [{qn.shape[0]}, R]")
    (Q, h), R = qn.shape, cand.shape[1]
    if h % 8 or not 1 <= R <= _lib.topk_max():
        raise _lib.TTError(f"gather_scores: h={h} must be a multiple of 8 and 1 <= R={R} <= {_lib.topk_max()}")
    out = torch.empty(Q, R, dtype=torch.float32, device=qn.device)
    call("tt_gather_scores", dtype_code(dn.dtype), qn.data_ptr(), Q, dn.data_ptr(), dn.shape[0], h, cand.data_ptr(), R,
         out.data_ptr(), stream_ptr(qn.device))
    return out
