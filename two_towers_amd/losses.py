"""Contrastive losses of enhanced_two_tower.py on the HIP path.

  InfoNCELoss(temperature=0.07)                 enhanced_two_tower.py:67-82
  MarginRankingLoss(margin=0.2, temperature=0.1) enhanced_two_tower.py:84-121
  get_hard_negatives(q, docs, positive_idx, k)   enhanced_two_tower.py:123-133
  HardNegativeMarginLoss(k=5, margin=0.2)        the config-3 composition:
      mine k hard negatives per query among the (global) doc pool, then the
      explicit-negative MarginRankingLoss — fused, without gathering negative rows.

Group masks (in-batch false negatives, DESIGN.md §3 "Group masks"): the in-batch losses and
the mining take `groups`, one integer id per pair. The pair is both row i and column i, and
column j is excluded for row i iff j is not i's own column, groups[i] >= 0 and groups[j] ==
groups[i] (the group rule of include/tt_hip.h). A negative id is "no group". The ids go to
the kernels as int32 and never appear in autograd; groups=None is the code path without them.

Every loss takes an optional torch.distributed process group: with world > 1 the
normalised doc vectors are all-gathered (global negative pool) and each rank returns
the GLOBAL mean loss while back-propagating only its own rows' share (see dist.py).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, dist, ops, timing
from ._lib import call, dtype_code, ptr, stream_ptr


def _dt_of(x: torch.Tensor, compute_dtype):
    return compute_dtype if compute_dtype is not None else torch.float32


def _finish_loss(local_sum: torch.Tensor, scale: float, group):
    """local_sum * scale as this rank's differentiable share; value = global mean."""
    loss = local_sum * scale
    if dist.active(group):
        tot = loss.detach().clone()
        dist.all_reduce_sum_(tot, group)
        loss = loss + (tot - loss.detach())
    return loss


def _group_ids(groups, B: int, device) -> torch.Tensor:
    """groups [B] of any integer dtype -> contiguous int32 on the device, detached."""
    g = torch.as_tensor(groups)
    if g.dtype.is_floating_point or g.dtype == torch.bool or g.dim() != 1 or g.shape[0] != B:
        raise _lib.TTError(f"groups must be an integer tensor [{B}] (one id per pair), got {g.dtype} "
                           f"{tuple(g.shape)}")
    return g.detach().to(device=device, dtype=torch.int32).contiguous()


class _NormCE(torch.autograd.Function):
    """sum_i CE_i over S = inv_tau * qn dn_global^T (- offdiag off the label), with
    qn/dn = normalize(q/d) (or raw when normalize=False). Returns the local row sum."""

    @staticmethod
    def forward(ctx, q, d, inv_tau, offdiag, eps, do_norm, dt, group, gids=None):
        """gids: this rank's int32 ids [B] or None. The column ids are the ranks' ids
        all-gathered like the document rows, the row ids the local ones."""
        _lib.require_gpu(q, d)
        q = q.float().contiguous()
        d = d.float().contiguous()
        rank, world = dist.rank_world(group)
        B = q.shape[0]
        if do_norm:
            qn, qn32, qnorm = ops.l2norm_fwd(q, eps, dt)
            dn_l, dn32, dnorm = ops.l2norm_fwd(d, eps, dt)
        else:
            qn, qn32, qnorm = (q if dt == torch.float32 else q.to(dt)), q, None
            dn_l, dn32, dnorm = (d if dt == torch.float32 else d.to(dt)), d, None
        dn = dist.all_gather_rows(dn_l, group)
        nd = dn.shape[0]
        lse = torch.empty(B, dtype=torch.float32, device=q.device)
        row = torch.empty(B, dtype=torch.float32, device=q.device)
        lib = _lib.load()
        ws = torch.empty(lib.tt_infonce_fwd_ws_size(B, nd), dtype=torch.uint8, device=q.device)
        esz = 2 if dt == torch.bfloat16 else 4
        cids = None if gids is None else dist.all_gather_rows(gids, group)
        with timing.region("infonce_fwd", 1, 2.0 * B * nd * q.shape[1], float(esz * (B + nd) * q.shape[1] + 8 * B)):
            if gids is None:
                call("tt_infonce_fwd", dtype_code(dt), qn.data_ptr(), B, dn.data_ptr(), nd, q.shape[1], inv_tau,
                     offdiag, rank * B, lse.data_ptr(), row.data_ptr(), ws.data_ptr(), stream_ptr(q.device))
            else:
                call("tt_infonce_fwd_grp", dtype_code(dt), qn.data_ptr(), B, dn.data_ptr(), nd, q.shape[1], inv_tau,
                     offdiag, rank * B, gids.data_ptr(), cids.data_ptr(), lse.data_ptr(), row.data_ptr(),
                     ws.data_ptr(), stream_ptr(q.device))
        out = torch.empty((), dtype=torch.float32, device=q.device)
        ops.total(row, 1.0, out)
        ctx.gids = (gids, cids)
        ctx.save = (qn, qn32, qnorm, dn, dn32, dnorm, lse)
        ctx.cfg = (inv_tau, offdiag, eps, do_norm, dt, group, rank, B)
        return out

    @staticmethod
    def backward(ctx, gout):
        qn, qn32, qnorm, dn, dn32, dnorm, lse = ctx.save
        inv_tau, offdiag, eps, do_norm, dt, group, rank, B = ctx.cfg
        h = qn.shape[1]
        nd = dn.shape[0]
        # the scalar upstream gradient stays on the device: the kernels read it
        gdev = gout.detach().float().reshape(1).contiguous()
        dqn = torch.empty(B, h, dtype=torch.float32, device=qn.device)
        ddn = torch.empty(nd, h, dtype=torch.float32, device=qn.device)
        lib = _lib.load()
        ws = torch.empty(lib.tt_infonce_bwd_ws_size(dtype_code(dt), B, nd, h), dtype=torch.uint8, device=qn.device)
        gids, cids = ctx.gids
        if gids is None:
            call("tt_infonce_bwd", dtype_code(dt), qn.data_ptr(), B, dn.data_ptr(), nd, h, inv_tau, offdiag, rank * B,
                 lse.data_ptr(), gdev.data_ptr(), dqn.data_ptr(), ddn.data_ptr(), ws.data_ptr(),
                 stream_ptr(qn.device))
        else:
            call("tt_infonce_bwd_grp", dtype_code(dt), qn.data_ptr(), B, dn.data_ptr(), nd, h, inv_tau, offdiag,
                 rank * B, gids.data_ptr(), cids.data_ptr(), lse.data_ptr(), gdev.data_ptr(), dqn.data_ptr(),
                 ddn.data_ptr(), ws.data_ptr(), stream_ptr(qn.device))
        ddn_l = dist.reduce_scatter_rows(ddn, group)
        if do_norm:
            dq = ops.l2norm_bwd(dqn, qn32, qnorm, eps)
            dd = ops.l2norm_bwd(ddn_l, dn32, dnorm, eps)
        else:
            dq, dd = dqn, ddn_l
        return dq, dd, None, None, None, None, None, None, None


class InfoNCELoss(nn.Module):
    """enhanced_two_tower.py:67-82: CE over normalised q·dᵀ / temperature, labels = arange."""

    def __init__(self, temperature=0.07, compute_dtype=None, process_group=None):
        super().__init__()
        self.temperature = temperature
        self.compute_dtype = compute_dtype
        self.process_group = process_group

    def forward(self, query_vec, doc_vec, groups=None):
        dt = _dt_of(query_vec, self.compute_dtype)
        _, world = dist.rank_world(self.process_group)
        if groups is None:
            s = _NormCE.apply(query_vec, doc_vec, 1.0 / self.temperature, 0.0, 1e-12, True, dt, self.process_group)
        else:
            s = _NormCE.apply(query_vec, doc_vec, 1.0 / self.temperature, 0.0, 1e-12, True, dt, self.process_group,
                              _group_ids(groups, query_vec.shape[0], query_vec.device))
        return _finish_loss(s, 1.0 / (query_vec.shape[0] * world), self.process_group)


class _SymCE(torch.autograd.Function):
    """sum_i ((lse_row_i - S_ii) + (lse_col_i - S_ii)) / 2 over the square S = inv_tau qn dn^T
    (one process): tt_infonce_sym_fwd / _bwd, both LSE vectors saved for the backward."""

    @staticmethod
    def forward(ctx, q, d, inv_tau, eps, do_norm, dt, gids=None):
        _lib.require_gpu(q, d)
        q = q.float().contiguous()
        d = d.float().contiguous()
        if q.dim() != 2 or q.shape != d.shape:
            raise _lib.TTError(f"SymmetricInfoNCELoss expects two [B, h] batches of one shape, got "
                               f"{tuple(q.shape)} and {tuple(d.shape)}")
        B, h = q.shape
        if do_norm:
            qn, qn32, qnorm = ops.l2norm_fwd(q, eps, dt)
            dn, dn32, dnorm = ops.l2norm_fwd(d, eps, dt)
        else:
            qn, qn32, qnorm = (q if dt == torch.float32 else q.to(dt)), q, None
            dn, dn32, dnorm = (d if dt == torch.float32 else d.to(dt)), d, None
        lse_row = torch.empty(B, dtype=torch.float32, device=q.device)
        lse_col = torch.empty(B, dtype=torch.float32, device=q.device)
        row = torch.empty(B, dtype=torch.float32, device=q.device)
        lib = _lib.load()
        ws = torch.empty(lib.tt_infonce_sym_fwd_ws_size(B, h), dtype=torch.uint8, device=q.device)
        esz = 2 if dt == torch.bfloat16 else 4
        with timing.region("infonce_sym_fwd", 1, 2.0 * B * B * h, float(esz * 2 * B * h + 12 * B)):
            if gids is None:
                call("tt_infonce_sym_fwd", dtype_code(dt), qn.data_ptr(), dn.data_ptr(), B, h, inv_tau,
                     lse_row.data_ptr(), lse_col.data_ptr(), row.data_ptr(), ws.data_ptr(), stream_ptr(q.device))
            else:
                call("tt_infonce_sym_fwd_grp", dtype_code(dt), qn.data_ptr(), dn.data_ptr(), B, h, inv_tau,
                     gids.data_ptr(), lse_row.data_ptr(), lse_col.data_ptr(), row.data_ptr(), ws.data_ptr(),
                     stream_ptr(q.device))
        out = torch.empty((), dtype=torch.float32, device=q.device)
        ops.total(row, 1.0, out)
        ctx.save = (qn, qn32, qnorm, dn, dn32, dnorm, lse_row, lse_col)
        ctx.gids = gids
        ctx.cfg = (inv_tau, eps, do_norm, dt)
        return out

    @staticmethod
    def backward(ctx, gout):
        qn, qn32, qnorm, dn, dn32, dnorm, lse_row, lse_col = ctx.save
        inv_tau, eps, do_norm, dt = ctx.cfg
        B, h = qn.shape
        gdev = gout.detach().float().reshape(1).contiguous()  # read by the kernels: no host sync
        dqn = torch.empty(B, h, dtype=torch.float32, device=qn.device)
        ddn = torch.empty(B, h, dtype=torch.float32, device=qn.device)
        lib = _lib.load()
        ws = torch.empty(lib.tt_infonce_sym_bwd_ws_size(dtype_code(dt), B, h), dtype=torch.uint8, device=qn.device)
        if ctx.gids is None:
            call("tt_infonce_sym_bwd", dtype_code(dt), qn.data_ptr(), dn.data_ptr(), B, h, inv_tau,
                 lse_row.data_ptr(), lse_col.data_ptr(), gdev.data_ptr(), dqn.data_ptr(), ddn.data_ptr(),
                 ws.data_ptr(), stream_ptr(qn.device))
        else:
            call("tt_infonce_sym_bwd_grp", dtype_code(dt), qn.data_ptr(), dn.data_ptr(), B, h, inv_tau,
                 ctx.gids.data_ptr(), lse_row.data_ptr(), lse_col.data_ptr(), gdev.data_ptr(), dqn.data_ptr(),
                 ddn.data_ptr(), ws.data_ptr(), stream_ptr(qn.device))
        if do_norm:
            dq = ops.l2norm_bwd(dqn, qn32, qnorm, eps)
            dd = ops.l2norm_bwd(ddn, dn32, dnorm, eps)
        else:
            dq, dd = dqn, ddn
        return dq, dd, None, None, None, None, None


class SymmetricInfoNCELoss(nn.Module):
    """simple_two_tower.py:68-78: (CE(S, arange) + CE(S^T, arange)) / 2 with S = q·dᵀ /
    temperature (the CLIP-style symmetric contrastive loss). The reference's inputs are
    already normalised, so normalize defaults to False; True normalises first (tt_l2norm).
    One process: both directions from one score pass (tt_infonce_sym_fwd/_bwd). With a
    process group of world > 1: the exact composition of the one-directional kernels,
    (CE(q, gather(d)) + CE(d, gather(q))) / 2 over the global batch."""

    def __init__(self, temperature=0.1, normalize=False, compute_dtype=None, process_group=None):
        super().__init__()
        self.temperature = temperature
        self.normalize = normalize
        self.compute_dtype = compute_dtype
        self.process_group = process_group

    def forward(self, query_vec, doc_vec, groups=None):
        dt = _dt_of(query_vec, self.compute_dtype)
        inv_tau = 1.0 / self.temperature
        B = query_vec.shape[0]
        # one id vector serves both directions: excl(i, j) is symmetric in i and j
        extra = () if groups is None else (_group_ids(groups, B, query_vec.device),)
        if not dist.active(self.process_group):
            return _SymCE.apply(query_vec, doc_vec, inv_tau, 1e-12, bool(self.normalize), dt, *extra) / B
        _, world = dist.rank_world(self.process_group)
        g = self.process_group
        s = 0.5 * (_NormCE.apply(query_vec, doc_vec, inv_tau, 0.0, 1e-12, bool(self.normalize), dt, g, *extra)
                   + _NormCE.apply(doc_vec, query_vec, inv_tau, 0.0, 1e-12, bool(self.normalize), dt, g, *extra))
        return _finish_loss(s, 1.0 / (B * world), g)


class _MarginFn(torch.autograd.Function):
    """sum_i relu(margin - cos(q_i, dpool[lab_i]) + mean_j cos(q_i, dpool[idx_ij]))."""

    @staticmethod
    def forward(ctx, q, dpool, idx, label_offset, margin, eps):
        _lib.require_gpu(q, dpool)
        q = q.float().contiguous()
        dpool = dpool.float().contiguous()
        qn, _, qnorm = ops.l2norm_fwd(q, eps, torch.float32)
        dn, _, dnorm = ops.l2norm_fwd(dpool, eps, torch.float32)
        B, h = q.shape
        k = idx.shape[1]
        row = torch.empty(B, dtype=torch.float32, device=q.device)
        call("tt_margin_fwd", qn.data_ptr(), B, dn.data_ptr(), dn.shape[0], h, label_offset, idx.data_ptr(), k,
             margin, row.data_ptr(), stream_ptr(q.device))
        out = torch.empty((), dtype=torch.float32, device=q.device)
        ops.total(row, 1.0, out)
        ctx.save = (qn, qnorm, dn, dnorm, idx)
        ctx.cfg = (label_offset, margin, eps)
        return out

    @staticmethod
    def backward(ctx, gout):
        qn, qnorm, dn, dnorm, idx = ctx.save
        label_offset, margin, eps = ctx.cfg
        B, h = qn.shape
        dqn = torch.empty_like(qn)
        ddn = torch.zeros_like(dn)
        ws = torch.empty(_lib.load().tt_margin_bwd_ws_size(B, dn.shape[0], h, idx.shape[1]), dtype=torch.uint8, device=qn.device)
        gdev = gout.detach().float().reshape(1).contiguous()  # read by the kernels: no host sync
        call("tt_margin_bwd", qn.data_ptr(), B, dn.data_ptr(), dn.shape[0], h, label_offset, idx.data_ptr(),
             idx.shape[1], margin, gdev.data_ptr(), dqn.data_ptr(), ddn.data_ptr(), ws.data_ptr(),
             stream_ptr(qn.device))
        return ops.l2norm_bwd(dqn, qn, qnorm, eps), ops.l2norm_bwd(ddn, dn, dnorm, eps), None, None, None, None


class MarginRankingLoss(nn.Module):
    """enhanced_two_tower.py:84-121.
    neg_doc_vec None: in-batch CE over q·dᵀ/τ (un-normalised) minus margin off the diagonal.
    neg_doc_vec [B*k, h] (query-major): mean(relu(margin - cos(q,pos) + mean_k cos(q,neg)))."""

    def __init__(self, margin=0.2, temperature=0.1, compute_dtype=None, process_group=None):
        super().__init__()
        self.margin = margin
        self.temperature = temperature
        self.compute_dtype = compute_dtype
        self.process_group = process_group

    def forward(self, query_vec, pos_doc_vec, neg_doc_vec=None, *, groups=None):
        B = query_vec.shape[0]
        if neg_doc_vec is None:
            dt = _dt_of(query_vec, self.compute_dtype)
            _, world = dist.rank_world(self.process_group)
            extra = () if groups is None else (_group_ids(groups, B, query_vec.device),)
            s = _NormCE.apply(query_vec, pos_doc_vec, 1.0 / self.temperature, self.margin, 0.0, False, dt,
                              self.process_group, *extra)
            return _finish_loss(s, 1.0 / (B * world), self.process_group)
        if groups is not None:
            raise _lib.TTError("MarginRankingLoss: groups mask in-batch negatives; with explicit negatives "
                               "(neg_doc_vec) there is nothing for them to mask")
        k = neg_doc_vec.shape[0] // B
        pool = torch.cat([pos_doc_vec, neg_doc_vec], 0)
        idx = (B + torch.arange(B * k, device=query_vec.device, dtype=torch.int32)).view(B, k).contiguous()
        s = _MarginFn.apply(query_vec, pool, idx, 0, self.margin, 1e-8)
        return s / B


MINE_SCAN_K = 16  # ttk::SK_MAX: above it tt_hardneg_topk stores the score block for every shape


def _largest_group(col_groups: torch.Tensor) -> int:
    """Size of the largest group among the ids >= 0 (1 when there is none). One host sync."""
    ids = col_groups[col_groups >= 0]
    if ids.numel() == 0:
        return 1
    return int(torch.unique(ids, return_counts=True)[1].max().item())


def mine_hard_negatives(query_vecs: torch.Tensor, doc_vecs: torch.Tensor, label_offset: int = 0, k: int = 5,
                        compute_dtype=torch.float32, eps: float = 1e-8, return_values: bool = False,
                        row_groups=None, col_groups=None, max_group_size=None):
    """Batched get_hard_negatives: for row i the positive is doc label_offset + i (masked
    to -1; label_offset < 0 masks nothing). Returns int32 [B, k] sorted by descending
    cosine, ties towards the lower doc index. 1 <= k <= min(tt_topk_max() = 1024, docs);
    above MINE_SCAN_K the scores are stored and radix-selected (tt_topk_rows), at most
    1 GiB of score block per call.

    row_groups [B] / col_groups [docs] (integer ids, both or neither): a column the group rule
    excludes for a row (module docstring) is never returned. The call mines k + g with the
    ungrouped path, g = max_group_size - 1 (the label column is expected to carry its row's
    id, as it does with one id per pair; with label_offset < 0, g = max_group_size), and
    tt_topk_drop_groups keeps the first k allowed: a row has at most g excluded columns, so
    these are the exact top k of the allowed columns. max_group_size is the caller's promise
    of the largest number of columns that share one id >= 0; None computes it from
    col_groups, which costs one host sync per call. k + g <= min(tt_topk_max(), docs), else
    TTError; k + g > MINE_SCAN_K leaves the streamed scan for the stored-score path."""
    _lib.require_gpu(query_vecs, doc_vecs)
    lib = _lib.load()
    B, nd = query_vecs.shape[0], doc_vecs.shape[0]
    if row_groups is not None or col_groups is not None:
        if row_groups is None or col_groups is None:
            raise _lib.TTError("mine_hard_negatives: row_groups and col_groups go together")
        rg = _group_ids(row_groups, B, query_vecs.device)
        cg = _group_ids(col_groups, nd, query_vecs.device)
        mgs = _largest_group(cg) if max_group_size is None else int(max_group_size)
        if mgs < 1:
            raise _lib.TTError(f"mine_hard_negatives: max_group_size={mgs} must be >= 1")
        g = mgs - 1 if label_offset >= 0 else mgs
        kin = k + g
        if not 1 <= k or kin > min(_lib.topk_max(), nd):
            raise _lib.TTError(f"mine_hard_negatives: k={k} + g={g} (max_group_size {mgs}) = {kin} needs "
                               f"1 <= k and k + g <= min({_lib.topk_max()}, {nd} docs)")
        cand = mine_hard_negatives(query_vecs, doc_vecs, label_offset, kin, compute_dtype, eps, return_values)
        cidx, cval = cand if return_values else (cand, None)
        idx = torch.empty(B, k, dtype=torch.int32, device=cidx.device)
        val = torch.empty(B, k, dtype=torch.float32, device=cidx.device) if return_values else None
        call("tt_topk_drop_groups", cidx.data_ptr(), ptr(cval), B, kin, label_offset, rg.data_ptr(), cg.data_ptr(),
             nd, k, idx.data_ptr(), ptr(val), None, stream_ptr(cidx.device))
        return (idx, val) if return_values else idx
    if not 1 <= k <= min(_lib.topk_max(), nd):
        raise _lib.TTError(f"mine_hard_negatives: k={k} needs 1 <= k <= min({_lib.topk_max()}, {nd} docs)")
    # rows per call: all of them, or for k > MINE_SCAN_K what keeps the score block within 1 GiB
    step = max(B, 1) if k <= MINE_SCAN_K else max(1, min(B, (1 << 28) // nd))
    with torch.no_grad():
        qn, _, _ = ops.l2norm_fwd(query_vecs.float().contiguous(), eps, compute_dtype, want_f32=False)
        dn, _, _ = ops.l2norm_fwd(doc_vecs.float().contiguous(), eps, compute_dtype, want_f32=False)
        h = qn.shape[1]
        idx = torch.empty(B, k, dtype=torch.int32, device=qn.device)
        val = torch.empty(B, k, dtype=torch.float32, device=qn.device) if return_values else None
        esz = 2 if compute_dtype == torch.bfloat16 else 4
        dc = dtype_code(compute_dtype)
        for r0 in range(0, B, step):
            n = min(B, r0 + step) - r0
            ws = torch.empty(lib.tt_hardneg_ws_size(dc, n, nd, h, k), dtype=torch.uint8, device=qn.device)
            with timing.region("hardneg_topk", 1, 2.0 * n * nd * h, float(esz * (n + nd) * h + n * k * 4)):
                call("tt_hardneg_topk", dc, qn[r0:].data_ptr(), n, dn.data_ptr(), nd, h,
                     label_offset + r0 if label_offset >= 0 else label_offset, k, idx[r0:].data_ptr(),
                     ptr(val[r0:]) if return_values else None, ws.data_ptr(), stream_ptr(qn.device))
    return (idx, val) if return_values else idx


def get_hard_negatives(query_vec, doc_vecs, positive_idx, k=5):
    """enhanced_two_tower.py:123-133 (one query). Returns int64 indices [k]."""
    idx = mine_hard_negatives(query_vec.reshape(1, -1), doc_vecs, int(positive_idx), k)
    return idx[0].long()


class HardNegativeMarginLoss(nn.Module):
    """Config 3 of BASELINE.json: per query, mine k hard negatives among all (global)
    docs with the positive masked, then MarginRankingLoss(margin) with those negatives.
    Equivalent to the reference composition
        idx_i = get_hard_negatives(q_i, d, i, k); MarginRankingLoss()(q, d, d[cat idx])."""

    def __init__(self, k=5, margin=0.2, compute_dtype=None, process_group=None, max_group_size=None):
        super().__init__()
        self.k = k
        self.margin = margin
        self.compute_dtype = compute_dtype
        self.process_group = process_group
        self.max_group_size = max_group_size  # of the gathered pool (mine_hard_negatives); None: one sync a step
        self.last_indices = None

    def forward(self, query_vec, doc_vec, groups=None):
        dt = _dt_of(query_vec, self.compute_dtype)
        rank, world = dist.rank_world(self.process_group)
        B = query_vec.shape[0]
        pool = dist.GatherRows.apply(doc_vec.float().contiguous(), self.process_group) if world > 1 else doc_vec
        if groups is None:
            idx = mine_hard_negatives(query_vec.detach(), pool.detach(), rank * B, self.k, dt)
        else:
            gids = _group_ids(groups, B, query_vec.device)
            idx = mine_hard_negatives(query_vec.detach(), pool.detach(), rank * B, self.k, dt, row_groups=gids,
                                      col_groups=dist.all_gather_rows(gids, self.process_group),
                                      max_group_size=self.max_group_size)
        self.last_indices = idx
        s = _MarginFn.apply(query_vec, pool, idx, rank * B, self.margin, 1e-8)
        return _finish_loss(s, 1.0 / (B * world), self.process_group)
