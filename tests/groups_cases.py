"""Cases, group patterns and the masked float64 references shared by the group-mask tests
(test_groups_host.py, test_gpu_groups_ref.py, test_gpu_groups.py) -- TEST INFRASTRUCTURE ONLY.

The group rule (include/tt_hip.h): column j is excluded for row i iff j != label_offset + i,
row_group[i] >= 0 and col_group[j] == row_group[i]. The references are infonce_ref of
oracle/loss_ref.py with S.masked_fill(excl, -inf) in front: an excluded entry adds nothing to
the log-sum-exp and its dS is 0. mask=False gives the unmasked reference, the planted defect
of the yardstick tests (a kernel that ignores the ids).

Everything here is computed on the CPU from the operands, never from a kernel's output, and
cached: a case's reference is computed once and left unchanged.
"""
import functools

import torch

from oracle import loss_ref as L
from oracle.loss_ref import BF16, F32, INV_TAU


# ------------------------------------------------------------------------ group patterns
def groups_threes(bq, nd, lab0):
    """130 x 300, label_offset 170: rows i < 120 in groups of three (i // 3), the rest -1;
    col_group[170 + i] = row_group[i], and col_group[j] = row_group[j] for j < 60, so a row's
    excluded columns also lie in a column tile and split other than its label's."""
    rg = torch.full((bq,), -1, dtype=torch.int32)
    rg[:120] = torch.arange(120, dtype=torch.int32) // 3
    cg = torch.full((nd,), -1, dtype=torch.int32)
    cg[lab0:lab0 + bq] = rg
    cg[:60] = rg[:60]
    return rg, cg


def groups_all_one(bq, nd, lab0):
    """1 x 129, label 128: every column carries the row's id, so all but the label is
    excluded and split 0 (columns 0..127) is excluded as a whole."""
    return torch.zeros(bq, dtype=torch.int32), torch.zeros(nd, dtype=torch.int32)


def groups_block_apart(bq, nd, lab0):
    """257 x 517, label_offset 0: groups of two (i, i + 128), mates one row block apart."""
    rg = torch.full((bq,), -1, dtype=torch.int32)
    rg[:256] = torch.arange(256, dtype=torch.int32) % 128
    cg = torch.full((nd,), -1, dtype=torch.int32)
    cg[:bq] = rg
    return rg, cg


def groups_tiles_apart(n, nd=None, lab0=0):
    """200 x 200: groups (i, i + 64) for i < 32 and (i, i + 128) for 32 <= i < 64: a mate lies
    in another 64-row swept tile and, for the second kind, in another 128-row own block, for
    both roles of the fused backward. Everything else is -1."""
    g = torch.full((n,), -1, dtype=torch.int32)
    i = torch.arange(32, dtype=torch.int32)
    g[:32], g[64:96] = i, i
    g[32:64], g[160:192] = 32 + i, 32 + i
    return g, g.clone()


def groups_pairs(n, nd=None, lab0=0):
    """groups of two neighbours (i // 2)."""
    g = (torch.arange(n) // 2).to(torch.int32)
    return g, g.clone()


# name: (bq, nd, {dtype: h}, label_offset, offdiag, normalised rows, inv_tau values, pattern)
FWD_CASES = {
    "threes_other_tile": (130, 300, {F32: 36, BF16: 72}, 170, 0.0, True, (1.0, INV_TAU), groups_threes),
    "all_but_label_excluded": (1, 129, {F32: 4, BF16: 8}, 128, 0.0, True, (1.0, INV_TAU), groups_all_one),
    "margin_branch_block_apart": (257, 517, {F32: 8, BF16: 8}, 0, 0.2, False, (10.0,), groups_block_apart),
}

# (dtype, bq, nd, h, label_offset, offdiag, infonce_flash values, pattern); inv_tau = 1 / 0.07
BWD_CASES = [
    (F32, 130, 300, 36, 170, 0.0, (1,), groups_threes),
    (BF16, 130, 300, 72, 170, 0.0, (1,), groups_threes),
    (BF16, 200, 200, 128, 0, 0.0, (1, 0), groups_tiles_apart),
    (BF16, 40, 40, 256, 0, 0.0, (1, 0), groups_pairs),
]

SYM_INV_TAU = 10.0
SYM_CASES = [(F32, 200, 36, (1,)), (BF16, 200, 128, (1, 0))]  # dtype, n, h, infonce_flash values


# ---------------------------------------------------------------------------- references
def excluded(bq, nd, lab0, rg, cg):
    """The rule as a bool matrix [bq, nd]."""
    rg, cg = rg.long(), cg.long()
    e = (rg[:, None] >= 0) & (cg[None, :] == rg[:, None])
    rows = torch.arange(bq)
    e[rows, lab0 + rows] = False
    return e


def masked_scores(q, d, inv_tau, offdiag, lab0, rg, cg, mask=True):
    s = L.infonce_scores(q, d, inv_tau, offdiag, lab0)
    if mask:
        s = s.masked_fill(excluded(q.shape[0], d.shape[0], lab0, rg, cg), float("-inf"))
    return s


def masked_ref(q, d, inv_tau, offdiag, lab0, g, rg, cg, ds_dtype=None, mask=True):
    """infonce_ref (oracle/loss_ref.py) over the masked scores: lse, row_loss, dq, dd."""
    s = masked_scores(q, d, inv_tau, offdiag, lab0, rg, cg, mask)
    rows = torch.arange(q.shape[0])
    lse = torch.logsumexp(s, dim=1)
    row_loss = lse - s[rows, lab0 + rows]
    ds = torch.softmax(s, dim=1)  # exp(-inf) = 0: an excluded dS is exactly 0
    ds[rows, lab0 + rows] -= 1.0
    ds *= g
    if ds_dtype is not None:
        ds = ds.to(ds_dtype).double()
    return lse, row_loss, inv_tau * (ds @ d.double()), inv_tau * (ds.t() @ q.double())


def masked_bwd_bound(q, d, inv_tau, offdiag, lab0, g, rg, cg):
    """bwd_row_bound (oracle/loss_ref.py) for the masked reference: twice the per-row error of
    the reference with dS rounded to bf16 against the unrounded one."""
    _, _, rq, rd = masked_ref(q, d, inv_tau, offdiag, lab0, g, rg, cg)
    _, _, bq_, bd_ = masked_ref(q, d, inv_tau, offdiag, lab0, g, rg, cg, ds_dtype=BF16)
    return (2.0 * L.row_err(bq_, rq)[0], 2.0 * L.row_err(bd_, rd)[0])


def masked_sym_ref(q, d, inv_tau, g, grp, ds_dtype=None, mask=True):
    """The symmetric loss (tt_infonce_sym_fwd / _bwd in include/tt_hip.h) over the masked
    square S: lse_row, lse_col, row_loss, dq, dd."""
    n = q.shape[0]
    s = masked_scores(q, d, inv_tau, 0.0, 0, grp, grp, mask)
    lr, lc = torch.logsumexp(s, dim=1), torch.logsumexp(s, dim=0)
    diag = s.diagonal()
    row = 0.5 * ((lr - diag) + (lc - diag))
    ds = 0.5 * g * (torch.softmax(s, dim=1) + torch.softmax(s, dim=0) - 2.0 * torch.eye(n, dtype=torch.float64))
    if ds_dtype is not None:
        ds = ds.to(ds_dtype).double()
    return lr, lc, row, inv_tau * (ds @ d.double()), inv_tau * (ds.t() @ q.double())


def masked_sym_bound(q, d, inv_tau, g, grp):
    r = masked_sym_ref(q, d, inv_tau, g, grp)
    b = masked_sym_ref(q, d, inv_tau, g, grp, ds_dtype=BF16)
    return (2.0 * L.row_err(b[3], r[3])[0], 2.0 * L.row_err(b[4], r[4])[0])


# ------------------------------------------------------------------------- cached cases
@functools.lru_cache(maxsize=None)
def fwd_case(name, dt):
    """q, d, rg, cg and per inv_tau: (masked lse, masked row_loss, unmasked lse, unmasked
    row_loss, smax). smax (un-normalised inputs only): per-row max |S| over the allowed
    columns, the scale of the absolute terms in infonce_fwd_errs."""
    bq, nd, hs, lab0, offdiag, normalised, taus, pattern = FWD_CASES[name]
    q, d = L.infonce_inputs(bq, nd, hs[dt], dt, normalised)
    rg, cg = pattern(bq, nd, lab0)
    per_tau = {}
    for inv_tau in taus:
        s = masked_scores(q, d, inv_tau, offdiag, lab0, rg, cg)
        rows = torch.arange(bq)
        lse = torch.logsumexp(s, dim=1)
        su = L.infonce_scores(q, d, inv_tau, offdiag, lab0)
        ulse = torch.logsumexp(su, dim=1)
        smax = None if normalised else s.masked_fill(torch.isinf(s), 0.0).abs().amax(1)
        per_tau[inv_tau] = (lse, lse - s[rows, lab0 + rows], ulse, ulse - su[rows, lab0 + rows], smax)
    return q, d, rg, cg, per_tau


@functools.lru_cache(maxsize=None)
def bwd_case(dt, bq, nd, h, lab0, offdiag, pattern):
    """q, d, rg, cg, g, the fp32 lse handed to the kernel, the masked references rq, rd, the
    bf16 per-row bounds, and the unmasked references uq, ud."""
    q, d = L.infonce_inputs(bq, nd, h, dt)
    rg, cg = pattern(bq, nd, lab0)
    g = 1.0 / bq
    lse, _, rq, rd = masked_ref(q, d, INV_TAU, offdiag, lab0, g, rg, cg)
    bounds = masked_bwd_bound(q, d, INV_TAU, offdiag, lab0, g, rg, cg)
    _, _, uq, ud = masked_ref(q, d, INV_TAU, offdiag, lab0, g, rg, cg, mask=False)
    return q, d, rg, cg, g, lse.float(), rq, rd, bounds, uq, ud


@functools.lru_cache(maxsize=None)
def sym_case(dt, n, h):
    """q, d, grp, g, the masked references (lse_row, lse_col, row_loss, dq, dd), the bf16
    per-row bounds and the unmasked references."""
    q, d = L.infonce_inputs(n, n, h, dt)
    grp, _ = groups_tiles_apart(n)
    g = 1.0 / n
    return (q, d, grp, g, masked_sym_ref(q, d, SYM_INV_TAU, g, grp), masked_sym_bound(q, d, SYM_INV_TAU, g, grp),
            masked_sym_ref(q, d, SYM_INV_TAU, g, grp, mask=False))
