"""Float64 restatements of the loss kernels and of the small row helpers around them, and
the comparison functions their tests share -- TEST INFRASTRUCTURE ONLY.

Written from the formulas in include/tt_hip.h (tt_infonce_fwd / _bwd, tt_l2norm_fwd / _bwd,
tt_margin_fwd, tt_colsum, tt_sum, tt_cast, tt_pack_rows), not from the kernels: plain torch,
nothing read from outside the repository. Every reference takes its operands as the kernel
sees them (already rounded to the storage dtype) and computes in float64 on the operands'
device, so the large cases can run where the data is.
tests/test_loss_ref_host.py pins the references against torch autograd and shows that each
comparison function below rejects a reference with one planted defect;
tests/test_gpu_infonce_ref.py and tests/test_gpu_rowops_ref.py compare the HIP kernels with
them through the same comparison functions.

Comparison functions return lists of (name, error, index, bound); check() prints the worst
and asserts error <= bound for each.
"""
from __future__ import annotations

import torch

from oracle.gru_ref import row_err, vec_err  # noqa: F401  (re-exported for the tests)

F32, BF16 = torch.float32, torch.bfloat16
TOL_ROW_F32 = 1e-4  # the project's per-row fp32 tolerance (tests/test_gpu_gru_ref.py)


# ------------------------------------------------------------------------- InfoNCE
def infonce_scores(q, d, inv_tau, offdiag, label_offset):
    """S = inv_tau q d^T - offdiag [j != label_i], label_i = label_offset + i. float64."""
    s = inv_tau * (q.double() @ d.double().t())
    rows = torch.arange(q.shape[0], device=q.device)
    lab = s[rows, label_offset + rows].clone()
    s -= offdiag
    s[rows, label_offset + rows] = lab
    return s


def infonce_fwd_ref(q, d, inv_tau, offdiag, label_offset):
    """lse [bq] and row_loss [bq] = lse - S[i][label_i] alone (the large forward case)."""
    s = infonce_scores(q, d, inv_tau, offdiag, label_offset)
    rows = torch.arange(q.shape[0], device=q.device)
    lse = torch.logsumexp(s, dim=1)
    return lse, lse - s[rows, label_offset + rows]


def infonce_ref(q, d, inv_tau, offdiag, label_offset, g, ds_dtype=None):
    """lse [bq], row_loss [bq] = lse - S[i][label_i], and the gradient of g * sum(row_loss):
    dS = g (softmax(S) - onehot(label)), dq = inv_tau dS d, dd = inv_tau dS^T q.
    ds_dtype = torch.bfloat16 rounds dS to bf16 before the two products, the rounding both
    bf16 backward paths perform on their MFMA operand; it serves only to size the bf16
    backward tolerance (bwd_row_bound)."""
    s = infonce_scores(q, d, inv_tau, offdiag, label_offset)
    rows = torch.arange(q.shape[0], device=q.device)
    lse = torch.logsumexp(s, dim=1)
    row_loss = lse - s[rows, label_offset + rows]
    ds = torch.softmax(s, dim=1)
    del s
    ds[rows, label_offset + rows] -= 1.0
    ds *= g
    if ds_dtype is not None:
        ds = ds.to(ds_dtype).double()
    dq = inv_tau * (ds @ d.double())
    dd = inv_tau * (ds.t() @ q.double())
    return lse, row_loss, dq, dd


def _abs_excess(got, ref, bound):
    """(worst |got - ref| / bound, index); bound a float or a per-row tensor. NaN / inf in got
    counts as infinite."""
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    bound = torch.as_tensor(bound, dtype=torch.float64).cpu().expand_as(ref)
    e = torch.nan_to_num((got - ref).abs(), nan=float("inf"), posinf=float("inf")) / bound
    k = int(e.argmax())
    return float(e[k]), (k,)


def infonce_fwd_errs(lse, row_loss, ref_lse, ref_row, dt, smax=None):
    """The forward bounds, per row, as error / bound (so every entry's bound is 1):
      bf16  |lse - ref| <= 1e-5 max|ref lse| + 2e-4,  |row_loss - ref| <= 2e-4
            (tests/test_gpu_infonce_bwd.py)
      fp32  |x - ref| <= 1e-4 |ref| + 1e-5            (tests/test_gpu_infonce_sym.py)
    smax: per-row max_j |S_ij| for un-normalised inputs; the absolute terms (2e-4, 1e-5), which
    were set for scores of size inv_tau * cosine, then scale with it (never below 1)."""
    ref_lse = ref_lse.detach().double().cpu()
    ref_row = ref_row.detach().double().cpu()
    scale = torch.ones_like(ref_lse) if smax is None else smax.detach().double().cpu().clamp(min=1.0)
    if dt == BF16:
        b_lse = 1e-5 * float(ref_lse.abs().max()) + 2e-4 * scale
        b_row = 2e-4 * scale
    else:
        b_lse = 1e-4 * ref_lse.abs() + 1e-5 * scale
        b_row = 1e-4 * ref_row.abs() + 1e-5 * scale
    return [("lse", *_abs_excess(lse, ref_lse, b_lse), 1.0), ("row_loss", *_abs_excess(row_loss, ref_row, b_row), 1.0)]


def whole_err(got, ref):
    """The whole-tensor measures of tests/test_gpu_infonce_bwd.py: (max-abs error relative to
    the largest reference entry, cosine)."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), 0.0
    err = float((got - ref).abs().max() / ref.abs().max())
    cos = float((got * ref).sum() / (got.norm() * ref.norm()))
    return err, cos


def bwd_row_bound(q, d, inv_tau, offdiag, label_offset, g):
    """The bf16 backward's per-row bounds (for dq, for dd): twice the per-row error (row_err)
    of the reference with dS rounded to bf16 against the unrounded reference. Also returns
    the two references. Nothing here comes from a kernel."""
    _, _, rq, rd = infonce_ref(q, d, inv_tau, offdiag, label_offset, g)
    _, _, bq_, bd_ = infonce_ref(q, d, inv_tau, offdiag, label_offset, g, ds_dtype=BF16)
    return (2.0 * row_err(bq_, rq)[0], 2.0 * row_err(bd_, rd)[0]), (rq, rd)


def infonce_bwd_errs(dq, dd, rq, rd, dt, row_bounds=None):
    """fp32: row_err <= 1e-4. bf16: max-abs <= 1.5e-2 of the largest entry and cosine >= 0.9999
    (the existing whole-tensor bound; the cosine is listed as 1 - cos <= 1e-4), and row_err <=
    row_bounds (bwd_row_bound)."""
    errs = []
    for name, got, ref, k in (("dq", dq, rq, 0), ("dd", dd, rd, 1)):
        if dt == BF16:
            e, cos = whole_err(got, ref)
            errs += [(name + " max-abs", e, (), 1.5e-2), (name + " 1-cos", 1.0 - cos, (), 1e-4),
                     (name + " per row", *row_err(got, ref), row_bounds[k])]
        else:
            errs.append((name + " per row", *row_err(got, ref), TOL_ROW_F32))
    return errs


# -------------------------------------------------------------------------- l2norm
def l2norm_ref(x, eps):
    """y = x / max(||x||, eps) row-wise, and ||x||. float64."""
    x = x.double()
    norm = x.pow(2).sum(1).sqrt()
    return x / norm.clamp(min=eps).unsqueeze(1), norm


def l2norm_bwd_ref(dy, y, norm, eps):
    """torch's gradient of l2norm_ref at the point (y, norm): (dy - y (y . dy)) / norm where
    norm > eps; where the clamp is active it passes no gradient to the norm: dy / eps."""
    dy, y, norm = dy.double(), y.double(), norm.double().unsqueeze(1)
    free = (dy - y * (y * dy).sum(1, keepdim=True)) / norm.clamp(min=eps)
    return torch.where(norm > eps, free, dy / eps)


def l2norm_fwd_errs(y32, norm, x, eps):
    """norm: 1e-5 relative (the kernel's summation, 16 sequential terms per lane, a 6-level
    wave tree and one sqrt, is bounded near 24 x 2^-24 = 1.4e-6; a dropped column of 1024
    with |x| in [0.5, 1.5] shifts it by 1.1e-4); y: the per-row fp32 tolerance. A zero
    reference norm must be matched exactly."""
    ry, rn = l2norm_ref(x, eps)
    return [("norm", *_abs_excess(norm, rn, (1e-5 * rn.abs()).clamp(min=1e-300)), 1.0),
            ("y", *row_err(y32, ry), TOL_ROW_F32)]


def l2norm_bwd_errs(dx, dy, y32, norm, eps):
    """dx against l2norm_bwd_ref at the kernel's own y32 and norm, per row:
        err[row] = max_j |dx - ref| / max(max_j |ref|, max_j |dy| / max(norm, eps)).
    Every row has a scale of its own (a clamped row's dy / eps is 1e12 times a free row's
    entries at the default eps), and it is never smaller than that of the two terms of
    (dy - y (y . dy)) / norm: with one column the terms cancel, the gradient is 0 up to the
    rounding of y, and the difference has no scale of its own. NaN / inf counts as infinite."""
    ref = l2norm_bwd_ref(dy, y32, norm, eps).cpu()
    dx = dx.detach().double().cpu()
    term = dy.detach().double().cpu().abs().amax(1) / norm.detach().double().cpu().clamp(min=eps)
    scale = torch.maximum(ref.abs().amax(1), term).clamp(min=1e-300)
    e = torch.nan_to_num((dx - ref).abs(), nan=float("inf"), posinf=float("inf")) / scale.unsqueeze(1)
    k = int(e.reshape(-1).argmax())
    return [("dx", float(e.reshape(-1)[k]), (k // e.shape[1], k % e.shape[1]), TOL_ROW_F32)]


# -------------------------------------------------------------------------- margin
def margin_ref(qn, dn, label_offset, idx, margin):
    """MarginRankingLoss with explicit negatives: pos_i = q_i . d_{label_offset + i}, negm_i the
    mean over the k columns of idx of q_i . d_{idx[i][j]}, row_loss = max(margin - pos + negm, 0)."""
    q, d = qn.double(), dn.double()
    rows = torch.arange(q.shape[0], device=q.device)
    pos = (q * d[label_offset + rows]).sum(1)
    negm = torch.einsum("bh,bkh->bk", q, d[idx.long()]).mean(1)
    return pos, negm, (margin - pos + negm).clamp(min=0.0)


def margin_fwd_errs(row_loss, pos, negm, margin):
    """Absolute 1e-5 (cosines are bounded by 1), and an exact 0.0 wherever the reference hinge
    is inactive by more than that bound."""
    arg = (margin - pos + negm).detach().double().cpu()
    got = row_loss.detach().double().cpu()
    off = arg < -1e-5
    nonzero = off & (got != 0.0)
    n = int(nonzero.sum())
    return [("row_loss", *_abs_excess(got, arg.clamp(min=0.0), 1e-5), 1.0),
            ("inactive rows with a loss other than 0.0", float(n), (int(nonzero.nonzero()[0]),) if n else (), 0.0)]


# ------------------------------------------------- exact restatements (fp32, on the CPU)
def colsum_order_ref(x, rows, cols, prev=None):
    """tt_colsum bit for bit. x fp32 [>= rows, ld >= cols] on the CPU. Wave w starts from 0 and
    adds rows w, w + 16, ... in order; the 16 wave sums are added to 0 in wave order; the
    optional accumulate then adds that total to the previous contents prev."""
    assert x.dtype == F32 and x.device.type == "cpu"
    waves = []
    for w in range(16):
        s = torch.zeros(cols, dtype=F32)
        for r in range(w, rows, 16):
            s = s + x[r, :cols]
        waves.append(s)
    t = torch.zeros(cols, dtype=F32)
    for s in waves:
        t = t + s
    return t if prev is None else prev + t


def bits_differ(got, ref):
    """(number of elements whose bits differ, index of the first). NaN equals NaN of any
    payload; +0 and -0 differ."""
    got, ref = got.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    it = torch.int16 if got.element_size() == 2 else torch.int32
    bad = (got.view(it) != ref.view(it)) & ~(torch.isnan(got) & torch.isnan(ref))
    n = int(bad.sum())
    return n, ((int(bad.nonzero()[0]),) if n else ())


def colsum_errs(out, x, rows, cols, prev=None):
    """out [cols] against colsum_order_ref (bit for bit) and against float64 within
    rows x 2^-24 x sum_r |x[r][c]| per column (prev included when given): every addition
    rounds once, by at most 2^-24 of a partial sum that sum|x| bounds; the additions to a
    zero are exact, which leaves at most rows - 1 inexact ones per column, plus one for the
    accumulate. rows = 0 must therefore be exact."""
    x = x.detach().cpu()
    n, idx = bits_differ(out, colsum_order_ref(x, rows, cols, prev))
    ref = x[:rows, :cols].double().sum(0)
    mag = x[:rows, :cols].double().abs().sum(0)
    if prev is not None:
        ref, mag = ref + prev.double(), mag + prev.double().abs()
    bound = (rows * 2.0 ** -24 * mag).clamp(min=1e-300)
    return [("bits differing from the stated order", float(n), idx, 0.0), ("vs float64", *_abs_excess(out, ref, bound), 1.0)]


def sum_errs(out, x, scale):
    """tt_sum: within (ceil(n / 256) + 12) x 2^-24 x |scale| x sum|x| of float64: a thread's chain
    of ceil(n / 256) additions, 6 levels of the wave tree, 3 additions of the four wave sums, the
    product with scale, and two for the fp32 rounding of the inputs to those steps."""
    x = x.detach().double().cpu().reshape(-1)
    n = x.numel()
    bound = max((-(-n // 256) + 12) * 2.0 ** -24 * abs(scale) * float(x.abs().sum()), 1e-300)
    return [("sum", *_abs_excess(out.reshape(1), (scale * x.sum()).reshape(1), bound), 1.0)]


def bf16_rne_ref(x):
    """fp32 -> bf16, round to nearest even (torch's .to(torch.bfloat16) is that rounding)."""
    return x.to(BF16)


def pack_rows_ref(src, e, ep, dt):
    """tt_pack_rows: [n, e] fp32 -> [n, ep] dt, columns e.. zero."""
    out = torch.zeros(src.shape[0], ep, dtype=dt)
    out[:, :e] = src.reshape(-1, e).to(dt)
    return out


def cast_errs(got, ref):
    n, idx = bits_differ(got, ref)
    return [("bits differing from round-to-nearest-even", float(n), idx, 0.0)]


def check(what, errs):
    """Print the worst entry (relative to its bound) and assert every error <= its bound."""
    worst = max(errs, key=lambda e: e[1] / e[3] if e[3] > 0 else (float("inf") if e[1] > 0 else 0.0))
    print(f"{what}: worst {worst[0]} {worst[1]:.3g} (bound {worst[3]:.3g}) at {worst[2]}")
    for name, e, idx, bound in errs:
        assert e <= bound, f"{what}: {name} {e:.3g} > {bound:.3g} at {idx}"


# ------------------------------------------------- the cases and inputs of the two test files
INV_TAU = 1 / 0.07

# name: (bq, nd, {dtype: h}, label_offset, offdiag, normalised rows, inv_tau values)
INFONCE_FWD_CASES = {
    "one_row_tail_label": (1, 129, {F32: 4, BF16: 8}, 128, 0.0, True, (1.0, INV_TAU)),
    "second_row_block_k_tail": (130, 300, {F32: 36, BF16: 72}, 170, 0.0, True, (1.0, INV_TAU)),
    "offdiag": (257, 517, {F32: 8, BF16: 8}, 0, 0.2, True, (1.0, INV_TAU)),
    "margin_branch_unnormalised": (257, 517, {F32: 8, BF16: 8}, 0, 0.2, False, (10.0,)),
    "h512": (130, 520, {BF16: 512}, 0, 0.0, True, (1.0, INV_TAU)),
    "short_last_split": (1100, 14853, {F32: 8, BF16: 8}, 13753, 0.0, True, (INV_TAU,)),
}

# (dtype, bq, nd, h, label_offset, offdiag, infonce_flash values)
INFONCE_BWD_CASES = [
    (F32, 1, 129, 4, 128, 0.0, (1,)),
    (F32, 130, 300, 36, 170, 0.0, (1,)),
    (F32, 257, 517, 8, 0, 0.2, (1,)),
    (F32, 257, 1001, 32, 744, 0.0, (1,)),
    (BF16, 1, 129, 8, 128, 0.0, (1,)),
    (BF16, 130, 300, 72, 170, 0.0, (1,)),
    (BF16, 257, 517, 8, 0, 0.2, (1,)),
    (BF16, 130, 520, 512, 0, 0.0, (1,)),
    (BF16, 1, 129, 128, 128, 0.0, (1, 0)),
    (BF16, 40, 40, 256, 0, 0.0, (1, 0)),
]


def infonce_inputs(bq, nd, h, dt, normalised=True):
    """q [bq, h] and d [nd, h] rounded to dt (and held in dt), from a seed of the shape."""
    gen = torch.Generator().manual_seed(bq + 7 * nd + 31 * h)
    q, d = torch.randn(bq, h, generator=gen), torch.randn(nd, h, generator=gen)
    if normalised:
        q, d = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(d, dim=1)
    return q.to(dt), d.to(dt)


L2NORM_ROWS = (1, 5, 130)
L2NORM_COLS = (1, 8, 63, 64, 65, 200, 1024)


def l2norm_inputs(rows, cols, zero_row=True):
    """x fp32 with |x| in [0.5, 1.5] and random signs, so every column carries weight in the
    norm; dy and a previous dx for the accumulate. Row rows - 1 is all zero (zero_row)."""
    gen = torch.Generator().manual_seed(1000 * rows + cols)
    mag = 0.5 + torch.rand(rows, cols, generator=gen)
    x = mag * (torch.randint(0, 2, (rows, cols), generator=gen) * 2 - 1)
    if zero_row:
        x[rows - 1] = 0.0
    return x, torch.randn(rows, cols, generator=gen), torch.randn(rows, cols, generator=gen)


def l2norm_clamped_inputs(rows=5, cols=200):
    """Rows of norm 0.1 for eps = 0.5: the clamped branch on ordinary numbers."""
    x, dy, prev = l2norm_inputs(rows, cols, zero_row=False)
    return 0.1 * x / x.norm(dim=1, keepdim=True), dy, prev


COLSUM_ROWS = (0, 1, 15, 16, 17, 300)
COLSUM_COLS = (1, 63, 64, 65, 3072)


def colsum_inputs(rows, cols):
    """x [max(rows, 1), ld = cols + 5] fp32 (the columns after cols are never to be read into
    the result) and the previous contents of out for the accumulate."""
    gen = torch.Generator().manual_seed(100 * rows + cols)
    return torch.randn(max(rows, 1), cols + 5, generator=gen), torch.randn(cols, generator=gen)


def cast_inputs(n):
    """fp32 values for the casts: the edge values first (exact ties both ways, +-0, fp32 and
    bf16 denormals, infinities, the largest finite values that round up to infinity, NaN),
    then normal values over many binades."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,  # ties to even: down, up
            0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807F8000,
            0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7FC00000, 0xFFC00001]
    edge = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(F32)
    gen = torch.Generator().manual_seed(n)
    body = torch.randn(max(n - edge.numel(), 0), generator=gen) * torch.exp2(
        torch.randint(-40, 40, (max(n - edge.numel(), 0),), generator=gen).float())
    return torch.cat([edge, body])[:n].contiguous()


def truncate_to_bf16(x):
    """The planted defect of the cast's sensitivity check: drop the low 16 bits."""
    return (x.view(torch.int32) & -65536).view(F32).to(BF16)


def margin_inputs(bq, nd, h, k, label_offset):
    """Normalised fp32 rows; idx [bq, k] int32 negatives with repeats inside and across rows.
    Row 0's negatives all equal its positive (loss = margin); the documents of rows 1 and 2
    are copies of their queries, so with distinct negatives their hinge is inactive."""
    gen = torch.Generator().manual_seed(bq + 3 * nd + 5 * h + 7 * k)
    q = torch.nn.functional.normalize(torch.randn(bq, h, generator=gen), dim=1)
    d = torch.nn.functional.normalize(torch.randn(nd, h, generator=gen), dim=1)
    idx = torch.randint(0, min(nd, 6), (bq, k), generator=gen, dtype=torch.int32)
    idx[0] = label_offset
    for r in (1, 2):
        d[label_offset + r] = q[r]
    return q.contiguous(), d.contiguous(), idx.contiguous()
