"""The float64 loss references (oracle/loss_ref.py) and their comparison functions, on the CPU.

1. The references agree with torch autograd in float64: F.cross_entropy on the shifted scores,
   F.normalize (free, clamped and all-zero rows), and the reference rule of MarginRankingLoss
   with explicit negatives; the exact restatements agree with their definitions.
2. Sensitivity, one check per case family of tests/test_gpu_infonce_ref.py and
   tests/test_gpu_rowops_ref.py: the family's own inputs, the comparison function the GPU test
   uses, the reference with ONE planted defect in place of the kernel's output; the comparison
   must fail. The correct reference rounded to fp32 must pass the same comparison. Defects:
     - one column dropped from one row's log-sum-exp: the column with the smallest weight, in
       the row where that weight is smallest over the whole case, at inv_tau = 1 (every forward
       case with nd <= 1000 and normalised rows, fp32 and bf16). The shift, as a multiple of the
       bound of infonce_fwd_errs, is printed. Smallest: bf16 2.62 (257 x 517 x 8), fp32 1.10
       (the same case: the fp32 bound's relative term 1e-4 |lse| is 6e-4 there, larger than
       the bf16 bound); the other cases read 2.95 to 13.7.
     - one column dropped from one row's norm (the smallest |x| of 1024 columns: 1.1e-4
       relative against the bound 1e-5);
     - one row left out of a column sum;
     - truncation instead of round-to-nearest-even in a cast;
     - the clamped l2norm backward replaced by the unclamped formula;
     - one row's dS column dropped from the InfoNCE backward (fp32 and bf16 bounds).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import loss_ref as L
from oracle.loss_ref import BF16, F32

SMALL_FWD = [(name, dt) for name, c in L.INFONCE_FWD_CASES.items() for dt in c[2] if c[1] <= 1000]


def _fails(what, errs):
    with pytest.raises(AssertionError):
        L.check(what, errs)


@pytest.mark.parametrize("name,dt", SMALL_FWD)
def test_infonce_ref_matches_autograd(name, dt):
    bq, nd, hs, lab0, offdiag, normalised, taus = L.INFONCE_FWD_CASES[name]
    q, d = L.infonce_inputs(bq, nd, hs[dt], dt, normalised)
    g = 1.0 / bq
    for inv_tau in taus:
        q64, d64 = q.double().requires_grad_(True), d.double().requires_grad_(True)
        labels = lab0 + torch.arange(bq)
        s = inv_tau * q64 @ d64.t() - offdiag * (1.0 - F.one_hot(labels, nd).double())
        row = F.cross_entropy(s, labels, reduction="none")
        (g * row.sum()).backward()
        lse, row_loss, dq, dd = L.infonce_ref(q, d, inv_tau, offdiag, lab0, g)
        torch.testing.assert_close(lse, torch.logsumexp(s.detach(), 1), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(row_loss, row.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dq, q64.grad, rtol=1e-10, atol=1e-13)
        torch.testing.assert_close(dd, d64.grad, rtol=1e-10, atol=1e-13)
        l2, r2 = L.infonce_fwd_ref(q, d, inv_tau, offdiag, lab0)
        assert torch.equal(l2, lse) and torch.equal(r2, row_loss)


@pytest.mark.parametrize("name,dt", [(n, dt) for n, dt in SMALL_FWD if L.INFONCE_FWD_CASES[n][5]])
def test_dropped_lse_column_fails_forward_comparison(name, dt):
    bq, nd, hs, lab0, offdiag, _, _ = L.INFONCE_FWD_CASES[name]
    q, d = L.infonce_inputs(bq, nd, hs[dt], dt)
    s = L.infonce_scores(q, d, 1.0, offdiag, lab0)
    lse, row = L.infonce_fwd_ref(q, d, 1.0, offdiag, lab0)
    L.check(f"{name} {dt} correct", L.infonce_fwd_errs(lse.float(), row.float(), lse, row, dt))
    w = s.clone()
    w[torch.arange(bq), lab0 + torch.arange(bq)] = float("inf")  # the label column stays
    col = w.argmin(1)
    r = int(w.gather(1, col[:, None]).reshape(-1).argmin())  # the least visible drop of the whole case
    keep = torch.ones(nd, dtype=torch.bool)
    keep[col[r]] = False
    bad = lse.clone()
    bad[r] = torch.logsumexp(s[r, keep], 0)
    errs = L.infonce_fwd_errs(bad.float(), (row + bad - lse).float(), lse, row, dt)
    print(f"{name} {dt}: dropping column {int(col[r])} of row {r} moves lse by {errs[0][1]:.2f} x its bound")
    _fails(f"{name} {dt} dropped column", errs)


@pytest.mark.parametrize("dt,bq,nd,h,lab0,offdiag,flash", L.INFONCE_BWD_CASES)
def test_dropped_ds_column_fails_backward_comparison(dt, bq, nd, h, lab0, offdiag, flash):
    """The backward bounds: the reference passes its own comparison (in bf16, the reference
    with dS rounded to bf16 passes at half the per-row bound by construction); with the
    largest off-label dS entry of one row left out of both products it fails."""
    q, d = L.infonce_inputs(bq, nd, h, dt)
    g = 1.0 / bq
    bounds, (rq, rd) = L.bwd_row_bound(q, d, L.INV_TAU, offdiag, lab0, g)
    got = L.infonce_ref(q, d, L.INV_TAU, offdiag, lab0, g, ds_dtype=BF16 if dt == BF16 else None)
    L.check("correct", L.infonce_bwd_errs(got[2].float(), got[3].float(), rq, rd, dt, bounds))
    s = L.infonce_scores(q, d, L.INV_TAU, offdiag, lab0)
    r = bq // 2
    ds = g * torch.softmax(s[r], 0)
    ds[lab0 + r] = 0.0
    j = int(ds.argmax())
    bq_, bd_ = rq.clone(), rd.clone()
    bq_[r] -= L.INV_TAU * ds[j] * d[j].double()
    bd_[j] -= L.INV_TAU * ds[j] * q[r].double()
    _fails("dropped dS entry", L.infonce_bwd_errs(bq_.float(), bd_.float(), rq, rd, dt, bounds))


@pytest.mark.parametrize("make,eps", [(lambda: L.l2norm_inputs(5, 200), 1e-12), (lambda: L.l2norm_inputs(130, 1024), 1e-12),
                                      (lambda: L.l2norm_inputs(1, 8), 1e-12), (L.l2norm_clamped_inputs, 0.5)])
def test_l2norm_ref_matches_autograd(make, eps):
    x, dy, _ = make()
    x64 = x.double().requires_grad_(True)
    y = F.normalize(x64, p=2, dim=1, eps=eps)
    y.backward(dy.double())
    ry, rn = L.l2norm_ref(x, eps)
    torch.testing.assert_close(ry, y.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(rn, x.double().norm(dim=1), rtol=1e-13, atol=0)
    dx = L.l2norm_bwd_ref(dy, ry, rn, eps)
    assert bool(torch.isfinite(dx).all())
    torch.testing.assert_close(dx, x64.grad, rtol=1e-10, atol=1e-12 / eps)
    if eps == 0.5:
        assert torch.equal(ry, x.double() / 0.5) and torch.equal(dx, dy.double() / 0.5)
    else:
        assert torch.equal(ry[-1], torch.zeros_like(ry[-1])) and float(rn[-1]) == 0.0
        assert torch.equal(dx[-1], dy[-1].double() / eps)


def test_dropped_norm_column_fails_l2norm_comparison():
    x, _, _ = L.l2norm_inputs(130, 1024)
    eps = 1e-12
    ry, rn = L.l2norm_ref(x, eps)
    L.check("correct", L.l2norm_fwd_errs(ry.float(), rn.float(), x, eps))
    r = 3
    c = int(x[r].abs().argmin())
    xb = x.clone()
    xb[r, c] = 0.0
    bn = rn.clone()
    bn[r] = xb[r].double().norm()
    by = ry.clone()
    by[r] = x[r].double() / bn[r]
    errs = L.l2norm_fwd_errs(by.float(), bn.float(), x, eps)
    print(f"dropping column {c} (|x| = {float(x[r, c].abs()):.3f}) moves the norm by {errs[0][1] * 1e-5:.3g} relative")
    assert errs[0][1] > 10.0  # ten bounds and more: 1.1e-4 against 1e-5
    _fails("dropped column", errs)


def test_unclamped_formula_fails_l2norm_backward_comparison():
    x, dy, _ = L.l2norm_clamped_inputs()
    eps = 0.5
    ry, rn = L.l2norm_ref(x, eps)
    y32, n32 = ry.float(), rn.float()
    good = L.l2norm_bwd_ref(dy, y32, n32, eps)
    L.check("correct", L.l2norm_bwd_errs(good.float(), dy, y32, n32, eps))
    unclamped = (dy.double() - y32.double() * (y32.double() * dy.double()).sum(1, keepdim=True)) / eps
    _fails("unclamped formula", L.l2norm_bwd_errs(unclamped.float(), dy, y32, n32, eps))


def test_margin_ref_matches_reference_rule():
    """MarginRankingLoss with explicit negatives: relu(margin - cos(q, d+) + mean_j cos(q, d-_j))."""
    q, d, idx = L.margin_inputs(9, 12, 100, 5, 3)
    pos, negm, loss = L.margin_ref(q, d, 3, idx, 0.2)
    q64, d64 = q.double(), d.double()
    cp = F.cosine_similarity(q64, d64[3:12], dim=1)
    cn = F.cosine_similarity(q64.unsqueeze(1), d64[idx.long()], dim=2).mean(1)
    torch.testing.assert_close(pos, cp, rtol=0, atol=1e-6)  # the rows are normalised in fp32
    torch.testing.assert_close(loss, torch.relu(0.2 - cp + cn), rtol=0, atol=1e-6)
    assert abs(float(loss[0]) - 0.2) < 1e-12 and float(loss[1]) == 0.0 and float(loss[2]) == 0.0
    L.check("correct", L.margin_fwd_errs(loss.float(), pos, negm, 0.2))
    bad = loss.clone()
    bad[1] = 1e-7  # an inactive hinge must give exactly 0.0
    _fails("inactive row not zero", L.margin_fwd_errs(bad.float(), pos, negm, 0.2))


def test_colsum_order_ref_and_left_out_row():
    for rows, cols in ((300, 65), (17, 3072), (16, 1), (0, 63)):
        x, prev = L.colsum_inputs(rows, cols)
        for p in (None, prev):
            ref = L.colsum_order_ref(x, rows, cols, p)
            L.check(f"correct {rows} x {cols}", L.colsum_errs(ref, x, rows, cols, p))
            if rows:
                xb = x.clone()
                xb[rows - 1] = 0.0  # row 16k + 15 at rows 16 and 300
                _fails("left-out row", L.colsum_errs(L.colsum_order_ref(xb, rows, cols, p), x, rows, cols, p))
    x, _ = L.colsum_inputs(300, 64)
    flat = x[:300, :64].sum(0)  # another order of the same sum
    assert L.colsum_errs(flat, x, 300, 64)[0][1] > 0 and L.colsum_errs(flat, x, 300, 64)[1][1] <= 1.0


def test_truncation_fails_cast_comparison():
    x = L.cast_inputs(4096)
    ref = L.bf16_rne_ref(x)
    L.check("correct", L.cast_errs(ref, ref.clone()))
    assert bool(torch.isnan(ref[20:22]).all()) and bool(torch.isinf(ref[[16, 17, 18]]).all())
    assert ref[:2].view(torch.int16).tolist() == [0x3F80, 0x3F82]  # ties go to the even neighbour
    _fails("truncation", L.cast_errs(L.truncate_to_bf16(x), ref))
    _fails("truncation of one tie", L.cast_errs(torch.cat([L.truncate_to_bf16(x[1:2]), ref[1:]]), ref))
    p = L.pack_rows_ref(x[:600].reshape(2, 300), 300, 304, BF16)
    assert torch.equal(p[:, 300:], torch.zeros(2, 4, dtype=BF16)) and L.bits_differ(p[:, :300], ref[:600])[0] == 0
    assert L.bits_differ(torch.tensor([0.0]), torch.tensor([-0.0]))[0] == 1


def test_sum_bound_reads_a_left_out_element_or_thread():
    """tt_sum's bound reads the 257th element (a thread's second trip) left out at n = 257, and
    one thread's whole chain (i % 256 == 255) left out at n = 100000, where the bound is 2.4e-5
    of sum|x| and a single element 1e-5."""
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(100000, generator=gen) + 0.5
    L.check("correct", L.sum_errs((0.25 * x.double().sum()).float(), x, 0.25))
    mask = torch.arange(100000) % 256 != 255
    _fails("left-out thread", L.sum_errs((0.25 * x[mask].double().sum()).float(), x, 0.25))
    L.check("correct 257", L.sum_errs((0.25 * x[:257].double().sum()).float(), x[:257], 0.25))
    _fails("left-out element", L.sum_errs((0.25 * x[:256].double().sum()).float(), x[:257], 0.25))
    L.check("empty", L.sum_errs(torch.zeros(()), x[:0], 0.25))
