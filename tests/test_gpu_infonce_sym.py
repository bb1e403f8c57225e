"""tt_infonce_sym_fwd / tt_infonce_sym_bwd (the symmetric InfoNCE of simple_two_tower.py:68-78,
(CE(S, arange) + CE(S^T, arange)) / 2 with S = inv_tau q d^T) through the C ABI, against
float64 logsumexp / softmax math on the operands as rounded to the dtype:
    lse_row_i = LSE_j S_ij, lse_col_j = LSE_i S_ij, row_loss_i = ((lse_row_i - S_ii) + (lse_col_i - S_ii)) / 2,
    dS_ij = g/2 (exp(S_ij - lse_row_i) + exp(S_ij - lse_col_j) - 2 [i == j]), dq = inv_tau dS d, dd = inv_tau dS^T q.
The column direction is the new ground: a tail row block must keep its rows >= n out of
the column sums (n = 130, 300, 200), and several row blocks must merge (n = 256, 2048).

Tolerances. Forward, bf16: lse within 1e-5 max|lse| + 2e-4, row_loss within 2e-4 (the
bounds of test_gpu_infonce_bwd.py); fp32: rtol 1e-4 / atol 1e-5. Backward,
bf16: dS is rounded to bf16 before the second product on both paths, so max-abs error
<= 1.5e-2 of the largest entry and cosine >= 0.9999; fp32: the fp32 tolerance."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import call, dtype_code, option  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
INV_TAU = 10.0

CASES = [  # n, h, dtype
    (256, 256, BF),    # two row blocks to merge
    (130, 256, BF),    # tail rows and tail columns
    (300, 128, BF),
    (2048, 128, BF),   # 16 blocks x split sweeps
    (200, 32, F32),    # materialised path
    (130, 8, F32),
]
PARAMS = [(n, h, dt, fl) for n, h, dt in CASES for fl in ((1, 0) if dt == BF else (1,))]


@functools.lru_cache(maxsize=None)
def reference(n, h, dt):
    """Rounded operands (fp32 values, CPU) and the float64 results; computed once per case."""
    gen = torch.Generator().manual_seed(n + 7 * h)
    q = torch.nn.functional.normalize(torch.randn(n, h, generator=gen), dim=1).to(dt).float()
    d = torch.nn.functional.normalize(torch.randn(n, h, generator=gen), dim=1).to(dt).float()
    q64, d64 = q.double(), d.double()
    s = INV_TAU * (q64 @ d64.t())
    lr, lc = torch.logsumexp(s, dim=1), torch.logsumexp(s, dim=0)
    diag = s.diagonal()
    row = 0.5 * ((lr - diag) + (lc - diag))
    g = 1.0 / n
    ds = 0.5 * g * (torch.softmax(s, dim=1) + torch.softmax(s, dim=0) - 2.0 * torch.eye(n, dtype=torch.float64))
    return q, d, lr, lc, row, INV_TAU * ds @ d64, INV_TAU * ds.t() @ q64


def run_sym(q, d, dt, flash, ws_fill):
    lib = _lib.load()
    n, h = q.shape
    qd, dd = q.to(DEV, dt).contiguous(), d.to(DEV, dt).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    nan = float("nan")
    lr, lc, row = (torch.full((n,), nan, device=DEV) for _ in range(3))
    wsf = torch.full((lib.tt_infonce_sym_fwd_ws_size(n, h),), ws_fill, dtype=torch.uint8, device=DEV)
    call("tt_infonce_sym_fwd", dtype_code(dt), qd.data_ptr(), dd.data_ptr(), n, h, INV_TAU, lr.data_ptr(),
         lc.data_ptr(), row.data_ptr(), wsf.data_ptr(), st)
    gdev = torch.tensor([1.0 / n], device=DEV)
    dq = torch.full((n, h), nan, device=DEV)
    ddn = torch.full((n, h), nan, device=DEV)
    with option("infonce_flash", flash):
        ws = torch.full((lib.tt_infonce_sym_bwd_ws_size(dtype_code(dt), n, h),), ws_fill, dtype=torch.uint8,
                        device=DEV)
        call("tt_infonce_sym_bwd", dtype_code(dt), qd.data_ptr(), dd.data_ptr(), n, h, INV_TAU, lr.data_ptr(),
             lc.data_ptr(), gdev.data_ptr(), dq.data_ptr(), ddn.data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize()
    return [t.cpu() for t in (lr, lc, row, dq, ddn)]


def one_direction(a, b, dt):
    """row losses of tt_infonce_fwd(a, b): CE of row i of inv_tau a b^T against label i"""
    lib = _lib.load()
    n, h = a.shape
    ad, bd = a.to(DEV, dt).contiguous(), b.to(DEV, dt).contiguous()
    lse = torch.empty(n, device=DEV)
    row = torch.empty(n, device=DEV)
    ws = torch.empty(lib.tt_infonce_fwd_ws_size(n, n), dtype=torch.uint8, device=DEV)
    call("tt_infonce_fwd", dtype_code(dt), ad.data_ptr(), n, bd.data_ptr(), n, h, INV_TAU, 0.0, 0, lse.data_ptr(),
         row.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return row.cpu()


def close_fwd(got, ref, dt, what):
    assert torch.isfinite(got).all(), what
    err = float((got.double() - ref).abs().max())
    if dt == BF:
        bound = 2e-4 if what == "row_loss" else 1e-5 * float(ref.abs().max()) + 2e-4
        print(f"{what}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, err, bound)
    else:
        print(f"{what}: max abs err {err:.3e}")
        torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("n,h,dt,flash", PARAMS)
def test_infonce_sym_matches_float64(n, h, dt, flash):
    q, d, rlr, rlc, rrow, rdq, rdd = reference(n, h, dt)
    lr, lc, row, dq, dd = run_sym(q, d, dt, flash, 0xFF)
    close_fwd(lr, rlr, dt, "lse_row")
    close_fwd(lc, rlc, dt, "lse_col")
    close_fwd(row, rrow, dt, "row_loss")
    for name, got, ref in (("dq", dq, rdq), ("dd", dd, rdd)):
        assert torch.isfinite(got).all(), name
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        cos = float((got.double() * ref).sum() / (got.double().norm() * ref.norm()))
        print(f"{name}: rel max err {err:.3e}, cosine {cos:.7f}")
        if dt == BF:
            assert err <= 1.5e-2 and cos >= 0.9999, (name, err, cos)
        else:
            torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-5)
    # deterministic, and independent of what the workspaces held before
    again = run_sym(q, d, dt, flash, 0x00)
    for a, b in zip((lr, lc, row, dq, dd), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n,h,dt", CASES)
def test_infonce_sym_equals_two_one_directional_calls(n, h, dt):
    """row_loss_i = (CE_i of tt_infonce_fwd(q, d) + CE_i of tt_infonce_fwd(d, q)) / 2, row by row
    and in the mean, within the forward tolerance."""
    q, d = reference(n, h, dt)[:2]
    row = run_sym(q, d, dt, 1, 0xFF)[2]
    comp = 0.5 * (one_direction(q, d, dt).double() + one_direction(d, q, dt).double())
    close_fwd(row, comp, dt, "row_loss")
    mean_err = abs(float(row.double().mean()) - float(comp.mean()))
    assert mean_err <= (2e-4 if dt == BF else 1e-5 + 1e-4 * abs(float(comp.mean()))), mean_err


def test_infonce_sym_empty_is_noop():
    call("tt_infonce_sym_fwd", dtype_code(F32), None, None, 0, 32, INV_TAU, None, None, None, None, None)
    call("tt_infonce_sym_bwd", dtype_code(F32), None, None, 0, 32, INV_TAU, None, None, None, None, None, None, None)
