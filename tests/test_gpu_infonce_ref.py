"""tt_infonce_fwd and tt_infonce_bwd through the C ABI, row by row against the float64
restatement oracle/loss_ref.py (infonce_ref) on the operands as rounded to the storage dtype:
    S = inv_tau q d^T - offdiag [j != label_i],  lse_i = log sum_j exp S_ij,
    row_loss_i = lse_i - S_i,label_i,  dS = g (softmax - onehot),  dq = inv_tau dS d,
    dd = inv_tau dS^T q.
The comparison functions are loss_ref's; tests/test_loss_ref_host.py shows on the CPU that
they reject a reference with one column dropped from one row.

Forward cases (oracle.loss_ref.INFONCE_FWD_CASES), bq x nd x h (fp32 / bf16), label offset,
offdiag; each the smallest instance of what it names. Geometry: row blocks rb = ceil(bq / 128),
column tiles nct = ceil(nd / 128), splits = min(nct, ceil(1024 / rb)), per = ceil(nct / splits)
tiles per workgroup, splits = ceil(nct / per).
  one_row_tail_label        1 x 129 x 4 / 8, 128, 0       one query row in a 128-row tile; one
        column in the tail tile, and it is the label; K = one 16-byte chunk of a K-tile.
        rb 1, nct 2, 2 splits of 1 tile.
  second_row_block_k_tail   130 x 300 x 36 / 72, 170, 0   two rows in the second row block; K =
        one 128-byte tile + 16 bytes; labels end at the last column. rb 2, nct 3, 3 splits of 1.
  offdiag                   257 x 517 x 8, 0, 0.2         one row in a third block, the
        off-diagonal shift. rb 3, nct 5, 5 splits of 1.
  margin_branch_unnormalised  the same shape with un-normalised randn rows, inv_tau 10: the
        in-batch MarginRankingLoss branch. Its rows span more than 88 in score, so the
        running-max rescale and underflowing terms are exercised.
  h512                      130 x 520 x 512 (bf16), 0, 0  the training hidden size; 4 K-tiles
        (bf16 1024 bytes = 8). rb 2, nct 5, 5 splits of 1.
  short_last_split          1100 x 14853 x 8, 13753, 0    a workgroup sweeps more than one
        column tile and the last split is short: rb 9, ceil(1024 / 9) = 114, nct 117, per 2,
        59 splits, the last with one tile (a partial one, which holds the last labels). Its
        float64 reference runs on the device; inv_tau = 1 / 0.07 only.
Every other normalised case runs at inv_tau = 1 (the flat softmax in which every single column
carries weight) and at 1 / 0.07.

Forward tolerances (the project's): bf16 |lse - ref| <= 1e-5 max|lse| + 2e-4 and |row_loss -
ref| <= 2e-4 (test_gpu_infonce_bwd.py); fp32 |x - ref| <= 1e-4 |ref| + 1e-5
(test_gpu_infonce_sym.py). For the un-normalised case the absolute terms are
multiplied by the row's max_j |S_ij| (they were set for |S| <= inv_tau; an fp32 score of size
|S| carries an error of order 2^-24 |S|). Errors are printed as multiples of the bound.

Backward cases (INFONCE_BWD_CASES), at inv_tau = 1 / 0.07, g = 1 / bq, lse = the reference's
rounded to fp32 (so the backward is judged alone):
  fp32 (materialised dS in fp32, two tt_gemm products): 1 x 129 x 4, 130 x 300 x 36,
      257 x 517 x 8 (offdiag 0.2), 257 x 1001 x 32 (nd % 8 = 1; the tt_gemm split counts are
      printed).
  bf16 materialised: 1 x 129 x 8, 130 x 300 x 72, 257 x 517 x 8, 130 x 520 x 512 (nd % 8 = 1, 4,
      5, 0: the pad columns of dS up to ldds = ceil(nd / 8) * 8 are never written).
  bf16 fused at its smallest shapes, 1 x 129 x 128 (one own row) and 40 x 40 x 256 (fewer than
      64 swept rows), and the same two with infonce_flash = 0.
Every workspace is tt_infonce_*_ws_size bytes of 0xFF (NaN in both dtypes) followed by a guard
that must survive; outputs are pre-filled with NaN; every case runs twice and dq, dd must have
identical bits.

Backward tolerances: fp32 row_err <= 1e-4 (the project's per-row fp32 value). bf16: the existing
whole-tensor bound (max-abs <= 1.5e-2 of the largest entry, cosine >= 0.9999) and, per row,
row_err <= twice the per-row error of the reference with dS rounded to bf16 against the
unrounded reference (loss_ref.bwd_row_bound, computed per case on the CPU, never from the
kernel's output). Per case, dq / dd: that reference error; the bound is twice it; the kernel's
error measured on an MI355X equals the reference error to the three digits printed, on the
materialised and the fused path alike (the kernels round dS exactly as the reference does):
  1 x 129 x 8       8.88e-4 / 3.10e-3        130 x 520 x 512   2.02e-3 / 2.90e-3
  130 x 300 x 72    2.06e-3 / 3.27e-3        1 x 129 x 128     7.19e-4 / 3.81e-3
  257 x 517 x 8     2.81e-3 / 2.75e-3        40 x 40 x 256     2.46e-3 / 2.64e-3
  whole tensor: max-abs <= 2.1e-3, 1 - cosine <= 1.2e-6 (40 x 40 x 256).
Largest errors measured on an MI355X otherwise:
  forward, as a fraction of the bound: fp32 0.0024 (offdiag, 1 / 0.07), 0.0041 un-normalised;
      bf16 0.012 (short_last_split: 2.4e-6 in row_loss), 0.0009 un-normalised
  backward fp32, per row: dq 1.3e-6, dd 2.1e-6 (257 x 1001 x 32; its dq product ran split-K in 2)
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import loss_ref as L  # noqa: E402
from oracle.loss_ref import BF16, F32, INV_TAU  # noqa: E402
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import TTError, call, dtype_code, option, stream_ptr  # noqa: E402

DEV = "cuda"
GUARD = 256


def _poisoned(nbytes):
    """nbytes of 0xFF (NaN in fp32 and bf16) followed by a guard."""
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    ws[:nbytes] = 0xFF
    ws[nbytes:] = 0xA5
    return ws


def _guard_ok(ws, nbytes):
    return bool((ws[nbytes:] == 0xA5).all())


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def run_fwd(q, d, inv_tau, offdiag, lab0):
    lib = _lib.load()
    (bq, h), nd = q.shape, d.shape[0]
    qd, dd = q.to(DEV).contiguous(), d.to(DEV).contiguous()
    lse, row = _nan(bq), _nan(bq)
    n = lib.tt_infonce_fwd_ws_size(bq, nd)
    ws = _poisoned(n)
    call("tt_infonce_fwd", dtype_code(q.dtype), qd.data_ptr(), bq, dd.data_ptr(), nd, h, inv_tau, offdiag, lab0,
         lse.data_ptr(), row.data_ptr(), ws.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(ws, n), "tt_infonce_fwd wrote past tt_infonce_fwd_ws_size"
    return lse.cpu(), row.cpu()


@pytest.mark.parametrize("name,dt", [(n, dt) for n, c in L.INFONCE_FWD_CASES.items() for dt in c[2]])
def test_infonce_fwd_rows_match_float64(name, dt):
    bq, nd, hs, lab0, offdiag, normalised, taus = L.INFONCE_FWD_CASES[name]
    q, d = L.infonce_inputs(bq, nd, hs[dt], dt, normalised)
    on = DEV if bq * nd > 1 << 20 else "cpu"  # the large case's float64 reference runs on the device
    for inv_tau in taus:
        lse, row = run_fwd(q, d, inv_tau, offdiag, lab0)
        rlse, rrow = L.infonce_fwd_ref(q.to(on), d.to(on), inv_tau, offdiag, lab0)
        smax = None
        if not normalised:
            s = L.infonce_scores(q, d, inv_tau, offdiag, lab0)
            smax = s.abs().amax(1)
            print(f"{name}: rows span up to {float((s.amax(1) - s.amin(1)).max()):.0f} in score, max |S| {float(smax.max()):.0f}")
        L.check(f"infonce fwd {name} {dt} inv_tau {inv_tau:.3g}", L.infonce_fwd_errs(lse, row, rlse, rrow, dt, smax))


@functools.lru_cache(maxsize=None)
def _bwd_case(dt, bq, nd, h, lab0, offdiag):
    """Inputs, the fp32 lse handed to the kernel, the float64 references and the bf16 per-row
    bounds of one backward case; computed once and left unchanged."""
    q, d = L.infonce_inputs(bq, nd, h, dt)
    g = 1.0 / bq
    bounds, (rq, rd) = L.bwd_row_bound(q, d, INV_TAU, offdiag, lab0, g)
    lse = L.infonce_fwd_ref(q, d, INV_TAU, offdiag, lab0)[0].float()
    return q, d, g, lse, rq, rd, bounds


def run_bwd(q, d, inv_tau, offdiag, lab0, lse, g, flash, what):
    """tt_infonce_bwd twice on poisoned workspaces; returns (dq, dd) of the first call after
    requiring identical bits from the second. g None: gscale = NULL."""
    lib = _lib.load()
    (bq, h), nd = q.shape, d.shape[0]
    dtc = dtype_code(q.dtype)
    qd, dd, lsed = q.to(DEV).contiguous(), d.to(DEV).contiguous(), lse.to(DEV)
    gdev = None if g is None else torch.tensor([g], dtype=torch.float32, device=DEV)
    outs = []
    with option("infonce_flash", flash):
        n = lib.tt_infonce_bwd_ws_size(dtc, bq, nd, h)
        assert n > 0
        for _ in range(2):
            ws, dq, ddn = _poisoned(n), _nan(bq, h), _nan(nd, h)
            call("tt_infonce_bwd", dtc, qd.data_ptr(), bq, dd.data_ptr(), nd, h, inv_tau, offdiag, lab0, lsed.data_ptr(),
                 None if gdev is None else gdev.data_ptr(), dq.data_ptr(), ddn.data_ptr(), ws.data_ptr(), stream_ptr())
            torch.cuda.synchronize()
            assert _guard_ok(ws, n), f"{what}: tt_infonce_bwd wrote past tt_infonce_bwd_ws_size"
            outs.append((dq.cpu(), ddn.cpu()))
    for a, b, name in zip(outs[0], outs[1], ("dq", "dd")):
        assert L.bits_differ(a, b)[0] == 0, f"{what}: two runs of {name} differ (a result depends on the workspace's contents)"
    return outs[0]


@pytest.mark.parametrize("dt,bq,nd,h,lab0,offdiag,flash",
                         [(*c[:6], f) for c in L.INFONCE_BWD_CASES for f in c[6]])
def test_infonce_bwd_rows_match_float64(dt, bq, nd, h, lab0, offdiag, flash):
    q, d, g, lse, rq, rd, bounds = _bwd_case(dt, bq, nd, h, lab0, offdiag)
    what = f"infonce bwd {dt} {bq} x {nd} x {h} flash {flash}"
    if dt == F32:
        lib = _lib.load()
        print(f"{what}: tt_gemm_pick_splits dq {lib.tt_gemm_pick_splits(bq, h, nd, 1)}, dd {lib.tt_gemm_pick_splits(nd, h, bq, 1)}")
    else:
        print(f"{what}: per-row error of the bf16-dS reference dq {bounds[0] / 2:.3g} dd {bounds[1] / 2:.3g}")
    dq, dd = run_bwd(q, d, INV_TAU, offdiag, lab0, lse, g, flash, what)
    errs = L.infonce_bwd_errs(dq, dd, rq, rd, dt, bounds)
    print(f"{what}: " + ", ".join(f"{n} {e:.3g}" for n, e, _, _ in errs))
    L.check(what, errs)


@pytest.mark.parametrize("dt,bq,nd,h,lab0,flash", [(BF16, 130, 300, 72, 170, 1), (BF16, 40, 40, 256, 0, 1), (F32, 130, 300, 36, 170, 1)])
def test_infonce_bwd_null_gscale_is_g_one(dt, bq, nd, h, lab0, flash):
    """gscale = NULL equals the g = 1 result bit for bit (materialised bf16, fused, fp32)."""
    q, d = L.infonce_inputs(bq, nd, h, dt)
    lse = L.infonce_fwd_ref(q, d, INV_TAU, 0.0, lab0)[0].float()
    a = run_bwd(q, d, INV_TAU, 0.0, lab0, lse, None, flash, "gscale NULL")
    b = run_bwd(q, d, INV_TAU, 0.0, lab0, lse, 1.0, flash, "g = 1")
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())
    assert L.bits_differ(a[0], b[0])[0] == 0 and L.bits_differ(a[1], b[1])[0] == 0


def _bwd_args(dt, bq, nd, h, lab0, ws="poison"):
    """Valid, allocated arguments for a call that must return before any launch."""
    lib = _lib.load()
    dtc = dtype_code(dt)
    t = dict(q=torch.zeros(max(bq, 1), h, dtype=dt, device=DEV), d=torch.zeros(nd, h, dtype=dt, device=DEV),
             lse=torch.zeros(max(bq, 1), device=DEV), dq=_nan(max(bq, 1), h), dd=_nan(nd, h))
    n = max(int(lib.tt_infonce_bwd_ws_size(dtc, max(bq, 1), nd, (h + 7) // 8 * 8)), 256)
    t["ws"], t["n"] = _poisoned(n), n
    args = (dtc, t["q"].data_ptr(), bq, t["d"].data_ptr(), nd, h, INV_TAU, 0.0, lab0, t["lse"].data_ptr(), None,
            t["dq"].data_ptr(), t["dd"].data_ptr(), None if ws is None else t["ws"].data_ptr(), stream_ptr())
    return t, args


def _untouched(t):
    torch.cuda.synchronize()
    assert bool(torch.isnan(t["dq"]).all()) and bool(torch.isnan(t["dd"]).all()), "an output was written"
    assert bool((t["ws"][:t["n"]] == 0xFF).all()) and _guard_ok(t["ws"], t["n"]), "the workspace was written"


@pytest.mark.parametrize("dt,h", [(F32, 8), (BF16, 8), (BF16, 128)])
def test_infonce_bwd_argument_checks_return_before_any_launch(dt, h):
    """bq = 0 is a no-op; labels outside [0, nd) and a null workspace are TTError; in every
    case the NaN-filled outputs and the poisoned workspace are untouched."""
    t, args = _bwd_args(dt, 0, 40, h, 0)
    call("tt_infonce_bwd", *args)
    _untouched(t)
    for bq, nd, lab0, ws, msg in ((8, 40, 33, "poison", "labels"), (8, 40, -1, "poison", "labels"), (8, 40, 0, None, "workspace")):
        t, args = _bwd_args(dt, bq, nd, h, lab0, ws)
        with pytest.raises(TTError, match=msg):
            call("tt_infonce_bwd", *args)
        _untouched(t)


@pytest.mark.parametrize("dt,h", [(F32, 6), (F32, 33), (BF16, 12), (BF16, 4), (BF16, 132)])
def test_infonce_bwd_rejects_misaligned_h(dt, h):
    """A row of h elements that is no multiple of 16 bytes is TT_EINVAL in tt_infonce_bwd as in
    tt_infonce_fwd, on both paths, before infonce_dscore_kernel or anything else is launched."""
    for flash in (1, 0):
        with option("infonce_flash", flash):
            t, args = _bwd_args(dt, 8, 40, h, 0)
            with pytest.raises(TTError, match="misaligned"):
                call("tt_infonce_bwd", *args)
            _untouched(t)
