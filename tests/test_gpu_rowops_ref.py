"""The small kernels around the losses, called directly through the C ABI and compared with
oracle/loss_ref.py: tt_l2norm_fwd / _bwd, tt_margin_fwd (with tt_margin_bwd on the same
inputs), tt_colsum, tt_sum, tt_cast and tt_pack_rows. The comparison functions are loss_ref's;
tests/test_loss_ref_host.py shows on the CPU that each rejects one planted defect. Outputs are
pre-filled with NaN and followed by guard elements that must survive.

tt_l2norm_fwd / _bwd: rows in {1, 5, 130} (one row; 4 rows per workgroup plus one; tails), cols
  in {1, 8, 63, 64, 65, 200, 1024} (one lane; under, at and over one wave; no multiple of 64; the
  limit of 16 columns per lane), fp32 and bf16 y, y32 given and NULL. |x| in [0.5, 1.5] with random
  signs. The last row of every case is all zero (one row: once zero, once not): y = 0, norm = 0,
  dx = dy / eps, no NaN. One case has eps = 0.5 and rows of norm 0.1: the clamped branch on
  ordinary numbers. 1025 and 1032 columns are TT_EINVAL, rows = 0 a no-op.
  Tolerances: norm 1e-5 relative (the summation, 16 sequential terms per lane, a 6-level wave
  tree and one sqrt, is bounded near 24 x 2^-24 = 1.4e-6: 7x slack, 10x below the shift of one
  dropped column); fp32 y and dx: the project's per-row fp32 tolerance 1e-4 (dx against the
  reference at the kernel's own y32 and norm); bf16 y = y32.to(bfloat16) bit for bit, and the
  y32 = NULL call gives the same bits as the other; accumulate = 1 equals dx_prev + dx_plain in
  fp32 bit for bit.
tt_margin_fwd: k in {1, 5, 17}, h in {8, 100, 512}, 37 rows (two 32-row groups of the backward),
  50 documents, label_offset 13, negatives drawn from 6 documents (repeats inside and across
  rows). Row 0's negatives all equal its positive: loss = margin. Rows 1 and 2 have their own
  query as positive: hinge inactive, loss exactly 0.0. Absolute tolerance 1e-5 (cosines are
  bounded by 1). tt_margin_bwd on the same inputs: a row's dqn is all zero exactly when its
  forward loss is 0. Row 0 is left out of that equivalence: its negatives' mean IS its
  positive, so its dqn = g (mean_j d_j - d_pos) is zero with a loss of margin; it is required to
  be below 1e-6 instead.
tt_colsum: rows in {0, 1, 15, 16, 17, 300} x cols in {1, 63, 64, 65, 3072}, ld = cols + 5,
  accumulate 0 and 1: bit-identical to colsum_order_ref and within rows x 2^-24 x sum|x| of
  float64; rows = 0 zeroes out / leaves it alone; 8 guard columns untouched.
tt_sum: n in {0, 1, 255, 256, 257, 100000}, scale 0.37: within (ceil(n / 256) + 12) x 2^-24 x
  |scale| x sum|x| of float64 (a thread's chain plus the reductions).
tt_cast / tt_pack_rows: bf16 results bit-identical to torch's round-to-nearest-even (exact
  ties, +-0, denormals, infinities, values that round up to infinity; NaN stays NaN), fp32 a bit
  copy; tt_pack_rows at (e, ep) = (300, 304), (1, 8), (8, 8) with zero pad columns, ep < e
  TT_EINVAL, n = 0 a no-op; one size each above 8192 x 256 elements (a second grid-stride trip).

The l2norm backward is measured per row against the larger of the row's reference gradient and
of its terms dy / norm (loss_ref.l2norm_bwd_errs): with one column the two terms cancel and the
gradient itself has no scale.

Largest errors measured on an MI355X:
  l2norm    norm 1.2e-7 relative (130 x 1024), y 1.7e-7 per row (130 x 65), dx 1.5e-7 per row
            (130 x 63), zero rows' dx 4.6e-8; bf16 y, the y32 = NULL calls and accumulate: 0 bits
  margin    row_loss 6.4e-8 at k = 1 (0.0064 of the bound) and under 1e-6 at every k; row 0's
            dqn 9.0e-8 (k 17, h 8)
  colsum    0 bits from the stated order everywhere; against float64 0.19 of the bound at
            15 <= rows <= 17, 0.0025 at 300 rows, and up to 0.997 at one row with accumulate
            (one rounding against a bound of one rounding)
  sum       0.013 of the bound (n 255)
  cast, pack_rows   0 bits
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import loss_ref as L  # noqa: E402
from oracle.loss_ref import BF16, F32  # noqa: E402
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import TTError, call, dtype_code, stream_ptr  # noqa: E402

DEV = "cuda"
GUARD = 64  # elements


def _out(n, dt=F32, fill=float("nan")):
    """n elements of fill followed by GUARD elements of 7 in one buffer."""
    buf = torch.full((n + GUARD,), fill, dtype=dt, device=DEV)
    buf[n:] = 7.0
    return buf


def _guard_ok(buf, n):
    return bool((buf[n:] == 7.0).all())


# ---------------------------------------------------------------------------- l2norm
def _l2norm_fwd(x, eps, dt, want_y32):
    rows, cols = x.shape
    n = rows * cols
    xd = x.to(DEV).contiguous()
    y, y32, norm = _out(n, dt), _out(n), _out(rows)
    call("tt_l2norm_fwd", dtype_code(dt), xd.data_ptr(), rows, cols, eps, y.data_ptr(),
         y32.data_ptr() if want_y32 else None, norm.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(y, n) and _guard_ok(y32, n) and _guard_ok(norm, rows), "tt_l2norm_fwd wrote past an output"
    if not want_y32:
        assert bool(torch.isnan(y32[:n]).all())
    return y[:n].reshape(rows, cols).cpu(), y32[:n].reshape(rows, cols).cpu(), norm[:rows].cpu()


def _l2norm_bwd(dy, y32, norm, eps, prev):
    rows, cols = dy.shape
    n = rows * cols
    dx = _out(n)
    if prev is not None:
        dx[:n] = prev.reshape(-1).to(DEV)
    args = [t.to(DEV).contiguous() for t in (dy, y32, norm)]
    call("tt_l2norm_bwd", args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), rows, cols, eps, dx.data_ptr(),
         int(prev is not None), stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(dx, n), "tt_l2norm_bwd wrote past dx"
    return dx[:n].reshape(rows, cols).cpu()


def _l2norm_case(what, x, dy, prev, eps):
    errs = []
    first = {}
    for dt in (F32, BF16):
        for want_y32 in (True, False):
            y, y32, norm = _l2norm_fwd(x, eps, dt, want_y32)
            if want_y32:
                first[dt] = (y, y32, norm)
                errs += [(f"{n} ({dt})", e, i, b) for n, e, i, b in L.l2norm_fwd_errs(y32, norm, x, eps)]
                errs.append((f"y {dt} bits differing from y32 rounded", float(L.bits_differ(y, y32.to(dt))[0]), (), 0.0))
            else:
                errs.append((f"y {dt} bits differing between y32 NULL and given", float(L.bits_differ(y, first[dt][0])[0]), (), 0.0))
                errs.append((f"norm {dt} bits differing between y32 NULL and given", float(L.bits_differ(norm, first[dt][2])[0]), (), 0.0))
    _, y32, norm = first[F32]
    dx = _l2norm_bwd(dy, y32, norm, eps, None)
    assert bool(torch.isfinite(dx).all()), f"{what}: dx is not finite"
    errs += L.l2norm_bwd_errs(dx, dy, y32, norm, eps)
    acc = _l2norm_bwd(dy, y32, norm, eps, prev)
    errs.append(("accumulate bits differing from dx_prev + dx", float(L.bits_differ(acc, prev + dx)[0]), (), 0.0))
    top = {k: max(e[1] for e in errs if e[0].startswith(k)) for k in ("norm (", "y (", "dx")}
    print(f"{what}: norm {top['norm ('] * 1e-5:.3g} relative, y {top['y (']:.3g}, dx {top['dx']:.3g} per row")
    L.check(what, errs)
    return y32, norm, dx


@pytest.mark.parametrize("cols", L.L2NORM_COLS)
@pytest.mark.parametrize("rows,zero_row", [(1, True), (1, False), (5, True), (130, True)])
def test_l2norm_matches_float64(rows, zero_row, cols):
    eps = 1e-12
    x, dy, prev = L.l2norm_inputs(rows, cols, zero_row)
    y32, norm, dx = _l2norm_case(f"l2norm {rows} x {cols} zero row {zero_row}", x, dy, prev, eps)
    if zero_row:
        assert float(norm[-1]) == 0.0 and not bool(y32[-1].any())
        assert L.row_err(dx[-1:], dy[-1:].double() / eps)[0] <= L.TOL_ROW_F32


def test_l2norm_clamped_branch_on_ordinary_numbers():
    """eps = 0.5, rows of norm 0.1: y = x / 0.5 and dx = dy / 0.5."""
    x, dy, prev = L.l2norm_clamped_inputs()
    y32, norm, dx = _l2norm_case("l2norm clamped", x, dy, prev, 0.5)
    L.check("l2norm clamped, closed form", [("y", *L.row_err(y32, x.double() / 0.5), L.TOL_ROW_F32),
                                             ("dx", *L.row_err(dx, dy.double() / 0.5), L.TOL_ROW_F32)])


def test_l2norm_limits():
    """More than 16 columns per lane is TT_EINVAL in both entry points; rows = 0 is a no-op."""
    buf = _out(4 * 1032)
    for cols in (1025, 1032):
        with pytest.raises(TTError):
            call("tt_l2norm_fwd", _lib.DT_F32, buf.data_ptr(), 4, cols, 1e-12, buf.data_ptr(), None, buf.data_ptr(), stream_ptr())
        with pytest.raises(TTError):
            call("tt_l2norm_bwd", buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 4, cols, 1e-12, buf.data_ptr(), 0, stream_ptr())
    call("tt_l2norm_fwd", _lib.DT_F32, buf.data_ptr(), 0, 64, 1e-12, buf.data_ptr(), None, buf.data_ptr(), stream_ptr())
    call("tt_l2norm_bwd", buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, 64, 1e-12, buf.data_ptr(), 0, stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:4 * 1032]).all()) and _guard_ok(buf, 4 * 1032)


# ---------------------------------------------------------------------------- margin
@pytest.mark.parametrize("h", [8, 100, 512])
@pytest.mark.parametrize("k", [1, 5, 17])
def test_margin_fwd_matches_float64(k, h):
    bq, nd, lab0, margin = 37, 50, 13, 0.2
    q, d, idx = L.margin_inputs(bq, nd, h, k, lab0)
    qd, dd, idd = q.to(DEV), d.to(DEV), idx.to(DEV)
    loss = _out(bq)
    call("tt_margin_fwd", qd.data_ptr(), bq, dd.data_ptr(), nd, h, lab0, idd.data_ptr(), k, margin, loss.data_ptr(), stream_ptr())
    n = _lib.load().tt_margin_bwd_ws_size(bq, nd, h, k)
    ws = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[n:] = 0xA5
    dqn, ddn = _out(bq * h), torch.zeros(nd, h, device=DEV)
    call("tt_margin_bwd", qd.data_ptr(), bq, dd.data_ptr(), nd, h, lab0, idd.data_ptr(), k, margin, None,
         dqn.data_ptr(), ddn.data_ptr(), ws.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(loss, bq) and _guard_ok(dqn, bq * h) and bool((ws[n:] == 0xA5).all())
    loss, dqn = loss[:bq].cpu(), dqn[:bq * h].reshape(bq, h).cpu()
    pos, negm, ref = L.margin_ref(q, d, lab0, idx, margin)
    assert int((ref == 0).sum()) >= 2 and int((ref > 1e-3).sum()) >= 2, "the case needs active and inactive rows"
    errs = L.margin_fwd_errs(loss, pos, negm, margin)
    errs.append(("row 0 (negatives = positive) against the margin", abs(float(loss[0]) - margin), (0,), 1e-5))
    assert float(loss[1]) == 0.0 and float(loss[2]) == 0.0
    zero_grad = ~dqn.ne(0).any(1)
    differ = (zero_grad != (loss == 0))[1:]
    errs.append(("rows whose dqn is zero without a zero loss or the reverse", float(differ.sum()), (), 0.0))
    errs.append(("row 0 dqn (mean of negatives = positive)", float(dqn[0].abs().max()), (0,), 1e-6))
    assert bool(torch.isfinite(dqn).all()) and bool(torch.isfinite(ddn).all())
    L.check(f"margin fwd k {k} h {h}", errs)


# ---------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("cols", L.COLSUM_COLS)
@pytest.mark.parametrize("rows", L.COLSUM_ROWS)
def test_colsum_is_the_stated_order_bit_for_bit(rows, cols):
    x, prev = L.colsum_inputs(rows, cols)
    xd = x.to(DEV)
    for acc in (0, 1):
        out = _out(cols)
        if acc:
            out[:cols] = prev.to(DEV)
        call("tt_colsum", xd.data_ptr(), rows, cols, x.shape[1], out.data_ptr(), acc, stream_ptr())
        torch.cuda.synchronize()
        assert _guard_ok(out, cols), "tt_colsum wrote past cols"
        got = out[:cols].cpu()
        if rows == 0:
            assert L.bits_differ(got, prev if acc else torch.zeros(cols))[0] == 0
        L.check(f"colsum {rows} x {cols} accumulate {acc}", L.colsum_errs(got, x, rows, cols, prev if acc else None))


# ------------------------------------------------------------------------------- sum
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100000])
def test_sum_matches_float64(n):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(max(n, 1), generator=gen)
    xd = x.to(DEV)
    out = _out(1)
    call("tt_sum", xd.data_ptr(), n, 0.37, out.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(out, 1)
    if n == 0:
        assert float(out[0]) == 0.0
    L.check(f"sum n {n}", L.sum_errs(out[:1].cpu(), x[:n], 0.37))


# --------------------------------------------------------------------- cast, pack_rows
@pytest.mark.parametrize("n", [4096, 8192 * 256 + 1000])
def test_cast_rounds_to_nearest_even(n):
    x = L.cast_inputs(n)
    xd = x.to(DEV)
    for dt in (BF16, F32):
        y = _out(n, dt)
        call("tt_cast", dtype_code(dt), xd.data_ptr(), n, y.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        assert _guard_ok(y, n), "tt_cast wrote past n"
        got = y[:n].cpu()
        assert bool(torch.isnan(got[20:22]).all()), "NaN must stay NaN"
        L.check(f"cast {dt} n {n}", L.cast_errs(got, L.bf16_rne_ref(x) if dt == BF16 else x))
    y = _out(8)
    call("tt_cast", _lib.DT_BF16, xd.data_ptr(), 0, y.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[:8]).all())


@pytest.mark.parametrize("n,e,ep", [(7, 300, 304), (7, 1, 8), (7, 8, 8), (6901, 300, 304)])
def test_pack_rows_rounds_and_pads(n, e, ep):
    src = L.cast_inputs(n * e).reshape(n, e)
    sd = src.to(DEV)
    for dt in (BF16, F32):
        out = _out(n * ep, dt)
        call("tt_pack_rows", dtype_code(dt), sd.data_ptr(), n, e, ep, out.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        assert _guard_ok(out, n * ep), "tt_pack_rows wrote past n * ep"
        L.check(f"pack_rows {dt} {n} x {e} -> {ep}", L.cast_errs(out[:n * ep].cpu().reshape(n, ep), L.pack_rows_ref(src, e, ep, dt)))
    out = _out(64)
    call("tt_pack_rows", _lib.DT_BF16, sd.data_ptr(), 0, e, ep, out.data_ptr(), stream_ptr())
    with pytest.raises(TTError):
        call("tt_pack_rows", _lib.DT_BF16, sd.data_ptr(), n, ep + 1, ep, out.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:64]).all()) and _guard_ok(out, 64)
