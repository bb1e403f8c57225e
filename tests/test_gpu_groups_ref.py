"""The group-mask entry points through the C ABI (include/tt_hip.h, "Group masks"):
tt_infonce_fwd_grp / _bwd_grp, tt_infonce_sym_fwd_grp / _sym_bwd_grp and tt_topk_drop_groups,
against the masked float64 references of tests/groups_cases.py (infonce_ref of
oracle/loss_ref.py over S.masked_fill(excl, -inf)) through loss_ref's comparison functions and
tolerances. tests/test_groups_host.py shows that the unmasked reference, i.e. a kernel that
ignored the ids, fails every one of these comparisons.

Forward (groups_cases.FWD_CASES), at inv_tau 1 and 1 / 0.07:
  threes_other_tile          130 x 300 x 36 / 72, label offset 170: 2 row blocks, 3 column tiles,
        3 splits of 1. Rows < 120 in groups of three; a row's mates sit at 170 + i (tiles 1, 2) and
        at j < 60 (tile 0, another split than the label's).
  all_but_label_excluded     1 x 129 x 4 / 8, label 128, every column in the row's group: split 0
        is excluded as a whole and must contribute the neutral partial: lse = S_label, row_loss = 0,
        no NaN.
  margin_branch_block_apart  257 x 517 x 8, offdiag 0.2, un-normalised rows at inv_tau 10, groups
        (i, i + 128).
Backward (BWD_CASES) at inv_tau 1 / 0.07, g = 1 / bq, lse = the masked reference's rounded to fp32:
  fp32 130 x 300 x 36 and bf16 130 x 300 x 72 (materialised dS); bf16 fused 200 x 200 x 128 with
  groups (i, i + 64) and (i, i + 128) (a mate in another 64-row swept tile and another 128-row own
  block, for both roles) and 40 x 40 x 256 with groups of two; the same two with infonce_flash = 0.
Symmetric (SYM_CASES): 200 x 200 fp32 h 36 and bf16 h 128 (fused, and infonce_flash = 0) with the
  200 x 200 pattern; the lse_col of columns 160..191, whose mates 32..63 sit in the other 128-row
  block, is checked on its own: the column-partial merge.
Workspaces are *_ws_size bytes of 0xFF followed by a guard, outputs are pre-filled with NaN, and
every case runs twice with identical bits.

Tolerances: loss_ref.infonce_fwd_errs and infonce_bwd_errs unchanged. The bf16 per-row backward
bound is twice the per-row error of the masked reference with dS rounded to bf16 against the
unrounded one (groups_cases.masked_bwd_bound / masked_sym_bound), computed on the CPU.

NULL ids and all -1 ids give the bits of the ungrouped entry point, for every kernel family; one
NULL id pointer is TTError with the poisoned outputs untouched.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import groups_cases as G  # noqa: E402
from oracle import loss_ref as L  # noqa: E402
from oracle.loss_ref import BF16, F32, INV_TAU  # noqa: E402
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import TTError, call, dtype_code, option, stream_ptr  # noqa: E402

DEV = "cuda"
GUARD = 256


def _poisoned(nbytes):
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    ws[:nbytes] = 0xFF
    ws[nbytes:] = 0xA5
    return ws


def _guard_ok(ws, nbytes):
    return bool((ws[nbytes:] == 0xA5).all())


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert L.bits_differ(x, y)[0] == 0, what


# ------------------------------------------------------------------------------ runners
def run_fwd(q, d, inv_tau, offdiag, lab0, rg, cg, entry="grp"):
    """tt_infonce_fwd_grp (entry "grp"; rg, cg may be None) or tt_infonce_fwd ("plain"), twice on
    poisoned workspaces with identical bits. Returns (lse, row_loss) on the CPU."""
    lib = _lib.load()
    (bq, h), nd = q.shape, d.shape[0]
    qd, dd = q.to(DEV).contiguous(), d.to(DEV).contiguous()
    rgd, cgd = (None if t is None else t.to(DEV) for t in (rg, cg))
    n = lib.tt_infonce_fwd_ws_size(bq, nd)
    outs = []
    for _ in range(2):
        lse, row, ws = _nan(bq), _nan(bq), _poisoned(n)
        if entry == "grp":
            call("tt_infonce_fwd_grp", dtype_code(q.dtype), qd.data_ptr(), bq, dd.data_ptr(), nd, h, inv_tau, offdiag,
                 lab0, _p(rgd), _p(cgd), lse.data_ptr(), row.data_ptr(), ws.data_ptr(), stream_ptr())
        else:
            call("tt_infonce_fwd", dtype_code(q.dtype), qd.data_ptr(), bq, dd.data_ptr(), nd, h, inv_tau, offdiag,
                 lab0, lse.data_ptr(), row.data_ptr(), ws.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        assert _guard_ok(ws, n), "wrote past tt_infonce_fwd_ws_size"
        outs.append((lse.cpu(), row.cpu()))
    _same_bits(outs[0], outs[1], "two forward runs differ")
    return outs[0]


def run_bwd(q, d, inv_tau, offdiag, lab0, rg, cg, lse, g, flash, entry="grp"):
    lib = _lib.load()
    (bq, h), nd = q.shape, d.shape[0]
    dtc = dtype_code(q.dtype)
    qd, dd, lsed = q.to(DEV).contiguous(), d.to(DEV).contiguous(), lse.to(DEV)
    rgd, cgd = (None if t is None else t.to(DEV) for t in (rg, cg))
    gdev = torch.tensor([g], dtype=torch.float32, device=DEV)
    outs = []
    with option("infonce_flash", flash):
        n = lib.tt_infonce_bwd_ws_size(dtc, bq, nd, h)
        for _ in range(2):
            ws, dq, ddn = _poisoned(n), _nan(bq, h), _nan(nd, h)
            if entry == "grp":
                call("tt_infonce_bwd_grp", dtc, qd.data_ptr(), bq, dd.data_ptr(), nd, h, inv_tau, offdiag, lab0,
                     _p(rgd), _p(cgd), lsed.data_ptr(), gdev.data_ptr(), dq.data_ptr(), ddn.data_ptr(), ws.data_ptr(),
                     stream_ptr())
            else:
                call("tt_infonce_bwd", dtc, qd.data_ptr(), bq, dd.data_ptr(), nd, h, inv_tau, offdiag, lab0,
                     lsed.data_ptr(), gdev.data_ptr(), dq.data_ptr(), ddn.data_ptr(), ws.data_ptr(), stream_ptr())
            torch.cuda.synchronize()
            assert _guard_ok(ws, n), "wrote past tt_infonce_bwd_ws_size"
            outs.append((dq.cpu(), ddn.cpu()))
    _same_bits(outs[0], outs[1], "two backward runs differ")
    return outs[0]


def run_sym(q, d, inv_tau, grp, g, flash, entry="grp", lse=None):
    """Symmetric forward + backward, twice. lse: (lse_row, lse_col) handed to the backward
    (default: the forward's own). Returns (lse_row, lse_col, row_loss, dq, dd)."""
    lib = _lib.load()
    n, h = q.shape
    dtc = dtype_code(q.dtype)
    qd, dd = q.to(DEV).contiguous(), d.to(DEV).contiguous()
    gd = None if grp is None else grp.to(DEV)
    gdev = torch.tensor([g], dtype=torch.float32, device=DEV)
    outs = []
    nf = lib.tt_infonce_sym_fwd_ws_size(n, h)
    with option("infonce_flash", flash):
        nb = lib.tt_infonce_sym_bwd_ws_size(dtc, n, h)
        for _ in range(2):
            lr, lc, row, dq, ddn = _nan(n), _nan(n), _nan(n), _nan(n, h), _nan(n, h)
            wf, wb = _poisoned(nf), _poisoned(nb)
            if entry == "grp":
                call("tt_infonce_sym_fwd_grp", dtc, qd.data_ptr(), dd.data_ptr(), n, h, inv_tau, _p(gd), lr.data_ptr(),
                     lc.data_ptr(), row.data_ptr(), wf.data_ptr(), stream_ptr())
            else:
                call("tt_infonce_sym_fwd", dtc, qd.data_ptr(), dd.data_ptr(), n, h, inv_tau, lr.data_ptr(),
                     lc.data_ptr(), row.data_ptr(), wf.data_ptr(), stream_ptr())
            blr, blc = (lr, lc) if lse is None else (lse[0].to(DEV), lse[1].to(DEV))
            if entry == "grp":
                call("tt_infonce_sym_bwd_grp", dtc, qd.data_ptr(), dd.data_ptr(), n, h, inv_tau, _p(gd), blr.data_ptr(),
                     blc.data_ptr(), gdev.data_ptr(), dq.data_ptr(), ddn.data_ptr(), wb.data_ptr(), stream_ptr())
            else:
                call("tt_infonce_sym_bwd", dtc, qd.data_ptr(), dd.data_ptr(), n, h, inv_tau, blr.data_ptr(),
                     blc.data_ptr(), gdev.data_ptr(), dq.data_ptr(), ddn.data_ptr(), wb.data_ptr(), stream_ptr())
            torch.cuda.synchronize()
            assert _guard_ok(wf, nf) and _guard_ok(wb, nb), "wrote past a symmetric workspace"
            outs.append(tuple(t.cpu() for t in (lr, lc, row, dq, ddn)))
    _same_bits(outs[0], outs[1], "two symmetric runs differ")
    return outs[0]


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name,dt", [(n, dt) for n, c in G.FWD_CASES.items() for dt in c[2]])
def test_grouped_fwd_rows_match_masked_float64(name, dt):
    _, _, _, lab0, offdiag, _, _, _ = G.FWD_CASES[name]
    q, d, rg, cg, per_tau = G.fwd_case(name, dt)
    for inv_tau, (rlse, rrow, _, _, smax) in per_tau.items():
        lse, row = run_fwd(q, d, inv_tau, offdiag, lab0, rg, cg)
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(row).all()), "NaN / inf in the forward"
        L.check(f"grouped fwd {name} {dt} inv_tau {inv_tau:.3g}", L.infonce_fwd_errs(lse, row, rlse, rrow, dt, smax))


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize("dt,bq,nd,h,lab0,offdiag,flash,pattern",
                         [(*c[:6], f, c[7]) for c in G.BWD_CASES for f in c[6]])
def test_grouped_bwd_rows_match_masked_float64(dt, bq, nd, h, lab0, offdiag, flash, pattern):
    q, d, rg, cg, g, lse, rq, rd, bounds, _, _ = G.bwd_case(dt, bq, nd, h, lab0, offdiag, pattern)
    what = f"grouped bwd {dt} {bq} x {nd} x {h} flash {flash}"
    dq, dd = run_bwd(q, d, INV_TAU, offdiag, lab0, rg, cg, lse, g, flash)
    errs = L.infonce_bwd_errs(dq, dd, rq, rd, dt, bounds)
    print(f"{what}: " + ", ".join(f"{n} {e:.3g} (bound {b:.3g})" for n, e, _, b in errs))
    L.check(what, errs)


# ---------------------------------------------------------------------------- symmetric
@pytest.mark.parametrize("dt,n,h,flash", [(*c[:3], f) for c in G.SYM_CASES for f in c[3]])
def test_grouped_sym_matches_masked_float64(dt, n, h, flash):
    q, d, grp, g, (rlr, rlc, rrow, rq, rd), bounds, _ = G.sym_case(dt, n, h)
    what = f"grouped sym {dt} {n} x {h} flash {flash}"
    # the backward is judged alone: it gets the masked reference's LSE vectors rounded to fp32
    lr, lc, row, dq, dd = run_sym(q, d, G.SYM_INV_TAU, grp, g, flash, lse=(rlr.float(), rlc.float()))
    L.check(what + " rows", L.infonce_fwd_errs(lr, row, rlr, rrow, dt))
    L.check(what + " columns", L.infonce_fwd_errs(lc, row, rlc, rrow, dt))
    far = slice(160, 192)  # columns whose mates 32..63 belong to the other 128-row block
    L.check(what + " columns 160..191", L.infonce_fwd_errs(lc[far], row[far], rlc[far], rrow[far], dt))
    errs = L.infonce_bwd_errs(dq, dd, rq, rd, dt, bounds)
    print(f"{what}: " + ", ".join(f"{n_} {e:.3g} (bound {b:.3g})" for n_, e, _, b in errs))
    L.check(what, errs)


# ------------------------------------------------- NULL ids, all -1 ids, exactly one NULL
@pytest.mark.parametrize("name,dt", [("threes_other_tile", F32), ("threes_other_tile", BF16),
                                     ("margin_branch_block_apart", BF16)])
def test_fwd_null_and_negative_ids_are_the_ungrouped_bits(name, dt):
    _, _, _, lab0, offdiag, _, taus, _ = G.FWD_CASES[name]
    q, d, rg, cg, _ = G.fwd_case(name, dt)
    plain = run_fwd(q, d, taus[-1], offdiag, lab0, None, None, entry="plain")
    assert bool(torch.isfinite(plain[0]).all())
    _same_bits(run_fwd(q, d, taus[-1], offdiag, lab0, None, None), plain, "NULL ids")
    _same_bits(run_fwd(q, d, taus[-1], offdiag, lab0, torch.full_like(rg, -1), torch.full_like(cg, -7)), plain,
               "negative ids")
    # ids >= 0 on the columns alone exclude nothing either
    _same_bits(run_fwd(q, d, taus[-1], offdiag, lab0, torch.full_like(rg, -1), cg), plain, "row ids -1")


@pytest.mark.parametrize("dt,bq,nd,h,lab0,offdiag,flash,pattern",
                         [(*c[:6], f, c[7]) for c in G.BWD_CASES for f in c[6]])
def test_bwd_null_and_negative_ids_are_the_ungrouped_bits(dt, bq, nd, h, lab0, offdiag, flash, pattern):
    q, d, rg, cg, g, _, _, _, _, _, _ = G.bwd_case(dt, bq, nd, h, lab0, offdiag, pattern)
    lse = L.infonce_fwd_ref(q, d, INV_TAU, offdiag, lab0)[0].float()
    plain = run_bwd(q, d, INV_TAU, offdiag, lab0, None, None, lse, g, flash, entry="plain")
    assert bool(torch.isfinite(plain[0]).all()) and bool(torch.isfinite(plain[1]).all())
    _same_bits(run_bwd(q, d, INV_TAU, offdiag, lab0, None, None, lse, g, flash), plain, "NULL ids")
    _same_bits(run_bwd(q, d, INV_TAU, offdiag, lab0, torch.full_like(rg, -1), torch.full_like(cg, -1), lse, g, flash),
               plain, "negative ids")


@pytest.mark.parametrize("dt,n,h,flash", [(*c[:3], f) for c in G.SYM_CASES for f in c[3]])
def test_sym_null_and_negative_ids_are_the_ungrouped_bits(dt, n, h, flash):
    q, d, grp, g, _, _, _ = G.sym_case(dt, n, h)
    plain = run_sym(q, d, G.SYM_INV_TAU, None, g, flash, entry="plain")
    assert all(bool(torch.isfinite(t).all()) for t in plain)
    _same_bits(run_sym(q, d, G.SYM_INV_TAU, None, g, flash), plain, "NULL ids")
    _same_bits(run_sym(q, d, G.SYM_INV_TAU, torch.full_like(grp, -1), g, flash), plain, "negative ids")


@pytest.mark.parametrize("dt,h", [(F32, 36), (BF16, 128)])
def test_exactly_one_null_id_pointer_is_einval_before_any_launch(dt, h):
    lib = _lib.load()
    bq, nd, lab0 = 130, 300, 170
    dtc = dtype_code(dt)
    q, d = torch.zeros(bq, h, dtype=dt, device=DEV), torch.zeros(nd, h, dtype=dt, device=DEV)
    rg, cg = torch.zeros(bq, dtype=torch.int32, device=DEV), torch.zeros(nd, dtype=torch.int32, device=DEV)
    zl = torch.zeros(bq, device=DEV)
    for a, b in ((rg, None), (None, cg)):
        nf = lib.tt_infonce_fwd_ws_size(bq, nd)
        lse, row, ws = _nan(bq), _nan(bq), _poisoned(nf)
        with pytest.raises(TTError, match="row_group and col_group"):
            call("tt_infonce_fwd_grp", dtc, q.data_ptr(), bq, d.data_ptr(), nd, h, 1.0, 0.0, lab0, _p(a), _p(b),
                 lse.data_ptr(), row.data_ptr(), ws.data_ptr(), stream_ptr())
        nb = lib.tt_infonce_bwd_ws_size(dtc, bq, nd, h)
        dq, dd, wb = _nan(bq, h), _nan(nd, h), _poisoned(nb)
        with pytest.raises(TTError, match="row_group and col_group"):
            call("tt_infonce_bwd_grp", dtc, q.data_ptr(), bq, d.data_ptr(), nd, h, 1.0, 0.0, lab0, _p(a), _p(b),
                 zl.data_ptr(), None, dq.data_ptr(), dd.data_ptr(), wb.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        for t in (lse, row, dq, dd):
            assert bool(torch.isnan(t).all()), "an output was written"
        assert bool((ws[:nf] == 0xFF).all()) and bool((wb[:nb] == 0xFF).all()), "a workspace was written"


def test_grouped_entry_points_keep_the_ungrouped_argument_checks():
    """labels outside [0, nd), a misaligned h and a null workspace are TTError as in the
    ungrouped calls, before anything is launched."""
    bq, nd, h = 8, 40, 8
    q, d = torch.zeros(bq, h, device=DEV), torch.zeros(nd, h, device=DEV)
    rg, cg = torch.zeros(bq, dtype=torch.int32, device=DEV), torch.zeros(nd, dtype=torch.int32, device=DEV)
    ws = _poisoned(1 << 16)
    for lab0, hh, w, msg in ((33, h, ws, "labels"), (0, 6, ws, "misaligned"), (0, h, None, "workspace")):
        lse, row, dq, dd = _nan(bq), _nan(bq), _nan(bq, h), _nan(nd, h)
        with pytest.raises(TTError, match=msg):
            call("tt_infonce_fwd_grp", 0, q.data_ptr(), bq, d.data_ptr(), nd, hh, 1.0, 0.0, lab0, rg.data_ptr(),
                 cg.data_ptr(), lse.data_ptr(), row.data_ptr(), _p(w), stream_ptr())
        with pytest.raises(TTError, match=msg):
            call("tt_infonce_bwd_grp", 0, q.data_ptr(), bq, d.data_ptr(), nd, hh, 1.0, 0.0, lab0, rg.data_ptr(),
                 cg.data_ptr(), lse.data_ptr(), None, dq.data_ptr(), dd.data_ptr(), _p(w), stream_ptr())
        torch.cuda.synchronize()
        for t in (row, dq, dd):
            assert bool(torch.isnan(t).all())
    assert bool((ws[:1 << 16] == 0xFF).all())


# ------------------------------------------------------------------ tt_topk_drop_groups
def _drop(idx_in, val_in, lab0, rg, cg, nd, k, want_val=True, want_nkept=True):
    rows, kin = idx_in.shape
    ii = idx_in.to(DEV, torch.int32).contiguous()
    vi = None if val_in is None else val_in.to(DEV, torch.float32).contiguous()
    idx = torch.full((rows, k), -12345, dtype=torch.int32, device=DEV)
    val = _nan(rows, k) if want_val and vi is not None else None
    nk = torch.full((rows,), -1, dtype=torch.int32, device=DEV) if want_nkept else None
    rgd, cgd = rg.to(DEV), cg.to(DEV)  # held until the synchronise below
    call("tt_topk_drop_groups", ii.data_ptr(), _p(vi), rows, kin, lab0, rgd.data_ptr(), cgd.data_ptr(),
         nd, k, idx.data_ptr(), _p(val), _p(nk), stream_ptr())
    torch.cuda.synchronize()
    return idx.cpu(), None if val is None else val.cpu(), None if nk is None else nk.cpu()


def test_topk_drop_groups_hand_built():
    """nd 12, label_offset 4 (labels 4..8). Columns 0, 1, 2 and the label 5 carry id 7.
      row 0, no group: everything kept, in order.
      row 1, group 7, label 5: mates 0, 1, 2 dropped, the label 5 kept (never excluded).
      row 2, group 7, label 6: mates 0, 1, 2 AND 5 dropped (5 is not its label); 2 kept < k 3:
             the last kept entry repeats.
      row 3, group 7, candidates all mates: nothing kept: the label column 7 with value -1.
      row 4, group 9 that no column carries: everything kept."""
    nd, lab0, k = 12, 4, 3
    cg = torch.tensor([7, 7, 7, -1, -1, 7, -1, -1, -1, -1, -1, -1], dtype=torch.int32)
    rg = torch.tensor([-1, 7, 7, 7, 9], dtype=torch.int32)
    idx_in = torch.tensor([[0, 1, 2, 3, 9], [0, 5, 1, 9, 2], [0, 5, 10, 1, 11], [0, 1, 2, 5, 0], [2, 1, 0, 5, 3]])
    val_in = torch.tensor([[.9, .8, .7, .6, .5]]).repeat(5, 1) + torch.arange(5)[:, None]
    idx, val, nk = _drop(idx_in, val_in, lab0, rg, cg, nd, k)
    assert idx.tolist() == [[0, 1, 2], [5, 9, 9], [10, 11, 11], [7, 7, 7], [2, 1, 0]]
    assert nk.tolist() == [3, 2, 2, 0, 3]
    pos = [[0, 1, 2], [1, 3, 3], [2, 4, 4], None, [0, 1, 2]]  # where each output came from in its row
    want = torch.stack([torch.full((k,), -1.0) if p is None else val_in[r, p] for r, p in enumerate(pos)])
    assert L.bits_differ(val, want)[0] == 0
    assert int(idx.min()) >= 0 and int(idx.max()) < nd
    # without values and without nkept: the same indices
    idx2, _, _ = _drop(idx_in, None, lab0, rg, cg, nd, k, want_val=False, want_nkept=False)
    assert torch.equal(idx, idx2)
    # candidates outside [0, nd) are dropped; label_offset < 0 and nothing kept: column 0
    bad = torch.tensor([[-1, 12, 99, 3, 4]])
    idx3, _, nk3 = _drop(bad, None, lab0, rg[:1], cg, nd, k)
    assert idx3.tolist() == [[3, 4, 4]] and nk3.tolist() == [2]
    idx4, _, nk4 = _drop(torch.tensor([[0, 1, 2]]), None, -1, rg[1:2], cg, nd, 2)
    assert idx4.tolist() == [[0, 0]] and nk4.tolist() == [0]


def test_topk_drop_groups_long_lists_keep_order():
    """kin 150 spans three 64-candidate passes of the wave; rows of every residue drop a
    different third of the candidates; 130 rows = more than one workgroup of four."""
    rows, kin, nd, k = 130, 150, 400, 97
    gen = torch.Generator().manual_seed(3)
    idx_in = torch.stack([torch.randperm(nd, generator=gen)[:kin] for _ in range(rows)]).to(torch.int32)
    val_in = torch.rand(rows, kin, generator=gen)
    cg = (torch.arange(nd) % 3).to(torch.int32)
    rg = (torch.arange(rows) % 4 - 1).to(torch.int32)  # -1, 0, 1, 2
    idx, val, nk = _drop(idx_in, val_in, 0, rg, cg, nd, k)
    for r in range(rows):
        keep = [(int(c), float(v)) for c, v in zip(idx_in[r], val_in[r])
                if not (int(c) != r and int(rg[r]) >= 0 and int(cg[int(c)]) == int(rg[r]))]
        n = min(len(keep), k)
        want = keep[:k] + [keep[n - 1]] * (k - n)
        assert int(nk[r]) == n
        assert idx[r].tolist() == [c for c, _ in want], r
        assert val[r].tolist() == [v for _, v in want], r
    assert int(idx.min()) >= 0 and int(idx.max()) < nd


def test_topk_drop_groups_argument_checks():
    z = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    for args, msg in (((z.data_ptr(), None, 2, 2, 0, z.data_ptr(), z.data_ptr(), 4, 3, out.data_ptr(), None, None), "k="),
                      ((z.data_ptr(), None, 2, 2, 3, z.data_ptr(), z.data_ptr(), 4, 1, out.data_ptr(), None, None), "labels"),
                      ((z.data_ptr(), None, 2, 2, 0, None, z.data_ptr(), 4, 1, out.data_ptr(), None, None), "null")):
        with pytest.raises(TTError, match=msg):
            call("tt_topk_drop_groups", *args, stream_ptr())
    call("tt_topk_drop_groups", z.data_ptr(), None, 0, 2, 0, z.data_ptr(), z.data_ptr(), 4, 1, out.data_ptr(), None, None,
         stream_ptr())  # rows = 0: a no-op
    torch.cuda.synchronize()
    assert out.tolist() == [-5] * 4
