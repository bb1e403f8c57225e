"""tt_gru_fwd and tt_gru_bwd, called directly, against the float64 reference of one recurrence
(oracle/gru_ref.py), value by value and row by row, in every kernel family.

The other GRU tests compare the forward families with each other (bit for bit) and see the
backward only through parameter gradients of a whole model, which are sums over all B*T rows.
Here every output row is measured against its own scale (oracle.gru_ref.row_err), so one wrong
batch row of a tail tile, one wrong 8-unit column group or a dropped final-state gradient
fails (tests/test_gru_ref.py shows the checker reads such faults at 0.2 and above).

Every case uses the product's layout (ldg 6H, ldy 2H, ldd 8H, ldf 2H, the two directions of
a tower side by side), asserts from the launch counts which family ran, and checks that the
row after B*T and the columns of a direction that is not part of the call keep a sentinel.
Forward: Y, the four blocks of the saved state S, and the dropout copy X1 (zero pattern
exactly oracle.cpu_ref.dropout_mask, drop_row0 != 0, one seed per tower). Backward, on S and Y
taken from the reference so that a forward fault cannot mask or cause a failure: dgx (the 3H
columns dar | daz | dan as one row), dgh (dhn), and the bias partial sums over the
tt_gru_bias_rows(B) rows of a buffer prefilled with 1e30; with dy alone, dfinal alone and both
(the last is in the ABI and in no product path).

Tolerances, per row: fp32 1e-4, bf16 2e-2 against the rounding-emulating reference.
Largest per-row errors measured on an MI355X (fixed seeds; the kernels are deterministic):
  forward (Y, S blocks, X1)          fp32      bf16
    per-step, 128-row tiles          4.2e-7    -
    per-step, 256-row tiles          3.3e-7    4.4e-3
    per-step, 3-stage ring           3.6e-7    5.4e-3
    per-step at H 1024               -         5.1e-3
    row-owning, depth 1 / 2 / 4      -         4.6e-3 (the three depths read the same)
    column-split, both forms         -         5.4e-3
  backward (dgx, dgh, bias sums)     fp32      bf16
    step, 64-row tiles               9.9e-7    1.34e-2
    step, 128-row tiles              8.8e-7    1.09e-2
    step, one chain and two          -         9.4e-3 (both read the same)
    step, 3-stage ring               6.3e-7    -
    256 x 256 tiles                  -         1.35e-2
    row-owning H 256 / 512 / 1024    -         1.54e-2 / 1.46e-2 / 1.11e-2
In bf16 7.8e-3 is one flipped last bit of a row's largest element; what lies above it comes
with dfinal (T = 4) and is the BPTT carry dh*z, which the kernels hold in bf16 (tt_gru_bwd_rec
dhstate "of dtype"; the row-owning kernel also stages the product as a bf16 image) and the
reference leaves unrounded: the float64 reference with only the carry rounded to bf16
reproduces the step kernels' figures in the same rows (checked at H 8, 136 and 256). dar and
daz measured against their own row scale instead of the whole dgx row's (printed, not
asserted) read up to 2.15e-2 for the same reason (H 8, where a row has 8 elements and its
largest can be a cancelled one).
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cpu_ref import dropout_mask  # noqa: E402
from oracle.gru_ref import dropout_err, gru_bwd_ref, gru_fwd_ref, row_err, vec_err  # noqa: E402
from two_towers_amd import _lib  # noqa: E402
from two_towers_amd._lib import GruBwdRec, GruFwdRec, call, get_option, option, stream_ptr  # noqa: E402
from two_towers_amd.towers import gru_fwd_workspace  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 1e-4, BF16: 2e-2}
SENT = -777.0
DROP_P, DROP_ROW0 = 0.1, 5
MODES = ("dy", "dfinal", "both")


@contextlib.contextmanager
def options(**kw):
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(option(k, v))
        yield


def _q(x, dt):
    return x.to(dt).double()


def _recmap(nrec, d0):
    """(tower, direction) of every record: towers of two directions, or one direction alone."""
    return [(0, d0)] if nrec == 1 else [(i // 2, i % 2) for i in range(nrec)]


@functools.lru_cache(maxsize=None)
def _ref(dt, H, B, T, ntow, seed):
    """Inputs (rounded to dt) and the reference forward per tower and direction, computed once
    per shape and shared by the forward and backward cases."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(ntow):
        G = torch.randn(B * T, 6 * H, generator=g).to(dt)
        whh = [(torch.randn(3 * H, H, generator=g) * H ** -0.5).to(dt) for _ in range(2)]
        bhn = [torch.randn(H, generator=g) * 0.5 for _ in range(2)]
        dY = torch.randn(B * T, 2 * H, generator=g).to(dt)
        dF = torch.randn(B, 2 * H, generator=g)
        fwd = [gru_fwd_ref(G[:, d * 3 * H:(d + 1) * 3 * H], whh[d], bhn[d], B, T, H, bool(d), dt) for d in range(2)]
        out.append(dict(G=G, whh=whh, bhn=bhn, dY=dY, dF=dF, fwd=fwd))
    return out


@functools.lru_cache(maxsize=None)
def _bwd_ref(dt, H, B, T, ntow, seed, mode, ti, d):
    r = _ref(dt, H, B, T, ntow, seed)[ti]
    Y, S = r["fwd"][d]
    dY = r["dY"][:, d * H:(d + 1) * H] if mode != "dfinal" else None
    dF = r["dF"][:, d * H:(d + 1) * H] if mode != "dy" else None
    return gru_bwd_ref(_q(S, dt), _q(Y, dt), dY, dF, r["whh"][d], B, T, H, bool(d), dt)


def _report(what, errs, tol):
    """Print every figure, then assert: a failure still shows the whole measurement."""
    worst = max(errs, key=lambda e: e[1])
    print(f"{what}: worst per-row error {worst[1]:.3g} ({worst[0]} at {worst[2]})")
    for name, e, idx in errs:
        assert e <= tol, f"{what}: {name} per-row error {e:.3g} > {tol:g} at {idx}"


def _sentinel_kept(t):
    return bool((t == SENT).all())


def _check_fwd(dt, H, B, T, nrec, persistent, use_ws=False, d0=0):
    lib = _lib.load()
    dtc, BT = _lib.dtype_code(dt), B * T
    recmap = _recmap(nrec, d0)
    ntow = (nrec + 1) // 2
    ref = _ref(dt, H, B, T, ntow, 1000 * H + 10 * B + T)
    # which family: 1 launch (persistent kernels) or one per step; asked for >= 2 steps so
    # that T = 1 cases tell the two apart as well
    Tq = max(T, 2)
    if use_ws:
        assert lib.tt_gru_fwd_launches_for(dtc, nrec, B, Tq, H, 6 * H, 2 * H) == 1
    else:
        assert lib.tt_gru_fwd_launches(dtc, Tq, H) == (1 if persistent else Tq)
    G = [r["G"].to(DEV) for r in ref]
    whh = [[w.to(DEV) for w in r["whh"]] for r in ref]
    bhn = [[b.to(DEV) for b in r["bhn"]] for r in ref]
    Y = [torch.full((BT + 1, 2 * H), SENT, dtype=dt, device=DEV) for _ in range(ntow)]
    X1 = [torch.full((BT + 1, 2 * H), SENT, dtype=dt, device=DEV) for _ in range(ntow)]
    S = [torch.full((BT, 4 * H), SENT, dtype=dt, device=DEV) for _ in range(nrec)]
    hs = torch.zeros(nrec, 2, B, H, dtype=torch.float32, device=DEV)
    seeds = [911 + 17 * ti for ti in range(ntow)]
    recs = (GruFwdRec * nrec)()
    for i, (ti, d) in enumerate(recmap):
        r = recs[i]
        r.g, r.whh, r.bhn = G[ti][:, d * 3 * H:].data_ptr(), whh[ti][d].data_ptr(), bhn[ti][d].data_ptr()
        r.y, r.x1, r.save = Y[ti][:, d * H:].data_ptr(), X1[ti][:, d * H:].data_ptr(), S[i].data_ptr()
        r.hstate, r.dir = hs[i].data_ptr(), d
        r.drop_seed, r.drop_col0, r.drop_row0 = seeds[ti], d * H, DROP_ROW0
    ws = gru_fwd_workspace(nrec, B, T, H, dt, torch.device(DEV)) if use_ws else None
    assert (ws is not None) == use_ws, "the column-split kernel does not apply to this shape"
    call("tt_gru_fwd", dtc, recs, nrec, B, T, H, 6 * H, 2 * H, DROP_P,
         ws.data_ptr() if use_ws else None, ws.numel() if use_ws else 0, stream_ptr())
    torch.cuda.synchronize()
    if use_ws:
        assert int(ws[:4].view(torch.int32).item()) == 0, "a column-split member wait timed out"
    errs = []
    for i, (ti, d) in enumerate(recmap):
        Yr, Sr = ref[ti]["fwd"][d]
        tag = f"tower {ti} dir {d} "
        errs.append((tag + "Y", *row_err(Y[ti][:BT, d * H:(d + 1) * H].reshape(B, T, H), _q(Yr, dt))))
        Sg = S[i].reshape(B, T, 4 * H)
        for k, name in enumerate(("ar", "az", "an", "ghn")):
            errs.append((tag + name, *row_err(Sg[:, :, k * H:(k + 1) * H], _q(Sr[:, :, k * H:(k + 1) * H], dt))))
        mult = dropout_mask(seeds[ti], BT, 2 * H, DROP_P, row0=DROP_ROW0)[:, d * H:(d + 1) * H].astype(np.float64)
        wrong, e = dropout_err(X1[ti][:BT, d * H:(d + 1) * H].reshape(B, T, H), Yr, torch.from_numpy(mult).reshape(B, T, H))
        assert wrong == 0, f"{tag}X1: {wrong} elements differ from the dropout mask's zero pattern"
        errs.append((tag + "X1", *e))
    for ti in range(ntow):
        for name, buf in (("Y", Y[ti]), ("X1", X1[ti])):
            assert _sentinel_kept(buf[BT]), f"{name}: the row after B*T was written"
            for d in range(2):
                if (ti, d) not in recmap:
                    assert _sentinel_kept(buf[:, d * H:(d + 1) * H]), f"{name}: columns of direction {d} were written"
    _report(f"fwd {dt} H {H} B {B} T {T} nrec {nrec}", errs, TOL[dt])


def _check_bwd(dt, H, B, T, nrec, persistent, d0=0):
    """The three modes of one family on one shape."""
    lib = _lib.load()
    dtc, BT = _lib.dtype_code(dt), B * T
    recmap = _recmap(nrec, d0)
    ntow = (nrec + 1) // 2
    seed = 1000 * H + 10 * B + T
    ref = _ref(dt, H, B, T, ntow, seed)
    Tq = max(T, 2)
    assert lib.tt_gru_bwd_launches(dtc, Tq, H) == (1 if persistent else Tq)
    nbr = lib.tt_gru_bias_rows(B)
    assert nbr == (B + 63) // 64
    whh = [[w.to(DEV) for w in r["whh"]] for r in ref]
    Y = [torch.cat([r["fwd"][0][0], r["fwd"][1][0]], 2).reshape(BT, 2 * H).to(dt).to(DEV) for r in ref]
    S = [ref[ti]["fwd"][d][1].reshape(BT, 4 * H).to(dt).to(DEV) for ti, d in recmap]
    dY = [r["dY"].to(DEV) for r in ref]
    dF = [r["dF"].to(DEV) for r in ref]
    for mode in MODES:
        dG = [torch.full((BT + 1, 8 * H), SENT, dtype=dt, device=DEV) for _ in range(ntow)]
        dhs = torch.zeros(nrec, 2, B, H, dtype=dt, device=DEV)
        part = torch.full((nrec, nbr, 4 * H), 1e30, dtype=torch.float32, device=DEV)
        recs = (GruBwdRec * nrec)()
        for i, (ti, d) in enumerate(recmap):
            r = recs[i]
            r.save, r.y, r.whh = S[i].data_ptr(), Y[ti][:, d * H:].data_ptr(), whh[ti][d].data_ptr()
            r.dy = dY[ti][:, d * H:].data_ptr() if mode != "dfinal" else None
            r.dfinal = dF[ti][:, d * H:].data_ptr() if mode != "dy" else None
            r.dgx, r.dgh = dG[ti][:, d * 3 * H:].data_ptr(), dG[ti][:, 6 * H + d * H:].data_ptr()
            r.dhstate, r.dbias_part, r.dir = dhs[i].data_ptr(), part[i].data_ptr(), d
        call("tt_gru_bwd", dtc, recs, nrec, B, T, H, 2 * H, 8 * H, 2 * H, stream_ptr())
        torch.cuda.synchronize()
        errs, blocks = [], []
        for i, (ti, d) in enumerate(recmap):
            dgx, dgh, dbias = _bwd_ref(dt, H, B, T, ntow, seed, mode, ti, d)
            tag = f"tower {ti} dir {d} "
            got = dG[ti][:BT].reshape(B, T, 8 * H)
            gx = got[:, :, d * 3 * H:(d + 1) * 3 * H]
            errs.append((tag + "dgx", *row_err(gx, _q(dgx, dt))))
            errs.append((tag + "dgh", *row_err(got[:, :, 6 * H + d * H:6 * H + (d + 1) * H], _q(dgh, dt))))
            errs.append((tag + "dbias", *vec_err(part[i].double().sum(0), dbias)))
            # for the record only: dar and daz against their own row scale instead of the whole
            # dgx row's, which dan dominates (see the module docstring)
            for k, name in enumerate(("dar", "daz")):
                blocks.append(row_err(gx[:, :, k * H:(k + 1) * H], _q(dgx[:, :, k * H:(k + 1) * H], dt))[0])
        print(f"  (dar / daz alone, not asserted: {max(blocks):.3g})")
        for ti in range(ntow):
            assert _sentinel_kept(dG[ti][BT]), "the gradient row after B*T was written"
            for d in range(2):
                if (ti, d) not in recmap:
                    assert _sentinel_kept(dG[ti][:, d * 3 * H:(d + 1) * 3 * H]), f"dgx of direction {d} was written"
                    assert _sentinel_kept(dG[ti][:, 6 * H + d * H:6 * H + (d + 1) * H]), f"dgh of direction {d} was written"
        _report(f"bwd {mode} {dt} H {H} B {B} T {T} nrec {nrec}", errs, TOL[dt])


# ------------------------------------------------------------------------------ forward

@pytest.mark.parametrize("H,B,T,nrec,d0", [(8, 1, 1, 1, 1), (8, 130, 3, 2, 0), (72, 1, 3, 1, 0), (72, 130, 1, 4, 0),
                                           (72, 130, 3, 2, 0)])
def test_per_step_forward_128_row_tiles(H, B, T, nrec, d0):
    """gru_fwd_step<float, 128, 2>: H 8 (one 8-unit group, under one MFMA tile), H 72 (a second,
    8-wide unit tile), one batch row, two batch tiles with a 2-row tail, T = 1."""
    with options(gru_step=1, gru_fwd_step_rows=128, gru_step_ring=2):
        _check_fwd(F32, H, B, T, nrec, persistent=False, d0=d0)


@pytest.mark.parametrize("dt,nrec", [(F32, 2), (BF16, 4)])
def test_per_step_forward_256_row_tiles(dt, nrec):
    """gru_fwd_step<T, 256, 2> (512 threads): B 260 is one full tile and a 4-row tail."""
    with options(gru_step=1, gru_fwd_step_rows=256):
        _check_fwd(dt, 72, 260, 2, nrec, persistent=False)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_per_step_forward_three_stage_ring(dt):
    """gru_fwd_step<T, 128, 3>: taken when the grid is at most one workgroup per CU."""
    with options(gru_step=1, gru_fwd_step_rows=128, gru_step_ring=3):
        _check_fwd(dt, 72, 130, 3, 2, persistent=False)


def test_per_step_forward_is_the_route_at_h1024():
    """bf16 H 1024 under the default options: above the persistent kernels' 512 units."""
    _check_fwd(BF16, 1024, 130, 2, 2, persistent=False)


@pytest.mark.parametrize("H,T,nrec,d0,depth", [(64, 1, 1, 1, 4), (192, 3, 2, 0, 4), (320, 3, 4, 0, 4), (512, 3, 2, 0, 4),
                                               (512, 3, 2, 0, 2), (512, 3, 2, 0, 1), (512, 1, 1, 0, 4)])
def test_row_owning_forward(H, T, nrec, d0, depth):
    """gru_fwd_seq without a workspace: runtime K-tile counts (H 64, 192, 320: depth 1) and the
    fixed H 512 instances at depth 4 / 2 / 1; B 65 is one 64-row workgroup and a 1-row tail."""
    with options(gru_fwd_xc=0, gru_depth=depth):
        _check_fwd(BF16, H, 65, T, nrec, persistent=True, d0=d0)


@pytest.mark.parametrize("H,xs,nrec,d0", [(256, 1, 2, 0), (512, 1, 4, 0), (512, 0, 1, 1)])
def test_column_split_forward(H, xs, nrec, d0):
    """gru_fwd_xc = 2 forces the column-split kernels on a small batch (B 70: groups with few or
    no rows): gru_fwd_xcp at H 256, both forms at H 512 (gru_fwd_xs 1 / 0)."""
    with options(gru_fwd_xc=2, gru_fwd_xs=xs):
        _check_fwd(BF16, H, 70, 3, nrec, persistent=True, use_ws=True, d0=d0)


# ----------------------------------------------------------------------------- backward

@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("H,B,T,nrec,d0", [(8, 1, 1, 1, 1), (8, 65, 4, 2, 0), (136, 1, 4, 1, 0), (136, 65, 1, 2, 0),
                                           (136, 65, 4, 2, 0)])
def test_step_backward_64_row_tiles(dt, H, B, T, nrec, d0):
    """gru_bwd_step<T, 64>: H 136 is one 128-unit tile and an 8-unit one, B 65 a 1-row tail."""
    with options(gru_bwd_rows=64):
        _check_bwd(dt, H, B, T, nrec, persistent=False, d0=d0)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("H", [136, 256])
def test_step_backward_128_row_tiles(dt, H):
    """gru_bwd_step<T, 128> on the two-stage product: B 130 is one tile and a 2-row tail, whose
    bias partials land in rows 0 and 1 of the three that tt_gru_bias_rows(130) counts."""
    with options(gru_bwd_rows=128, gru_bwd_persist=0, gru_bwd_big=0, gru_step_ring=2):
        _check_bwd(dt, H, 130, 4, 2, persistent=False)


@pytest.mark.parametrize("streams", [1, 2])
def test_step_backward_one_chain_and_two(streams):
    """Four recurrences on one chain of step launches (gru_bwd_streams = 1) and split over the
    caller's stream and the side stream (the default)."""
    assert get_option("gru_bwd_streams") == 2
    with options(gru_bwd_streams=streams):
        _check_bwd(BF16, 136, 130, 3, 4, persistent=False)


def test_step_backward_three_stage_ring():
    with options(gru_step_ring=3):
        _check_bwd(F32, 136, 65, 3, 2, persistent=False)


@pytest.mark.parametrize("H,nrec,d0", [(256, 2, 0), (512, 1, 1)])
def test_big_tile_backward(H, nrec, d0):
    """gru_bwd_big (256 x 256 tiles, one launch per step): B 257 is one tile and a 1-row tail;
    its bias partials go to the even rows of the five that tt_gru_bias_rows(257) counts."""
    assert get_option("gru_bwd_big") == 1
    with options(gru_bwd_rows=128, gru_bwd_persist=0):
        _check_bwd(BF16, H, 257, 3, nrec, persistent=False, d0=d0)


@pytest.mark.parametrize("H,T,nrec,d0,persist", [(256, 1, 2, 0, 1), (256, 4, 2, 0, 1), (512, 4, 4, 0, 1),
                                                 (1024, 1, 1, 1, 2), (1024, 4, 2, 0, 2)])
def test_row_owning_backward(H, T, nrec, d0, persist):
    """gru_bwd_rows<H>, one launch: the default at H 256 / 512 (carry on chip), and H 1024 in two
    column passes with gru_bwd_persist = 2 (carry through dhstate). B 130: a 2-row tail tile."""
    assert get_option("gru_bwd_persist") == 1 and get_option("gru_bwd_rows") == 0
    with options(gru_bwd_persist=persist):
        _check_bwd(BF16, H, 130, T, nrec, persistent=True, d0=d0)
